"""The C ABI of the several-point KZG opening called from C++ with raw device pointers through include/sylow_hip_kzg_points.h
(tests/cpp/kzg_points_host_test.cpp), compiled with g++ and run on the GPU: open three polynomials at four points each under one proof per
polynomial, verify, alter one claimed value, repeat one point."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_points_host_test.cpp")


def build_exe(exe):
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_kzg_points_compiles(tmp_path):
    """CPU: the test builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    exe = str(tmp_path / "kzg_points_host_test")
    build_exe(exe)
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_kzg_points_runs(tmp_path):
    exe = str(tmp_path / "kzg_points_host_test")
    build_exe(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    # every row verifies; y[1][2] altered fails the middle row alone; a repeated point fails the last row alone; the quotient call's values are
    # the opening's; k = 0 and k = 65 are E_ARG
    assert lines["POINTS"] == "111 101 110 1 11"
