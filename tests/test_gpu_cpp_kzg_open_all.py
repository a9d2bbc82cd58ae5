"""The C++ host layer's sylow::KzgProver::open_all (include/sylow_hip.hpp) compiled with g++ and run on the GPU at log_n = 4: the proofs
against KzgProver::open of the polynomial repeated, the values against fr::ntt, the flags of a constant, the capped grid, the verifier."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_open_all_host_test.cpp")


def build_exe(exe):
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_kzg_open_all_compiles(tmp_path):
    """CPU: the wrapper builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    exe = str(tmp_path / "kzg_open_all_host_test")
    build_exe(exe)
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_kzg_open_all_runs(tmp_path):
    exe = str(tmp_path / "kzg_open_all_host_test")
    build_exe(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    assert lines["OPENALL"] == "11111"
