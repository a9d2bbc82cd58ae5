"""The C ABI of the folded KZG openings called from C++ with raw device pointers (tests/cpp/kzg_multi_host_test.cpp), compiled with g++ and
run on the GPU: open five polynomials in the groups {3, 0, 2}, verify the folded rows, alter one claimed value, and compare the linear
combination with Horner over fr::mul and fr::add."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_multi_host_test.cpp")


def build_exe(exe):
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_kzg_multi_compiles(tmp_path):
    """CPU: the test builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    exe = str(tmp_path / "kzg_multi_host_test")
    build_exe(exe)
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_kzg_multi_runs(tmp_path):
    exe = str(tmp_path / "kzg_multi_host_test")
    build_exe(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    # every group verifies (the empty one: identity rows); y_4 + 1 fails the last group alone; both folded rows pass the cached verifier;
    # the empty group's row is (identity, 0, identity); lincomb == Horner; a group_start that ends short of m is E_ARG
    assert lines["MULTI"] == "111 110 11 111"
