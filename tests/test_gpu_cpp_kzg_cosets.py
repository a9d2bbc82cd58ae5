"""The C ABI of the KZG proofs on every coset of the domain called from C++ with raw device pointers through include/sylow_hip_kzg_cosets.h
(tests/cpp/kzg_cosets_host_test.cpp), compiled with g++ and run on the GPU: prepare the table at (log_c, log_l) = (3, 2), open two polynomials
on their eight cosets, verify the sixteen rows, alter one cell value, move one row to another coset, name a coset out of range."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_cosets_host_test.cpp")


def build_exe(exe):
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_kzg_cosets_compiles(tmp_path):
    """CPU: the test builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    exe = str(tmp_path / "kzg_cosets_host_test")
    build_exe(exe)
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_kzg_cosets_runs(tmp_path):
    exe = str(tmp_path / "kzg_cosets_host_test")
    build_exe(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    # the pinned plan gives the same words and no proof is the identity; every row verifies; a value altered fails row 5 alone, another coset
    # fails row 9 alone, an index past c fails row 3 alone; log_c + log_l = 28 and planes_log = log_l + 1 are E_ARG
    assert lines["COSETS"] == "11 1 111 11"
