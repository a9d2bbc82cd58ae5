"""The C++ host layer's sylow::msm (include/sylow_hip.hpp) compiled with g++ and run on the GPU: equal to sylow::aggregate with one
job on both MSM routes, and the identity where the terms cancel or there are none."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "msm_host_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "msm_host_test")


def build_exe():
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-o", EXE,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_msm_compiles():
    """CPU: the wrapper builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    build_exe()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_msm_runs():
    build_exe()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    assert lines["MSM"] == "110"
    assert lines["IDENT"] == "11"
