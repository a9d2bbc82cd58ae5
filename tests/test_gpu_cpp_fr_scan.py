"""The C ABI of the scans over Fr and of PLONK's permutation grand product called from C++ with raw device pointers through
include/sylow_hip_fr_scan.h (tests/cpp/fr_scan_host_test.cpp), compiled with g++ and run on the GPU at log_n = 3, W = 2: the identity columns
and z against words baked in from tests/fr_scan_model.py, which this file re-derives on the CPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fr_scan_host_test.cpp")


def build_exe(exe):
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_fr_scan_compiles(tmp_path):
    """CPU: the test builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    exe = str(tmp_path / "fr_scan_host_test")
    build_exe(exe)
    assert os.path.exists(exe)


def test_the_baked_values_are_the_model_s():
    """CPU: the constants of the C++ source against tests/fr_scan_model.py"""
    import fr_scan_model as M
    src = open(SRC).read()

    def table(name):
        body = re.search(r"static const uint64_t " + name + r"\[\d+\]\[4\] = \{(.*?)\n\};", src, flags=re.S).group(1)
        rows = re.findall(r"\{([^{}]*)\}", body)
        return [sum(int(w.strip().rstrip("ul"), 0) << (64 * k) for k, w in enumerate(r.split(","))) for r in rows]

    shifts, log_n, n = [1, 5], 3, 8
    mapping = [p * 3 % 16 for p in range(16)]
    assert "shifts = {1, 5, 0, 0, 0, 0, 0, 0}" in src and "q = p * 3 % 16" in src and "1000 + 17 * cycle_of[p]" in src
    assert "beta = {0x1234567, 0, 0, 0}, gamma = {0x89ABCDEF, 0, 0, 0}" in src
    cycles = sorted(M.cycles(mapping), key=min)
    cycle_of = [next(c for c, cyc in enumerate(cycles) if p in cyc) for p in range(16)]
    assert "cycle_of[16] = {" + ", ".join(map(str, cycle_of)) + "}" in src
    flat = [1000 + 17 * c for c in cycle_of]
    wires = [flat[:n], flat[n:]]
    sigma = M.sigma_from_mapping(shifts, log_n, mapping)
    z, total, status = M.permutation(wires, sigma, shifts, 0x1234567, 0x89ABCDEF, log_n)
    assert table("IDENT") == [v for col in M.identity(shifts, log_n) for v in col] and table("Z") == z and (total, status) == (1, 0)
    assert "wires[3] += 1" in src and len(next(c for c in cycles if 3 in c)) == 4
    wires[0][3] += 1
    assert M.permutation(wires, sigma, shifts, 0x1234567, 0x89ABCDEF, log_n)[2] == 2


@pytest.mark.gpu
def test_cpp_fr_scan_runs(tmp_path):
    exe = str(tmp_path / "fr_scan_host_test")
    build_exe(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    # the identity columns and z are the model's, on the default form and the tuned one, with z_n = 1 and status 0; one changed wire gives
    # status 2; the running product of 1 .. 8 is the factorials and the exclusive sum the triangular numbers; the ratio scan telescopes;
    # W = 33, op = 2, totals_tile = 0 and an output over an input are E_ARG
    assert lines["FRSCAN"] == "1 1 1 1 1 1"
