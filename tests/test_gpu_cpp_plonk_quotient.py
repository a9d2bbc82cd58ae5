"""The C ABI of PLONK's quotient polynomial called from C++ with raw device pointers through include/sylow_plonk.h
(tests/cpp/plonk_quotient_host_test.cpp), compiled with g++ and run on the GPU at log_n = 3, W = 2, E = 4: the tail of the table and t against
words baked in from tests/plonk_quotient_model.py, which this file re-derives on the CPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "plonk_quotient_host_test.cpp")


def build_exe(exe):
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_plonk_quotient_compiles(tmp_path):
    """CPU: the test builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    exe = str(tmp_path / "plonk_quotient_host_test")
    build_exe(exe)
    assert os.path.exists(exe)


def test_the_baked_values_are_the_model_s():
    """CPU: the constants of the C++ source against tests/plonk_quotient_model.py"""
    import fr_scan_model as S
    import plonk_quotient_model as Q
    src = open(SRC).read()
    R = Q.R

    def table(name):
        body = re.search(r"static const uint64_t " + name + r"\[\d+\]\[4\] = \{(.*?)\n\};", src, flags=re.S).group(1)
        rows = re.findall(r"\{([^{}]*)\}", body)
        return [sum(int(w.strip().rstrip("ul"), 0) << (64 * k) for k, w in enumerate(r.split(","))) for r in rows]

    shifts, log_n, log_e, W, n = [1, 5], 3, 2, 2, 8
    mapping = [p * 3 % 16 for p in range(16)]
    assert "shifts = {1, 5, 0, 0, 0, 0, 0, 0}" in src and "q = p * 3 % 16" in src and "1000 + 17 * cycle_of[p]" in src
    assert "beta = {0x1234567, 0, 0, 0}, gamma = {0x89ABCDEF, 0, 0, 0}, alpha = {0x13579BDF, 0, 0, 0}" in src
    assert "= i + 1; " in src and "= 2 * i + 3; " in src and "= i + 2; " in src and "log_n = 3, log_e = 2, W = 2" in src
    cycles = sorted(S.cycles(mapping), key=min)
    cycle_of = [next(c for c, cyc in enumerate(cycles) if p in cyc) for p in range(16)]
    assert "cycle_of[16] = {" + ", ".join(map(str, cycle_of)) + "}" in src
    flat = [1000 + 17 * c for c in cycle_of]
    wires = [flat[:n], flat[n:]]
    q0, q1, qm = [i + 1 for i in range(n)], [2 * i + 3 for i in range(n)], [i + 2 for i in range(n)]
    qc = [-(qm[i] * wires[0][i] * wires[1][i] + q0[i] * wires[0][i] + q1[i] * wires[1][i]) % R for i in range(n)]
    assert table("QC") == qc
    sigma = S.sigma_from_mapping(shifts, log_n, mapping)
    beta, gamma, alpha = 0x1234567, 0x89ABCDEF, 0x13579BDF
    z, total, status = S.permutation(wires, sigma, shifts, beta, gamma, log_n)
    assert (total, status) == (1, 0)
    rows, zinv = Q.table([q0, q1, qm, qc], sigma, log_n, log_e)
    assert table("ZINV") == zinv
    wc, zc = [Q.coefficients(w, log_n) for w in wires], Q.coefficients(z, log_n)
    t, status = Q.quotient(rows, zinv, wc, zc, None, shifts, beta, gamma, alpha, log_n, log_e)
    d = Q.degree_bound(log_n, W, n, n)
    assert status == 0 and d == 21 < 32 and table("T") == t[:d - n + 1] and not any(t[d - n + 1:]) and "T[14][4]" in src
    # the exact quotient: the schoolbook route agrees
    quo, rem = Q.divide_by_vanishing(Q.numerator([q0, q1, qm, qc], sigma, wc, zc, None, shifts, beta, gamma, alpha, log_n), log_n)
    assert not any(rem) and quo == t[:len(quo)]
    assert "wires[3] += 1" in src
    wires[0][3] += 1
    assert Q.quotient(rows, zinv, [Q.coefficients(w, log_n) for w in wires], zc, None, shifts, beta, gamma, alpha, log_n, log_e)[1] == 1
    assert not Q.args_ok(log_n, log_e, W, n, 27) and "full(log_n, log_e, W, 27," in src


@pytest.mark.gpu
def test_cpp_plonk_quotient_runs(tmp_path):
    exe = str(tmp_path / "plonk_quotient_host_test")
    build_exe(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    # the tail of the table is the model's; z closes; t is the model's with status 0 on the default form and the tuned one; the fused kernel
    # alone between two transforms gives the same t; one changed wire gives status 1; W = 1 and 33, log_n + log_e = 29, len_z = 27,
    # max_blocks = 0 and t_out over the wires are E_ARG
    assert lines["PLONKQ"] == "1 1 1 1 1 1"
