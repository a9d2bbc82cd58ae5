"""CPU: the model of the proofs at every point of the domain (tests/kzg_open_all_model.py).  The convolution route of kzg_open_all.hip, run
stage by stage on discrete logarithms, gives the quotients of synthetic division evaluated at tau -- for a random tau, a tau inside the
domain and a cube root of unity (an identity in the table) -- with as many products as the plan's formula says, and h_(n-1) = 0."""
import random

import pytest

import kzg_open_all_model as M
import ntt_model as N
from ntt_model import R

TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
TAUS = {"random": lambda log_n: TAU, "in_domain": lambda log_n: pow(N.omega(log_n), 3, R), "cube_root": lambda log_n: M.CUBE_ROOT}


def poly(log_n, seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(1 << log_n)]


@pytest.mark.parametrize("kind", sorted(TAUS))
@pytest.mark.parametrize("log_n", range(7))
def test_convolution_route_is_synthetic_division(log_n, kind):
    tau, f, n = TAUS[kind](log_n), poly(log_n, 0x0A11 + log_n), 1 << log_n
    table = M.table_logs(tau, log_n)
    assert table == N.ntt_direct(M.x_logs(tau, log_n), log_n + 1)
    if kind == "cube_root" and log_n in (2, 4):
        assert table[0] == 0                                         # 1 + tau + .. + tau^(n-2) with 3 | n - 1
    got, h, made = M.convolution(f, table, log_n)
    assert got == M.proof_logs(f, tau, log_n)
    assert h == M.h_logs(f, tau, log_n) and h[n - 1] == 0
    assert made == M.multiplications(log_n)
    if log_n >= 1:
        assert N.ntt_direct(h, log_n) == got                         # pi = the forward transform of h


@pytest.mark.parametrize("log_n", range(1, 6))
def test_planted_polynomials(log_n):
    n, tau = 1 << log_n, TAU
    table = M.table_logs(tau, log_n)
    w2 = pow(N.omega(log_n + 1), 3, R)
    cases = {"zero": [0] * n, "constant": [7] + [0] * (n - 1), "top": [0] * (n - 1) + [1], "no_top": poly(log_n, 5)[:n - 1] + [0],
             "wide": [R + 3, (1 << 256) - 1] + [R] * (n - 2), "root": ([-w2 % R, 1] + [0] * (n - 2))}
    for name, f in cases.items():
        got, h, _ = M.convolution(f, table, log_n)
        assert got == M.proof_logs(f, tau, log_n), name
        if name in ("zero", "constant"):
            assert got == [0] * n
    if log_n >= 2:                                                   # X - w_2n^3 vanishes at the point F_3 is the value at
        f = cases["root"]
        assert N.ntt_radix2(f + [0] * n, log_n + 1)[3] == 0


def test_multiplication_count_matches_the_plan_header():
    src = open(M.PLAN).read()
    assert "return wide(log_n) + g1_ntt_plan::multiplications(wide_log(log_n)) + g1_ntt_plan::multiplications(log_n);" in src
    import g1_ntt_model as G
    for log_n in range(28):
        assert M.multiplications(log_n) == (2 << log_n) + G.multiplications(log_n + 1) + G.multiplications(log_n)
    assert [M.multiplications(k) for k in range(4)] == [2, 5, 14, 38]
