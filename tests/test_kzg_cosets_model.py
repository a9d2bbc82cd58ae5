"""CPU: the model of the proofs on every coset of the domain (tests/kzg_cosets_model.py).  The convolution route of kzg_cosets.hip, run array by
array and stage by stage on discrete logarithms, gives the quotients of long division by X^l - v^i evaluated at tau -- for a random tau, a
tau inside the domain and a cube root of unity -- for every plane count, with as many products as the plan's formula says, and h_(c-1) = 0.
At log_l = 0 it is tests/kzg_open_all_model.py.  The twist formula of the interpolant is Lagrange's, and the reduced row satisfies the
single-point identity in exponents."""
import random

import pytest

import kzg_cosets_model as M
import kzg_open_all_model as OA
import ntt_model as N
from ntt_model import R

TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
TAUS = {"random": lambda log_n: TAU, "in_domain": lambda log_n: pow(N.omega(log_n), 3, R), "cube_root": lambda log_n: M.CUBE_ROOT}
SHAPES = [(log_c, log_l) for log_c in range(7) for log_l in range(7 - log_c)]


def poly(log_n, seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(1 << log_n)]


@pytest.mark.parametrize("kind", sorted(TAUS))
@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_convolution_route_is_long_division(log_c, log_l, kind):
    log_n, c = log_c + log_l, 1 << log_c
    tau, f = TAUS[kind](log_n), poly(log_n, 0x0C05 + 16 * log_c + log_l)
    table = M.table_logs(tau, log_c, log_l)
    assert table[0] == N.ntt_direct(M.x_logs(tau, 0, log_c, log_l), log_c + 1)
    want = M.proof_logs(f, tau, log_c, log_l)
    for planes_log in range(log_l + 1):
        got, h, made = M.convolution(f, table, log_c, log_l, planes_log)
        assert got == want, planes_log
        assert h == M.h_logs(f, tau, log_c, log_l)[:c - 1] + [0] and h[c - 1] == 0
        assert made == M.multiplications(log_c, log_l)
    if log_c >= 1:
        assert N.ntt_direct(h, log_c) == want                        # pi = the forward transform of h over v = w^l
        assert N.omega(log_c) == M.roots(log_c, log_l)[1]


@pytest.mark.parametrize("log_n", range(6))
def test_single_point_cosets_are_the_open_all_model(log_n):
    f = poly(log_n, 0x0C06 + log_n)
    assert M.x_logs(TAU, 0, log_n, 0) == OA.x_logs(TAU, log_n) and M.table_logs(TAU, log_n, 0) == [OA.table_logs(TAU, log_n)]
    assert M.proof_logs(f, TAU, log_n, 0) == OA.proof_logs(f, TAU, log_n)
    assert M.convolution(f, M.table_logs(TAU, log_n, 0), log_n, 0) == OA.convolution(f, OA.table_logs(TAU, log_n), log_n)
    assert M.multiplications(log_n, 0) == OA.multiplications(log_n)


def test_one_coset_has_the_identity_as_its_proof():
    for log_l in range(5):
        f = poly(log_l, 0x0C07)
        assert M.proof_logs(f, TAU, 0, log_l) == [0] and M.convolution(f, M.table_logs(TAU, 0, log_l), 0, log_l)[0] == [0]


@pytest.mark.parametrize("log_c,log_l", [(1, 2), (2, 1), (3, 2), (2, 3)])
def test_planted_polynomials(log_c, log_l):
    n, l, c = 1 << (log_c + log_l), 1 << log_l, 1 << log_c
    table = M.table_logs(TAU, log_c, log_l)
    v3 = pow(M.roots(log_c, log_l)[1], 3 % c, R)
    vanish = [0] * n
    vanish[0], vanish[l] = -v3 % R, (vanish[l] + 1) % R
    cases = {"zero": [0] * n, "low": poly(log_l, 3) + [0] * (n - l), "top": [0] * (n - 1) + [1], "no_top": poly(log_c + log_l, 5)[:n - 1] + [0],
             "wide": [R + 3, (1 << 256) - 1] + [R] * (n - 2), "vanish": vanish}
    for name, f in cases.items():
        got, h, _ = M.convolution(f, table, log_c, log_l)
        assert got == M.proof_logs(f, TAU, log_c, log_l), name
        if name in ("zero", "low"):
            assert got == [0] * c                                    # degree below l: every quotient is zero
    q, rem = M.divide(vanish, 3 % c, log_c, log_l)
    assert q == [1] + [0] * (n - 1) and rem == [0] * l               # X^l - v^3: the quotient on coset 3 is the constant 1 and R is zero


def test_multiplication_count_matches_the_plan_header():
    src = open(M.PLAN).read()
    assert "return mul_sat(wide(log_c), elems(log_l)) + g1_ntt_plan::multiplications(wide_log(log_c)) + g1_ntt_plan::multiplications(log_c);" in src
    import g1_ntt_model as G
    for log_c in range(28):
        for log_l in range(28 - log_c):
            assert M.multiplications(log_c, log_l) == (2 << (log_c + log_l)) + G.multiplications(log_c + 1) + G.multiplications(log_c)
    assert M.multiplications(10, 4) == (1 << 15) + OA.multiplications(10) - (2 << 10)


@pytest.mark.parametrize("log_c,log_l", [(0, 0), (0, 3), (1, 0), (1, 2), (2, 1), (3, 2), (2, 4)])
def test_the_twist_is_lagrange_interpolation_and_the_reduced_row_holds(log_c, log_l):
    log_n, c = log_c + log_l, 1 << log_c
    f = poly(log_n, 0x0C08 + log_n)
    ys = M.cells(M.values(f, log_c, log_l), log_c, log_l)
    proofs, c_log = M.proof_logs(f, TAU, log_c, log_l), M.evaluate(f, TAU)
    for i in range(c):
        r = M.interp_twist(ys[i], i, log_c, log_l)
        assert r == M.interp_lagrange(ys[i], i, log_c, log_l) == M.divide(f, i, log_c, log_l)[1]
        assert M.interp_twist(ys[i], i + 3 * c, log_c, log_l) == r   # idx >= c: the words of idx mod c
        cred, z = M.reduced_row(c_log, i, ys[i], TAU, log_c, log_l)
        assert M.single_point_holds(cred, z, proofs[i], TAU, log_l)
        assert not M.single_point_holds(cred, z, (proofs[i] + 1) % R, TAU, log_l)
        if c > 1:
            assert not M.single_point_holds(*M.reduced_row(c_log, (i + 1) % c, ys[i], TAU, log_c, log_l), proofs[i], TAU, log_l)
    rnd = poly(log_l, 0x0C09)
    assert M.interp_twist(rnd, c - 1, log_c, log_l) == M.interp_lagrange(rnd, c - 1, log_c, log_l)
