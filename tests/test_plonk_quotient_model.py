"""CPU: the integer model of PLONK's quotient (tests/plonk_quotient_model.py) against itself: the schoolbook route (products by the definition,
long division by X^n - 1) and the pointwise route of the device (the table on K, the fused step, the transform back) agree; a satisfied
witness, blinded or not, leaves remainder 0, status 0 and the exact long-division quotient; a changed wire, a changed public input and a
scaled z leave status 1 where the flag is exact (D < N); and the bound D - n < N is the one the header states."""
import random

import pytest

import ntt_model as T
import plonk_quotient_model as Q

R = Q.R
SEED = 0x51A7E


def challenges(rng):
    return rng.randrange(R), rng.randrange(R), rng.randrange(R)


def both_routes(c, rows, zi, wc, zc, pc, beta, gamma, alpha, log_e):
    """(t, status, quotient, remainder); the two routes compared at every point of K"""
    log_n, lb = c["log_n"], c["log_n"] + log_e
    t, status = Q.quotient(rows, zi, wc, zc, pc, c["shifts"], beta, gamma, alpha, log_n, log_e)
    quo, rem = Q.divide_by_vanishing(Q.numerator(c["selectors"], c["sigma"], wc, zc, pc, c["shifts"], beta, gamma, alpha, log_n), log_n)
    assert len(quo) <= Q.degree_bound(log_n, c["W"], len(wc[0]), len(zc)) - (1 << log_n) + 1
    x, w = Q.SHIFT, T.omega(lb)
    for i, v in enumerate(Q.on_coset(t, lb)):
        assert v == (Q.p_eval(quo, x) + Q.p_eval(rem, x) * zi[i % (1 << log_e)]) % R, i
        x = x * w % R
    return t, status, quo, rem


@pytest.mark.parametrize("log_e", [2, 3])
@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("log_n", [0, 1, 3])
def test_the_two_routes_agree_and_a_satisfied_witness_divides(log_n, W, log_e):
    rng = random.Random(SEED + 100 * log_n + 10 * W + log_e)
    n, big = 1 << log_n, 1 << (log_n + log_e)
    for with_pi in (False, True):
        c = Q.circuit(rng, log_n, W, with_pi)
        rows, zi = Q.table(c["selectors"], c["sigma"], log_n, log_e)
        assert len(rows) == 2 * W + 3 and all(len(r) == big for r in rows) and len(zi) == 1 << log_e
        for blinded in (False, True):
            len_w, len_z = (n + 2, n + 3) if blinded else (n, n)
            if not Q.args_ok(log_n, log_e, W, len_w, len_z):
                assert blinded, "the unblinded case always fits"
                continue
            beta, gamma, alpha = challenges(rng)
            wc, zc, pc = Q.witness_polys(c, beta, gamma, rng if blinded else None)
            assert (len(wc[0]), len(zc)) == (len_w, len_z)
            t, status, quo, rem = both_routes(c, rows, zi, wc, zc, pc, beta, gamma, alpha, log_e)
            assert not any(rem) and status == 0 and t == quo + [0] * (big - len(quo)), (with_pi, blinded)


@pytest.mark.parametrize("log_n,W,log_e", [(3, 2, 2), (3, 3, 2), (3, 4, 3), (1, 2, 2), (0, 2, 2)])
def test_a_broken_witness_raises_the_flag_where_it_is_exact(log_n, W, log_e):
    rng = random.Random(SEED + 7 * log_n + W)
    n, big = 1 << log_n, 1 << (log_n + log_e)
    assert Q.degree_bound(log_n, W, n, n) < big, "D < N: status 0 is divisibility"
    c = Q.circuit(rng, log_n, W, with_pi=True)
    rows, zi = Q.table(c["selectors"], c["sigma"], log_n, log_e)
    beta, gamma, alpha = challenges(rng)
    wc, zc, pc = Q.witness_polys(c, beta, gamma)
    assert both_routes(c, rows, zi, wc, zc, pc, beta, gamma, alpha, log_e)[1] == 0
    wires = [list(w) for w in c["wires"]]
    wires[W - 1][n - 1] = (wires[W - 1][n - 1] + 1) % R
    changed_wire = Q.witness_polys(c, beta, gamma, wires=wires)[0]
    changed_pi = Q.coefficients([(c["pi"][0] + 1) % R] + c["pi"][1:], log_n)
    for what, args in (("wire", (changed_wire, zc, pc)), ("pi", (wc, zc, changed_pi)), ("z", (wc, Q.p_scale(zc, 3), pc))):
        t, status, quo, rem = both_routes(c, rows, zi, *args, beta, gamma, alpha, log_e)
        assert any(rem) and status == 1, what


def test_the_degree_bound_and_the_refused_lengths():
    # D = max((len_z - 1) + W max(len_w - 1, 1), 2 (len_w - 1) + n - 1, n + len_z - 2), written out by hand
    assert Q.degree_bound(3, 3, 8, 8) == 28 and Q.degree_bound(3, 3, 10, 11) == 37 and Q.degree_bound(0, 2, 1, 1) == 2
    assert Q.degree_bound(3, 2, 1, 20) == 26 and Q.degree_bound(2, 2, 9, 1) == 19 and Q.degree_bound(4, 2, 1, 1) == 15
    # blinded W = 3 over E = 4: D - n = 3 n + 5 < 4 n from n = 8 on
    assert not Q.args_ok(2, 2, 3, 6, 7) and Q.args_ok(3, 2, 3, 10, 11) and Q.args_ok(3, 2, 3, 32, 5) is False
    assert Q.args_ok(3, 2, 2, 8, 26) and not Q.args_ok(3, 2, 2, 8, 27), "D - n = N - 1 fits, N does not"
    assert not Q.args_ok(3, 2, 1, 8, 8) and not Q.args_ok(3, 2, 33, 1, 1) and not Q.args_ok(3, 2, 2, 0, 8) and not Q.args_ok(3, 2, 2, 33, 8)
    # the table's tail: X^n - 1 on K takes E values, indexed by i mod E
    for log_n, log_e in ((0, 2), (3, 2), (2, 3)):
        zi, w = Q.zinv(log_n, log_e), T.omega(log_n + log_e)
        for i in range(1 << (log_n + log_e)):
            assert (pow(Q.SHIFT * pow(w, i, R), 1 << log_n, R) - 1) * zi[i % (1 << log_e)] % R == 1
