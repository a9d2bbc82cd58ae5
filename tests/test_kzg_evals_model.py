"""CPU: the integer model of KZG from evaluation form (tests/kzg_evals_model.py) against the DEFINITIONS it abbreviates, at n <= 64:
interpolate with tests/ntt_model.py, divide by (X - z) with tests/kzg_prove_model.py, evaluate again; sum_i L_i(tau) f_i = f(tau); batch
inversion against pow, zeros included.  And the new entry points are declared with their shapes and bindings."""
import random

import pytest

import kzg_evals_model as E
import kzg_prove_model as KP
import ntt_model as N
from kzg_evals_model import EDGE_WORDS, R

NEW_SYMBOLS = ("sylow_hip_fr_batch_inv", "sylow_hip_kzg_quotient_evals_batch", "sylow_hip_kzg_open_evals_batch")


def by_definition(evals, log_n, z):
    """(q values, y) through the coefficients: intt, the recurrence of the coefficient-form quotient, ntt"""
    coeffs = N.ntt_direct(evals, log_n, inverse=True) if log_n <= 4 else N.ntt_radix2(evals, log_n, inverse=True)
    q, y = KP.quotient(coeffs, z)
    return N.ntt_radix2(q, log_n), y


def test_constants_agree_with_the_transform():
    assert E.W == N.W and E.R == N.R == KP.R and E.P == KP.P
    assert all(E.omega(k) == N.omega(k) for k in range(29))
    assert all((R - ((R - 1) >> k)) * (1 << k) % R == 1 for k in range(29))
    K = E.plan_constants()
    assert K == {"EVALS_BLOCK": 256, "EVALS_LANE_ELEMS": 8, "EVALS_CHUNK": 2048, "EVALS_LOG_N_MAX": 28}


def test_batch_inv_is_pow_with_the_zero_rule():
    rng = random.Random(0xE0)
    for n in (1, 2, 7, 8, 9, 64, 100):
        a = [rng.randrange(1 << 256) for _ in range(n)]
        for i, w in enumerate(EDGE_WORDS):
            if i < n:
                a[(i * 5) % n] = w
        got = E.batch_inv(a)
        assert got == [pow(v % R, R - 2, R) for v in a]
        assert all((v * g) % R == (1 if v % R else 0) for v, g in zip(a, got))
    assert E.batch_inv([0, 0, 0]) == [0, 0, 0] and E.batch_inv([0, 5, R]) == [0, pow(5, -1, R), 0] and E.batch_inv([]) == []


@pytest.mark.parametrize("log_n", range(7))
def test_quotient_outside_the_domain_is_the_division_of_the_interpolant(log_n):
    rng = random.Random(0xE1 + log_n)
    n = 1 << log_n
    for z in [rng.randrange(R), 0, R, E.TOP, 2, rng.randrange(1 << 256)]:
        if E.hit_index(log_n, z) is not None:
            continue
        evals = [rng.randrange(1 << 256) for _ in range(n)]
        q, y = E.quotient(evals, log_n, z)
        wq, wy = by_definition(evals, log_n, z)
        assert y == wy and q == wq, (log_n, z)


@pytest.mark.parametrize("log_n", range(7))
def test_quotient_inside_the_domain_is_the_division_of_the_interpolant(log_n):
    rng = random.Random(0xE2 + log_n)
    n, w = 1 << log_n, E.omega(log_n)
    for k in sorted({0, 1 % n, n // 2, n - 1, rng.randrange(n)}):
        z = pow(w, k, R)
        evals = [rng.randrange(R) for _ in range(n)]
        for zz in (z, z + R):                                   # however the word was written
            q, y = E.quotient(evals, log_n, zz)
            wq, wy = by_definition(evals, log_n, zz)
            assert y == wy == evals[k] and q == wq, (log_n, k)
            assert E.quotient(evals, log_n, zz, k=k) == (q, y)
    if log_n:
        assert E.hit_index(log_n, R - 1) == n // 2


def test_quotient_of_a_constant_is_zero_and_log_n_0():
    for log_n in (0, 3):
        n = 1 << log_n
        for z in (5, 1, R - 1, 0):
            q, y = E.quotient([7] * n, log_n, z)
            assert y == 7 and q == [0] * n
    assert E.quotient([R + 3], 0, 1) == ([0], 3) and E.quotient([9], 0, 12345) == ([0], 9)


@pytest.mark.parametrize("log_n", [0, 1, 3, 6])
def test_lagrange_basis_evaluates_the_interpolant(log_n):
    rng = random.Random(0xE3 + log_n)
    n, tau = 1 << log_n, rng.randrange(2, R)
    lag = E.lagrange_at(log_n, tau)
    assert sum(lag) % R == 1                                    # the basis sums to the constant 1
    for _ in range(3):
        evals = [rng.randrange(R) for _ in range(n)]
        coeffs = N.ntt_radix2(evals, log_n, inverse=True)
        assert sum(l * f for l, f in zip(lag, evals)) % R == KP.evaluate(coeffs, tau)
    # and the opening's identity in the exponent: q(tau) (tau - z) = f(tau) - y, inside and outside the domain
    evals = [rng.randrange(R) for _ in range(n)]
    f_tau = sum(l * f for l, f in zip(lag, evals)) % R
    for z in (rng.randrange(R), pow(E.omega(log_n), n - 1, R)):
        q, y = E.quotient(evals, log_n, z)
        assert sum(l * v for l, v in zip(lag, q)) % R * (tau - z) % R == (f_tau - y) % R


def test_new_entry_points_are_declared_bound_and_shaped():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sylow_amd import _lib, _shapes
    table = _shapes.table()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in table, name
    names, shapes = table["sylow_hip_kzg_quotient_evals_batch"]
    assert names[:6] == ["evals", "log_n", "m", "z", "q_out", "y_out"]
    live = {0x1000: 4 * 8 * 3 * 8, 0x2000: 4 * 3 * 8, 0x3000: 4 * 8 * 3 * 8, 0x4000: 4 * 3 * 8}
    _shapes.check_call("sylow_hip_kzg_quotient_evals_batch", (0x1000, 3, 3, 0x2000, 0x3000, 0x4000), live)
    _shapes.check_call("sylow_hip_kzg_quotient_evals_batch", (0x1000, 3, 3, 0x2000, None, 0x4000), live)
    with pytest.raises(ValueError):
        _shapes.check_call("sylow_hip_kzg_quotient_evals_batch", (0x1000, 4, 3, 0x2000, 0x3000, 0x4000), live)
    with pytest.raises(ValueError):
        _shapes.check_call("sylow_hip_fr_batch_inv", (0x2000, 0x4000, 4), live)
    _shapes.check_call("sylow_hip_fr_batch_inv", (0x2000, 0x4000, 3), live)
