"""The model of the several-point KZG opening (tests/kzg_points_model.py) against plain long division: the identities kzg_points.hip rests on.
CPU only."""
import random

import pytest

import kzg_points_model as M
import kzg_prove_model as KP

R = M.R


def _case(rng, ln, k, distinct=True):
    f = [rng.randrange(R) for _ in range(ln)]
    zs = rng.sample(range(1, 1 << 40), k) if distinct else [rng.randrange(1, 5) for _ in range(k)]
    return f, zs


@pytest.mark.parametrize("k", [1, 2, 3, 5, 7])
def test_weighted_quotients_are_the_long_division(k):
    rng = random.Random(0x51 + k)
    for ln in list(range(1, 20)) + [40]:
        f, zs = _case(rng, ln, k)
        q, y = M.quotient_points(f, zs)
        want_q, want_r = M.long_division(f, M.vanishing(zs))
        assert q == want_q, (ln, k)
        assert y == [KP.evaluate(f, z) for z in zs]
        assert M.remainder_points(zs, y) == want_r
        assert q[max(ln - k, 0):] == [0] * min(k, ln)              # the degree drops by k


@pytest.mark.parametrize("ln,k", [(9, 3), (33, 7), (4, 4), (2, 5)])
def test_identity_at_a_random_tau(ln, k):
    rng = random.Random(0x52 + ln)
    f, zs = _case(rng, ln, k)
    tau = rng.randrange(R)
    q, y = M.quotient_points(f, zs)
    lhs = (KP.evaluate(f, tau) - KP.evaluate(M.remainder_points(zs, y), tau)) % R
    assert lhs == KP.evaluate(q, tau) * KP.evaluate(M.vanishing(zs), tau) % R
    assert M.row_holds(KP.evaluate(f, tau), zs, y, KP.evaluate(q, tau), tau)
    bad = list(y)
    bad[k // 2] = (bad[k // 2] + 1) % R
    assert not M.row_holds(KP.evaluate(f, tau), zs, bad, KP.evaluate(q, tau), tau)


@pytest.mark.parametrize("k", [1, 2, 4, 7])
def test_short_polynomials_have_a_zero_quotient(k):
    rng = random.Random(0x53 + k)
    for ln in range(1, k + 1):
        f, zs = _case(rng, ln, k)
        q, y = M.quotient_points(f, zs)
        assert q == [0] * ln
        assert M.remainder_points(zs, y) == f + [0] * (k - ln)     # R = f


def test_repeated_points_drop_out():
    """a point that collides with another gets the weight 0: the row equals the formula over the points that collide with none"""
    rng = random.Random(0x54)
    f = [rng.randrange(R) for _ in range(12)]
    zs = [5, 9, 5 + R, 11, 9]                                      # 5 twice (written differently), 9 twice, 11 alone
    a, distinct = M.weights(zs)
    assert not distinct and [bool(v) for v in a] == [False, False, False, True, False]
    den = 1
    for z in zs:
        if z % R != 11:
            den = den * (11 - z) % R
    assert a[3] == M.inv0(den)
    q, y = M.quotient_points(f, zs)
    q11, _ = KP.quotient(f, 11)
    assert q == [a[3] * v % R for v in q11] and y == [KP.evaluate(f, z % R) for z in zs]
    assert not M.row_holds(KP.evaluate(f, 77), zs, y, KP.evaluate(q, 77), 77)      # rejected whatever else it holds
    assert M.weights([3, 4, 3 + 2 * R])[1] is False and M.weights([3, 4, 5])[1] is True
    assert M.weights([7]) == ([1], True)                           # k = 1: the empty product


def test_one_point_is_the_single_point_model():
    rng = random.Random(0x55)
    for ln in (1, 2, 17):
        f = [rng.randrange(1 << 256) for _ in range(ln)]
        z = rng.randrange(1 << 256)
        q, y = M.quotient_points(f, [z])
        want_q, want_y = KP.quotient(f, z)
        assert q == want_q and y == [want_y]
        assert M.vanishing([z]) == [-z % R, 1] and M.remainder_points([z], y) == [want_y]


def test_plan_constants_are_read_from_the_source():
    c = M.plan_constants()
    assert c["KZGPT_MAX_POINTS"] == 64 and c["KZGPT_BLOCK"] == c["KZG_POLY_BLOCK"] and c["KZGPT_ROW_BLOCK"] >= c["KZGPT_MAX_POINTS"]
