"""The crafted inputs of the layout tests (helpers.py): every point is on its curve, and the values really carry the extreme internal digits
they are meant to -- computed with the exact host model of the carry-free core (tools/f29_model.py: from_fp, then the reduce pass that
w2_from_s2 applies)."""
import os
import sys

import numpy as np

from helpers import M29, P, RP_INV, TOP_BOUND, crafted_fp12_rows, crafted_g1_points, crafted_g2_points, crafted_g2_projective, \
    crafted_values, fp_cbrt
from group_law_model import internal_digits
from oracle import coracle
from oracle import pyref as R
from test_gpu_multi_pairing import G1, G2

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import f29_model as M  # noqa: E402


def test_crafted_values_have_extreme_digits():
    vals = crafted_values()
    assert all(0 <= v < P for v in vals) and {0, 1, P - 1} <= set(vals)
    digits = [internal_digits(v) for v in vals]
    for v, d in zip(vals, digits):
        assert M.value(d) % P == v * pow(2, 261, P) % P          # the model's digits are the value the core holds
        assert all(0 <= x <= M29 for x in d[:8])
    lows = [d[:8] for d in digits]
    assert [M29] * 8 in lows and [0] * 8 in lows                 # every low limb at 2^29 - 1; all zero
    assert [M29 if i % 2 else 0 for i in range(8)] in lows
    tops = {d[8] for d in digits}
    assert {1_585_000, 1_400_000, -1_400_000, -TOP_BOUND} <= tops       # the top-limb targets are reached as given
    assert min(tops) < -TOP_BOUND                                 # and past the bound through the reduce pass's rounding
    assert max(abs(M.value(d)) for d in digits) > 0.4999 * P
    # the first 35 values are the set the lane-pair tower test has always used, in the same order
    assert all(M.value(internal_digits(v)) == (v * pow(2, 261, P) % P + P // 2) % P - P // 2 for v in vals[:35])


def test_fp_cbrt():
    for a in [0, 1, 8, 27, P - 1, 2, 3, 5, 7] + crafted_values()[:20]:
        x = fp_cbrt(a)
        if x is None:
            assert pow(a, (P - 1) // 3, P) != 1
        else:
            assert pow(x, 3, P) == a % P
    assert sum(fp_cbrt(v) is not None for v in crafted_values()) > 5


def test_crafted_points_on_curve():
    g1 = crafted_g1_points()
    assert len(g1) >= 16
    vals = set(crafted_values())
    assert sum(x in vals for x, _ in g1) >= 8 and sum(y in vals for _, y in g1) >= 8
    for x, y in g1:
        assert R.g1_is_on_curve_affine(x, y)
    g2 = crafted_g2_points()
    assert len(g2) >= 16
    for x, y in g2:
        assert R.g2_is_on_curve_affine(x, y)
        assert x[0] in vals and x[1] in vals
    for (x, y, z), (ax, ay) in zip(crafted_g2_projective(), g2):
        assert z != (0, 0) and z[0] in vals and z[1] in vals
        assert R.fp2_mul(ax, z) == x and R.fp2_mul(ay, z) == y


def test_crafted_fp12_shapes():
    rows = crafted_fp12_rows()
    assert rows[0] == [0] * 12 and rows[1] == [1] + [0] * 11
    nz = [tuple(i for i, v in enumerate(r) if v) for r in rows]
    for slot in range(12):
        assert (slot,) in nz                                     # a single non-zero coefficient in each slot
    assert (0, 1) in nz and tuple(range(6)) in nz and tuple(range(6, 12)) in nz
    assert sum(len(set(r)) == 1 and r[0] not in (0, 1) for r in rows) >= 4
    assert all(0 <= v < P for r in rows for v in r)
    assert RP_INV * pow(2, 261, P) % P == 1


def test_oracle_miller_steps_match_precompute():
    """the oracle's step wrappers are the steps of its G2 precompute: the first two line coefficients of the generator's table"""
    q = coracle.pack(G2, 16)
    p = coracle.pack(G1, 8)
    table = coracle.g2_precompute(q).reshape(87, 24)
    r = np.concatenate([q, coracle.pack([1, 0], 8)], axis=1)
    d = coracle.g2_doubling_step(r, p)
    px, py = G1
    e = [coracle.from_limbs(table[0, 8 * k:8 * k + 8]) for k in range(3)]
    got = coracle.from_limbs(d[0, 24:])
    assert got[0:2] == e[0] and got[2:4] == [v * py % P for v in e[1]] and got[4:6] == [v * px % P for v in e[2]]
    a = coracle.g2_addition_step(d[:, :24], q, p)                # ATE_NAF[0] = 1: the second coefficient is R + Q
    e = [coracle.from_limbs(table[1, 8 * k:8 * k + 8]) for k in range(3)]
    got = coracle.from_limbs(a[0, 24:])
    assert got[0:2] == e[0] and got[2:4] == [v * py % P for v in e[1]] and got[4:6] == [v * px % P for v in e[2]]
    dbl, _ = coracle.g2_to_affine(coracle.g2_double(r))
    assert np.array_equal(coracle.g2_to_affine(d[:, :24])[0], dbl)
