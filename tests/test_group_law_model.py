"""The lazy group law (proj_add_lazy / proj_double_lazy) replayed on the limb-exact host model (tests/group_law_model.py over
tools/f29_model.py), for every policy the device instantiates: OpsF29, OpsW2, OpsW2I.  No device is involved: the reference is the
reference's own formulas in plain integers mod p (oracle/pyref.py: proj_add / proj_double, RCB'15 algorithms 7 and 9).

What is asserted is what the comments of bn254_pairing.hpp and plk_group.hip state: coordinates N-class, a difference of two coordinates a
legal product operand as it stands, inputs |V| <= 7 (doubling) and <= 2.1 / 2.3 (addition) give outputs |V| <= 2.1 (G1) / 2.3 (G2), and no
i32 / i64 value of the schedule wraps (the model raises Overflow where the device would)."""
import random

import pytest

import group_law_model as G
from group_law_model import M, P
from helpers import SEED
from oracle import pyref as R

M29 = M.M29
S29 = 1 << 29
# the isomorphic twist E'': y^2 = x^3 + (9 - u), 3 b'' = 27 - 3 u (plk_group.hip)
F2I = R._Field(R.fp2_add, R.fp2_sub, R.fp2_neg, R.fp2_mul, R.fp2_inv, R.FP2_ZERO, R.FP2_ONE, (9, P - 1))
POLICIES = {"OpsF29": (G.OpsF29, R.F1), "OpsW2": (G.OpsW2, R.F2), "OpsW2I": (G.OpsW2I, F2I)}
LOWS = [[M29] * 8, [0] * 8, [M29 if i % 2 else 0 for i in range(8)], [0 if i % 2 else M29 for i in range(8)], [1 << 28] * 8]


def top_limb(lo, v, sign):
    """the largest top limb t of sign `sign` with |value(lo + [t])| <= v p"""
    base = M.value(lo + [0])
    t = (int(v * P) - base) >> 232 if sign > 0 else -((int(v * P) + base) >> 232)
    assert M.V(lo + [t]) <= v < M.V(lo + [t + sign])
    return t


def adversarial_vectors(v):
    """N-class digit vectors with |V| <= v: every low-limb pattern under the top limbs 0 and the two bounds +-T(v)"""
    return [lo + [t] for lo in LOWS for t in (0, top_limb(lo, v, 1), top_limb(lo, v, -1))]


def random_vector(rng, v):
    lo = [rng.randrange(S29) for _ in range(8)]
    return lo + [rng.randint(top_limb(lo, v, -1), top_limb(lo, v, 1))]


def draw_point(O, rng, v, adversarial):
    n_parts = len(O.parts(O.zero()))
    pick = (lambda: rng.choice(adversarial_vectors_cached(v))) if adversarial else (lambda: random_vector(rng, v))
    return tuple(O.coord([pick() for _ in range(n_parts)]) for _ in range(3))


_VECTORS = {}


def adversarial_vectors_cached(v):
    if v not in _VECTORS:
        _VECTORS[v] = adversarial_vectors(v)
    return _VECTORS[v]


def check_output(O, r):
    assert G.n_class(O, r), "an output low limb outside [0, 2^29)"
    assert G.max_v(O, r) <= O.bound, (G.max_v(O, r), O.bound)


def check_double(O, F, p):
    r = G.proj_double_lazy(O, p)
    assert G.from_model(O, r) == R.proj_double(F, G.from_model(O, p))
    check_output(O, r)
    return r


def check_add(O, F, p, q):
    r = G.proj_add_lazy(O, p, q)
    assert G.from_model(O, r) == R.proj_add(F, G.from_model(O, p), G.from_model(O, q))
    check_output(O, r)
    return r


@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("adversarial", [True, False], ids=["adversarial", "random"])
def test_formulas_and_bounds_as_stated(policy, adversarial):
    """value == the reference's formulas in plain integers, no Overflow, outputs N-class with |V| inside the stated bound: doublings with
    inputs up to |V| = 7, additions with inputs up to the policy's own output bound (2.1 / 2.3), and at the small |V| of loaded points"""
    cls, F = POLICIES[policy]
    O = cls()
    rng = random.Random(SEED + 900 + adversarial)
    worst = 0.0
    for v in (0.5, O.bound, 7):
        for _ in range(60):
            p, q = draw_point(O, rng, v, adversarial), draw_point(O, rng, min(v, O.bound), adversarial)
            worst = max(worst, G.max_v(O, check_double(O, F, p)))
            if v <= O.bound:
                worst = max(worst, G.max_v(O, check_add(O, F, p, q)))
    assert worst > 1.0                                            # the rows do reach the "+ 1" of a product's value bound


@pytest.mark.parametrize("policy", sorted(POLICIES))
def test_identity_and_mixed_rows(policy):
    """the rows the complete formulas exist for, on adversarial digits: P + 0, 0 + P, 0 + 0, P + P, P + (-P), doubling of Z == 0"""
    cls, F = POLICIES[policy]
    O = cls()
    rng = random.Random(SEED + 902)
    zero = G.proj_zero(O)
    for _ in range(10):
        p = draw_point(O, rng, O.bound, True)
        for a, b in ((p, zero), (zero, p), (zero, zero), (p, p), (p, G.proj_neg(O, p))):
            check_add(O, F, a, b)
        z0 = (p[0], p[1], O.zero())
        assert G.from_model(O, check_double(O, F, z0)) == R.proj_zero(F)


@pytest.mark.parametrize("policy", sorted(POLICIES))
def test_closure_chain(policy):
    """64 alternating doublings and additions fed from their own outputs, from adversarial digits: the outputs stay N-class inside the bound,
    so the class invariant the comments state is closed under the two formulas"""
    cls, F = POLICIES[policy]
    O = cls()
    rng = random.Random(SEED + 901)
    for start in range(3):
        acc, other = draw_point(O, rng, O.bound, True), draw_point(O, rng, O.bound, True)
        for step in range(64):
            if step % 2 == 0:
                acc = check_double(O, F, acc)
            else:
                acc, other = check_add(O, F, acc, other), acc


def run_mutant(policy, mutation, rows=60):
    """(rows that raised Overflow, rows with a wrong value) of the mutated schedule on adversarial rows at the policy's bound"""
    cls, F = POLICIES[policy]
    O = cls(mutation)
    rng = random.Random(SEED + 903)
    overflow = wrong = 0
    for _ in range(rows):
        p, q = draw_point(O, rng, O.bound, True), draw_point(O, rng, O.bound, True)
        try:
            if mutation == "norm_x8_negative_limb":
                ok = G.from_model(O, G.proj_double_lazy(O, p)) == R.proj_double(F, G.from_model(O, p))
            else:
                ok = G.from_model(O, G.proj_add_lazy(O, p, q)) == R.proj_add(F, G.from_model(O, p), G.from_model(O, q))
            wrong += not ok
        except M.Overflow:
            overflow += 1
    return overflow, wrong


@pytest.mark.parametrize("policy", sorted(POLICIES))
def test_mutation_norm_x8_on_a_negative_limb_is_caught(policy):
    """norm_x8 on a D-class vector of the same value (norm(2 t0) - t0 limb by limb): the unsigned carry chain of f29_norm_x8 wraps, the
    model raises Overflow -- on most adversarial rows, for every policy"""
    overflow, wrong = run_mutant(policy, "norm_x8_negative_limb")
    assert overflow + wrong > 0, (overflow, wrong)


@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("mutation", ["skip_norm_3t0", "skip_w2_norm_b3"])
def test_mutations_that_are_harmless_at_these_inputs(policy, mutation):
    """Omitting the norm of t0 = 3 t0, and omitting w2_norm in OpsW2::mul_b3_lazy, are HARMLESS on the adversarial rows: neither Overflow
    nor a wrong value.  The rows plant extreme digits in the INPUT coordinates; the operands these two norms protect are sums of product
    outputs, whose digits the inputs do not control, and lazy arithmetic is exact as long as nothing wraps.  This test records that (it
    asserts the harmlessness, so the statement cannot go stale) and test_what_the_two_norms_protect states the worst case directly:

      * 3 t0 un-normalised has limbs < 3 * 2^29.  f29_mul against an N-class operand: 9 * 3 * 2^58 + sum(p limbs) * 2^29 (= 3.0 * 2^58)
        < 2^63, so on OpsF29 the norm can never be needed for the column bound.  On lane pairs f29_dot2_ilp adds TWO such products per
        column, 54 * 2^58 > 2^63: the norm is needed there, at digits only a crafted product OUTPUT could have.
      * OpsW2::mul_b3_lazy multiplies by the two fixed constants of 3 b'; their low limbs sum to 3.6 and 3.5 (in units of 2^29), so with
        operand limbs up to 2^30 a column stays under (7.1 * 2 + 3.0) * 2^58 < 2^63: for THESE constants the carry pass is not needed
        for the column bound at any digits; it keeps the leaf's stated operand class (N or D)."""
    overflow, wrong = run_mutant(policy, mutation)
    assert (overflow, wrong) == (0, 0)


def test_what_the_two_norms_protect():
    """the worst-case operands of the classes the two harmless mutations produce, straight into the leaves"""
    ones = [M29] * 8 + [0]
    three = [3 * M29] * 8 + [0]
    neg_ones = [-M29] * 8 + [0]
    M.mul(three, ones)                                            # OpsF29: 3 t0 un-normalised fits the column accumulator
    with pytest.raises(M.Overflow):
        M.dot2_ilp(three, ones, three, ones)                      # lane pairs: two such products per column do not
    with pytest.raises(M.Overflow):
        M.dot2_ilp(three, neg_ones, three, neg_ones)
    wide = [2 * M29 + 1] * 8 + [0]                                # limbs 2^30 - 1: the operand of mul_b3_lazy without its carry pass
    for a0, a1 in ((wide, wide), (wide, neg_ones), (neg_ones, wide)):
        G.OpsW2._mul_ilp((a0, a1), (G.B3_K0, G.B3_K1))            # fits, whatever the digits: the constants' limbs are small enough
    assert sum(M.P29[:8]) < 3.01 * S29
    assert sum(abs(x) for x in G.B3_K0[:8]) + sum(abs(x) for x in G.B3_K1[:8]) < 7.1 * S29


# ---- the planted rows of the GPU tests are what they claim ----------------------------------------------------------------------------
def operand_extremes(O, rows):
    """per first-layer operand, (largest, smallest) low limb over the rows"""
    hi, lo = [-S29] * 6, [S29] * 6
    for a, b, ai, bi in rows:
        for k, d in enumerate(G.first_layer_operands(O, G.load_affine(O, a, ai), G.load_affine(O, b, bi))):
            for v in O.parts(d):
                hi[k], lo[k] = max(hi[k], max(v[:8])), min(lo[k], min(v[:8]))
    return hi, lo


def test_on_curve_rows_reach_the_operand_bounds():
    """Over the on-curve rows of tests/test_gpu_group_law_bounds.py, with Z the stored Montgomery one as the kernels load it:
      * x1 - y1 and x2 - y2 reach a limb of magnitude >= 0.99 * 2^29 with both signs (measured 0.9965 / -0.9991 on G1, 0.9992 / -0.9931
        on the twist);
      * y - z and x - z are differences against the FIXED digits of 2^261 mod p.  Its smallest low limb is 0.0405 and its largest 0.9143
        (units of 2^29), so the reachable range is exactly [-0.9143, 0.9595] on a lane that holds the one, and [0, 1) on the odd lane of a
        pair (z = 0 there).  Asserted: the crafted points reach both ends of that range, the negative end to within 1024 / 2^29 (it is met
        exactly where the crafted coordinate's limb is 0; a twist point's y is a square root, its limb there is 315)."""
    one_hi, one_lo = max(G.ONE[:8]), min(G.ONE[:8])
    for O, pts, cols in ((G.OpsF29(), G.g1_points(), None), (G.OpsW2(), G.g2_points(), G.G2_SLICE)):
        rows = G.add_rows(pts, cols)
        assert any(ai for _, _, ai, _ in rows) and any(bi for _, _, _, bi in rows)
        hi, lo = operand_extremes(O, rows)
        for k in (0, 1):
            assert hi[k] >= 0.99 * S29 and lo[k] <= -0.99 * S29, (O.name, k, hi[k] / S29, lo[k] / S29)
        for k in (2, 3, 4, 5):
            assert -one_hi <= lo[k] <= -one_hi + 1024, (O.name, k, lo[k] / S29)
            assert hi[k] >= M29 - one_lo, (O.name, k, hi[k] / S29)
    assert len(G.g1_points()) == 38 and len(G.g2_points()) == 27
    assert all(R.g1_is_on_curve_affine(x, y) for x, y in G.g1_points())
    assert all(R.g2_is_on_curve_affine(x, y) for x, y in G.g2_points())


def test_off_curve_rows_reach_the_worst_column():
    """every off-curve row has ALL eight low limbs of x1 - y1 and of x2 - y2 (both lanes on the twist) at magnitude >= 2^29 - 2: the worst
    column sum a product leaf can meet from two coordinates.  324 ordered value pairs qualify; none of the rows is on its curve."""
    assert len(G.qualifying_pairs()) == 324
    for O, group, on_curve in ((G.OpsF29(), "g1", R.g1_is_on_curve_affine), (G.OpsW2(), "g2", R.g2_is_on_curve_affine)):
        rows = G.offcurve_rows(group)
        assert len(rows) >= 32 and len(set(rows)) == len(rows)
        signs = set()
        for a, b, _, _ in rows:
            assert not on_curve(*a) and not on_curve(*b)
            d = G.first_layer_operands(O, G.load_affine(O, a), G.load_affine(O, b))
            assert all(abs(x) >= S29 - 2 for k in (0, 1) for v in O.parts(d[k]) for x in v[:8])
            signs.add(tuple(v[0] > 0 for k in (0, 1) for v in O.parts(d[k])))
        assert len(signs) == 4 ** len(O.parts(O.zero()))          # every combination of operand signs, so both signs of the column sum


@pytest.mark.parametrize("policy", ["OpsF29", "OpsW2"])
def test_planted_rows_through_the_model(policy):
    """the planted rows through the model's addition and doubling: no Overflow, the reference's value, outputs inside the bound.  (A
    stride over the on-curve rows keeps every point on both sides and the run to seconds.)"""
    cls, F = POLICIES[policy]
    O = cls()
    g1 = policy == "OpsF29"
    rows = G.add_rows(G.g1_points())[::13] if g1 else G.add_rows(G.g2_points(), G.G2_SLICE)[::5]
    n_on = len(rows)
    rows += G.offcurve_rows("g1" if g1 else "g2")[::2]
    for i, (a, b, ai, bi) in enumerate(rows):
        p, q = G.load_affine(O, a, ai), G.load_affine(O, b, bi)
        check_add(O, F, p, q)
        check_add(O, F, p, G.proj_neg(O, q))
        d = check_double(O, F, p)
        if i < n_on:                                              # on the curve P + P and 2 P are one projective point
            assert R.proj_eq(F, G.from_model(O, check_add(O, F, p, p)), G.from_model(O, d))
