"""CPU: the carry-free field core (sylow_amd/csrc/bn254_f29.hpp) at the bounds it states.  tools/f29_model.py transcribes each routine
with the device's i32 / u32 / i64 widths and raises where a device value would wrap; these tests check its constants against the header,
its results against exact integer formulas, and run it on vectors that sit on every stated bound: limbs at +-L 2^29, top limbs at
+-(2^28 - 1), L(a) L(b) = 2.5 both ways, values at +-64 p for to_fp, reduce inputs at |limb| = 2^36 - 1 and on rounding boundaries of
the quotient estimate, and the linear-combination coefficients the kernels actually pass (CALL_SITES, checked against the sources).
tests/test_gpu_f29_bounds.py sends the same vectors through the device and compares every output word with the model."""
import glob
import os
import random
import re
import sys
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import f29_model as M  # noqa: E402

P = M.P
HDR = os.path.join(ROOT, "sylow_amd", "csrc", "bn254_f29.hpp")
CSRC = os.path.join(ROOT, "sylow_amd", "csrc")
TOP = (1 << 28) - 1                  # the largest top limb of a normalized value
B29 = 1 << 29
RINV = pow(M.RP, -1, P)              # 2^-261 mod p
PT = Fraction(P, 1 << 232)           # p / 2^232 = 3171406.4...


def congruent(r, x):
    return (M.value(r) - x) % P == 0


# ---- vector generators --------------------------------------------------------------------------------------------------
def pattern(lim, top, kind, sign=1):
    """9 limbs: the 8 low limbs at +-lim (all +, all -, alternating, or the alternation shifted by one) and the top limb at +-top"""
    s = {"pos": [1] * 8, "neg": [-1] * 8, "alt": [(-1) ** i for i in range(8)], "tla": [-((-1) ** i) for i in range(8)]}[kind]
    return [sign * x * lim for x in s] + [sign * top]


def bound_vectors(lim, top, rng=None, n_random=0, nonneg=False):
    """vectors whose limbs sit on the bound (|low| <= lim, |top| <= top): the patterns at +-top and 0 on top, then random ones"""
    kinds = ["pos"] if nonneg else ["pos", "neg", "alt", "tla"]
    out = []
    for k in kinds:
        for t in (top, -top, 0):
            out.append(pattern(lim, 0, k)[:8] + [t])
    for _ in range(n_random):
        lo = 0 if nonneg else -lim
        out.append([rng.randint(lo, lim) for _ in range(8)] + [rng.randint(-top, top)])
    return out


def normalized_random(rng, n, vmax=None):
    """normalized vectors: low limbs uniform in [0, 2^29), top limb uniform over |top| < 2^28 (or over |value| <= vmax p)"""
    out = []
    for _ in range(n):
        t = TOP if vmax is None else min(TOP, int(vmax * PT))
        out.append([rng.randrange(B29) for _ in range(8)] + [rng.randint(-t, t)])
    return out


def l_pair_limits():
    """(lim_a, lim_b) with L(a) L(b) = 2.5 exactly, split both ways, plus the L = 1 pair of normalized operands"""
    return [(5 * B29 // 2, B29), (B29, 5 * B29 // 2), (5 * B29 // 4, 2 * B29), (2 * B29, 5 * B29 // 4), (B29 - 1, B29 - 1)]


def mul_cases(rng, n_random=0):
    """(a, b) pairs for f29_mul at L(a) L(b) <= 2.5: every pattern pair at the limits, then random pairs at the same limits"""
    cases = []
    for la, lb in l_pair_limits():
        ta, tb = min(la // 2, (1 << 31) - 1), min(lb // 2, (1 << 31) - 1)
        va, vb = bound_vectors(la, ta), bound_vectors(lb, tb)
        cases += [(a, b) for a in va for b in vb]
        for _ in range(n_random):
            cases.append(([rng.randint(-la, la) for _ in range(8)] + [rng.randint(-ta, ta)],
                          [rng.randint(-lb, lb) for _ in range(8)] + [rng.randint(-tb, tb)]))
    return cases


def dot2_cases(rng, n_random=0):
    """four operands with |limbs| < 2^29, signs free (u2_mul passes a negated operand), tops at +-(2^28 - 1)"""
    vs = bound_vectors(B29 - 1, TOP)
    cases = [(a, b, a, b) for a in vs for b in vs] + [(a, b, b, a) for a in vs for b in vs[::3]]
    for _ in range(n_random):
        cases.append(tuple([rng.randint(-B29 + 1, B29 - 1) for _ in range(8)] + [rng.randint(-TOP, TOP)] for _ in range(4)))
    return cases


def sqr_cases(rng, n_random=0):
    """N-class inputs: low limbs in [0, 2^29), top at +-(2^28 - 1)"""
    return bound_vectors(B29 - 1, TOP, nonneg=True) + [[B29 - 1] * 8 + [t] for t in (TOP, -TOP, 1, -1)] + normalized_random(rng, n_random)


def to_fp_values():
    """values at the edges of (-64 p, 64 p) and the representations of 0, +-p, plus multiples of p around the conditional subtractions"""
    vals = [-64 * P + 1, 64 * P - 1, 0, P, -P, P - 1, -P + 1, 1, -1, 2 * P, -2 * P, 4 * P, -4 * P, 32 * P, -32 * P, 63 * P, -63 * P]
    vals += [k * P + d for k in range(-64, 64) for d in (-1, 0, 1) if -64 * P < k * P + d < 64 * P]
    return sorted(set(vals))


def to_fp_cases(rng, n_random=0):
    cases = [M.digits(v) for v in to_fp_values()]
    for _ in range(n_random):
        cases.append(M.digits(rng.randrange(-64 * P + 1, 64 * P)))
    return cases


def rounding_t8(count=6, span=1 << 31):
    """top-limb sums t8 (|t8| < 2^31) whose quotient estimate (t8 K + 2^43) / 2^44 lies within |t8| / 2^44 of a rounding boundary:
    q changes there when K is off by one, either way"""
    up, down, t = [], [], span - 1
    while (len(up) < count or len(down) < count) and t > 0:
        f = (t * M.K + (1 << 43)) % (1 << 44)
        if f < t and len(down) < count:
            down.append(t)
        elif f >= (1 << 44) - t and len(up) < count:
            up.append(t)
        t -= 1
    return up + down + [-x for x in up + down]


def reduce_cases(rng, n_random=0):
    """(a, b, k0, k1) with limb(i) = k0 a[i] + k1 b[i] (hook op 8): every low limb at +-(2^36 - 1) in every pattern, the top at
    +-(2^31 - 1) and on the rounding boundaries of the quotient estimate"""
    lim, cases = (1 << 31) - 1, []
    tops = [(1 << 31) - 1, -(1 << 31) + 1, 0, 1, -1] + rounding_t8()
    for kind in ("pos", "neg", "alt", "tla"):
        s = pattern(1, 0, kind)[:8]
        for t8 in tops:
            a = [x * lim for x in s] + [t8 >> 5]
            b = [x * 31 for x in s] + [t8 & 31]
            cases.append((a, b, 32, 1))
    for t8 in rounding_t8():                                 # the boundary t8 with zero low limbs: q decides alone
        cases.append(([0] * 8 + [t8 >> 5], [0] * 8 + [t8 & 31], 32, 1))
    for _ in range(n_random):
        a = [rng.randint(-lim, lim) for _ in range(8)] + [rng.randint(-(1 << 26) + 1, (1 << 26) - 1)]
        b = [rng.randint(-31, 31) for _ in range(9)]
        cases.append((a, b, 32, 1))
    return cases


def reduce_limbs(a, b, k0, k1):
    return [x * k0 + y * k1 for x, y in zip(a, b)]


# ---- constants ---------------------------------------------------------------------------------------------------------------------
def test_model_constants_match_the_header():
    src = open(HDR).read()
    body = re.search(r"void f29_p\(i32 \(&p\)\[9\]\) \{(.*?)\}", src, re.S).group(1)
    assert [int(x, 16) for x in re.findall(r"p\[\d\] = (0x[0-9a-f]+);", body)] == M.P29
    assert sum(x << (29 * i) for i, x in enumerate(M.P29)) == P and all(0 <= x < B29 for x in M.P29)
    assert int(re.search(r"#define BN_PINV29 (0x[0-9a-f]+)u", src).group(1), 16) == M.PINV29
    assert (P * M.PINV29 + 1) % B29 == 0                                           # -p^-1 mod 2^29
    assert re.findall(r"\* (\d+)ll \+ \(1ll << 43\)\) >> 44", src) == [str(M.K)] * 2  # both reduce passes use the model's K
    k64 = re.search(r"const i32 k64\[9\] = \{([^}]*)\}", src).group(1)
    assert [int(x, 16) for x in k64.split(",")] == M.K64
    assert sum(x << (29 * i) for i, x in enumerate(M.K64)) == 64 * P and all(0 <= x < B29 for x in M.K64)
    c4 = re.search(r"const u32 c0 = (0x[0-9a-f]+)u, c1 = (0x[0-9a-f]+)u, c2 = (0x[0-9a-f]+)u, c3 = (0x[0-9a-f]+)u, c4 = (0x[0-9a-f]+)u, "
                   r"c5 = (0x[0-9a-f]+)u, c6 = (0x[0-9a-f]+)u, c7 = (0x[0-9a-f]+)u;", src).groups()
    assert [int(x, 16) for x in c4] == M.P4 and M.words_value(M.P4) == 4 * P
    two = re.search(r"cond_sub_const\(r, ((?:0x[0-9a-f]+u, ){7}0x[0-9a-f]+u)\);  // 2p", src).group(1)
    assert [int(x.strip().rstrip("u"), 16) for x in two.split(",")] == M.P2 and M.words_value(M.P2) == 2 * P
    assert M.RP == 1 << 261 and M.P1 == M.int_to_words(P)


def test_quotient_multiplier_and_its_error_bound():
    """K / 2^44 estimates 2^232 / p; the header's bound |value - q p| < 0.51 p follows for |limb(8)| < 2^31 and |limb(i<8)| < 2^36"""
    exact = Fraction(1 << 276, P)                                                   # 2^44 / (p / 2^232) = 5547124.38...
    assert abs(M.K - exact) < 44                                                    # 5547168: 43.6 above, i.e. 7.9e-6 relative
    est_err = (1 << 31) * abs(Fraction(M.K, 1 << 44) - 1 / PT)                      # |q - t8 / (p / 2^232)| beyond rounding
    eps_err = Fraction(1 << 8) / PT                                                 # the low limbs: |eps| < 2^8 units of 2^232
    assert Fraction(1, 2) + est_err + eps_err < Fraction(51, 100)
    assert est_err < Fraction(6, 1000)                                              # as the header states it: < 0.006 p


# ---- correctness and stated output bounds, at the bounds ------------------------------------------------------------------------
def check_product(r, x, vmag, name):
    """r = x / 2^261 mod p in the Montgomery window: low limbs in [0, 2^29), -vmag/2^261 <= value < vmag/2^261 + p"""
    assert congruent(r, x * RINV), name
    assert all(0 <= v < B29 for v in r[:8]), name
    v = M.value(r)
    assert -vmag <= v * M.RP and v * M.RP < vmag + P * M.RP, name
    if Fraction(vmag, P * P) / 169 + 1 < 84:                 # the header's window (V(a) V(b) / 169 + 1) p keeps the top limb normalized
        assert M.normalized(r), name


def test_mul_and_leaf_at_l_product_2_5():
    rng = random.Random(1)
    cases = mul_cases(rng, n_random=60)
    assert len(cases) > 700
    for a, b in cases:
        assert M.L(a) * M.L(b) <= 2.5
        check_product(M.mul(a, b), M.value(a) * M.value(b), abs(M.value(a) * M.value(b)), ("mul", a, b))


def test_mul_rejects_what_overflows_past_the_bound():
    """the model's checks are live: L(a) L(b) = 4 (every limb at +-2^30) wraps a column accumulator"""
    a = [1 << 30] * 8 + [0]
    with pytest.raises(M.Overflow):
        M.mul(a, [2 ** 31 - 1] * 8 + [0])


def test_dot2_forms_at_the_bound():
    rng = random.Random(2)
    for a, b, c, d in dot2_cases(rng, n_random=60):
        x = M.value(a) * M.value(b) + M.value(c) * M.value(d)
        mag = abs(M.value(a) * M.value(b)) + abs(M.value(c) * M.value(d))
        r = M.dot2(a, b, c, d)
        check_product(r, x, mag, ("dot2", a, b, c, d))
        assert M.dot2_ilp(a, b, c, d) == r                   # the same column sums, only split differently: identical digits


def test_sqr_at_the_bound():
    rng = random.Random(3)
    for a in sqr_cases(rng, n_random=100):
        r = M.sqr(a)
        check_product(r, M.value(a) ** 2, M.value(a) ** 2, ("sqr", a))
        assert r == M.mul(a, a)                              # the same columns, the cross products only taken once


def test_norm_family_at_the_bound():
    rng = random.Random(4)
    for a in bound_vectors(3 * B29, 3 * (1 << 28), rng, 200):            # lazy values, L <= 3
        r = M.norm(a)
        assert M.value(r) == M.value(a) and all(0 <= v < B29 for v in r[:8])
    for a in bound_vectors(B29 - 1, TOP, rng, 200, nonneg=True):       # norm_x8: N-class input
        r = M.norm_x8(a)
        assert M.value(r) == 8 * M.value(a) and all(0 <= v < B29 for v in r[:8])
    vs = bound_vectors(B29 - 1, B29 - 1, rng, 40)                      # norm_sub3: |limbs| < 2^29, the top limb included
    for a in vs:
        for b in vs:
            r = M.norm_sub3(a, b)
            assert M.value(r) == M.value(a) - 3 * M.value(b) and all(0 <= v < B29 for v in r[:8])
    M.norm_sub3([B29 - 1] * 9, [-(B29 - 1)] * 9)                      # the i32 sums reach 2^31 - 1 ...
    M.norm_sub3([-(B29 - 1)] * 9, [B29 - 1] * 9)                      # ... and -2^31 exactly
    with pytest.raises(M.Overflow):
        M.norm_sub3([B29] * 9, [-B29] * 9)                             # one past: |limbs| = 2^29 wraps


def check_reduce(r, x):
    assert congruent(r, x) and all(0 <= v < B29 for v in r[:8])
    assert abs(M.value(r)) * 100 < 51 * P                              # |V| < 0.51
    return abs(Fraction(M.value(r), P))


def expected_reduce_digits(limbs):
    """the pass as a formula: q = floor((t8 K + 2^43) / 2^44) with the header's K, result = the digits of value - q p"""
    src = open(HDR).read()
    k = int(re.search(r"t8 \* (\d+)ll \+ \(1ll << 43\)", src).group(1))
    q = (limbs[8] * k + (1 << 43)) // (1 << 44)
    return M.digits(sum(x << (29 * i) for i, x in enumerate(limbs)) - q * P)


def test_reduce_from_at_2_36_and_on_rounding_boundaries():
    rng = random.Random(5)
    cases = reduce_cases(rng, n_random=300)
    worst = 0
    for a, b, k0, k1 in cases:
        limbs = reduce_limbs(a, b, k0, k1)
        assert all(abs(x) < 1 << 36 for x in limbs[:8]) and abs(limbs[8]) < 1 << 31
        r = M.reduce_from(limbs)
        worst = max(worst, check_reduce(r, M.value(limbs)))
        assert r == expected_reduce_digits(limbs), limbs
    assert Fraction(50, 100) < worst < Fraction(51, 100)              # the cases do reach the rounding edge
    assert any(max(abs(x) for x in reduce_limbs(*c)[:8]) == (1 << 36) - 1 for c in cases)


def test_quotient_boundaries_are_sensitive_to_k():
    """each rounding_t8 value changes q when K moves by one: a device or model with K +- 1 cannot pass the reduce tests"""
    ts = rounding_t8()
    q = lambda t, k: (t * k + (1 << 43)) >> 44
    assert any(q(t, M.K + 1) != q(t, M.K) for t in ts) and any(q(t, M.K - 1) != q(t, M.K) for t in ts)


def test_reduce_terms_and_norm_terms_match_reduce_from():
    rng = random.Random(6)
    vs = bound_vectors(B29 - 1, TOP_V, rng, 30)                         # operands with |V| <= 8, as at the call sites
    for a in vs[::3]:
        for b in vs[::2]:
            for ka, kb in ((1, 1), (3, -2), (-30, 27), (54, 6)):
                limbs = reduce_limbs(a, b, ka, kb)
                r = M.reduce_terms([a, b], [ka, kb])
                assert r == M.reduce_from(limbs) == M.lin2(a, ka, b, kb)
                check_reduce(r, M.value(limbs))
                n = M.norm_terms([a, b], [ka, kb])
                assert M.value(n) == M.value(limbs) and all(0 <= v < B29 for v in n[:8])


def test_xi_lin_at_its_stated_bounds():
    """u2_xi_lin: low limbs of x, y at +-(2^31 - 1), top limbs at the tightened bound 10 |k| |x[8]| + |m| |y[8]| < 2^31"""
    lim = (1 << 31) - 1
    for k, m in ((1, 1), (3, 2), (-1, 1), (1, 0)):
        top = ((1 << 31) - 1) // (10 * abs(k) + abs(m))
        for kx in ("pos", "neg", "alt", "tla"):
            for ts in (1, -1):
                x0 = pattern(lim, 0, kx)[:8] + [ts * top]
                x1 = [-v for v in x0[:8]] + [-ts * top]
                y = pattern(lim, 0, kx)[:8] + [ts * top]
                c0, c1 = M.u2_xi_lin(x0, x1, y, y, k, m)
                xv0, xv1, yv = M.value(x0), M.value(x1), M.value(y)
                check_reduce(c0, k * (9 * xv0 - xv1) + m * yv)
                check_reduce(c1, k * (xv0 + 9 * xv1) + m * yv)


def test_xi_lin_needs_its_top_limb_condition():
    """why u2_xi_lin bounds its top limbs separately: at |x[8]|, |y[8]| = 2^31 - 1 (inside a plain "|limbs| < 2^31") the combined top
    limb reaches 32 (2^31 - 1) > 2^31 and the reduce pass misses |V| < 0.51"""
    lim = (1 << 31) - 1
    x0 = [0] * 8 + [lim]
    x1 = [0] * 8 + [-lim]
    y = [0] * 8 + [lim]
    c0, _ = M.u2_xi_lin(x0, x1, y, y, 3, 2)
    assert congruent(c0, 3 * (9 * M.value(x0) - M.value(x1)) + 2 * M.value(y))
    assert abs(M.value(c0)) * 100 > 51 * P


def test_to_fp_on_the_whole_input_range():
    rng = random.Random(7)
    inv32 = pow(32, -1, P)
    for a in to_fp_cases(rng, n_random=300):
        w = M.to_fp(a)
        assert all(0 <= x < 1 << 32 for x in w)
        assert M.words_value(w) == M.value(a) * inv32 % P, a  # canonical, not only congruent
    with pytest.raises(M.Overflow):
        M.to_fp(M.digits(-64 * P - (1 << 240)))               # below -64 p the offset value goes negative


def test_from_fp_round_trip():
    rng = random.Random(8)
    for x in [0, 1, P - 1, (1 << 256) - 1, 1 << 255] + [rng.randrange(1 << 256) for _ in range(200)]:
        a = M.from_fp(M.int_to_words(x))
        assert M.value(a) == (32 * x) % (1 << 261) and all(0 <= v < B29 for v in a)
        if x < P:
            assert M.words_value(M.to_fp(a)) == x


def test_from_plain_on_every_256_bit_word():
    """f29_from_plain (plk_multi.hip) feeds the raw words of the table-driven Miller loop -- G1 coordinates and line coefficients -- to
    the carry-free core.  The header lets a caller pass any 256-bit word (>= p reduced like Fp::new), up to 2^256 - 1 ~ 5.29 p: the
    digits are exact (the top digit takes bits 232..255), the product by R'^2 wraps no i32 / i64 (the model raises), and the output is
    the N class the comment claims -- normalized, value = X R' mod p up to a multiple of p, inside [-(V/169) p, (V/169 + 1) p), V < 5.3"""
    src = open(os.path.join(ROOT, "sylow_amd", "csrc", "plk_multi.hip")).read()
    rr = re.search(r"BN_DEV F29 f29_from_plain\(const Fp& x\) \{.*?const F29 rr\{\{([^}]*)\}\};", src, re.S).group(1)
    assert [int(x, 16) for x in rr.split(",")] == M.RR and M.value(M.RR) == M.RP * M.RP % P
    rng = random.Random(9)
    top = (1 << 256) - 1
    xs = [0, 1, P - 1, P, P + 1, 2 * P, 5 * P, top - 5 * P, top - 5 * P + 1, top, top - 1, 1 << 255, (1 << 256) - (1 << 232)]
    xs += [sum(((1 << 29) - 1 if (i + j) % 2 else 0) << (29 * i) for i in range(9)) & top for j in range(2)]   # alternating full digits
    xs += [rng.randrange(1 << 256) for _ in range(300)] + [rng.randrange(P) + k * P for k in range(1, 6) for _ in range(20)]
    worst = 0.0
    for x in xs:
        if x > top:
            continue
        w = M.int_to_words(x)
        d = M.plain_digits(w)
        assert M.value(d) == x and all(0 <= v < B29 for v in d[:8]) and 0 <= d[8] < 1 << 24, hex(x)
        r = M.from_plain(w)                                   # raises Overflow on any wrap
        v = M.value(r)
        assert M.normalized(r) and M.L(r) <= 1, hex(x)
        assert (v - x * M.RP) % P == 0, hex(x)
        bound = M.V(d) * M.V(M.RR) / 169
        assert -bound * P <= v < (bound + 1) * P, hex(x)
        worst = max(worst, M.V(d))
    assert 5.28 < worst < 5.3                                 # 2^256 / p = 5.29
    # the representatives of one value give congruent outputs: the kernels' results (canonical on the way out) are the same
    for x in (0, 1, P - 1, rng.randrange(P)):
        outs = {M.value(M.from_plain(M.int_to_words(x + k * P))) % P for k in range(6) if x + k * P <= top}
        assert len(outs) == 1


# ---- call sites ------------------------------------------------------------------------------------------------------------------
# Every coefficient the kernels pass to the linear passes.  Keys: ("call", file, wrapper, first coefficient, second coefficient) for the
# u2_/w2_/f29_ lin2 and xi_lin wrappers, ("init", file, initializer text) for the coefficient arrays handed to f29_reduce_terms /
# f29_norm_terms directly.  Values: (pass, operand low-limb bound, [every lane / branch variant of the coefficient vector]) -- xi_lin
# variants are written out as the reduce_terms vector (9k, +-k, m) over (x, partner's x, y), u2_xi_lin as (k, m).  The operand bound
# is what the site's comment states: R / N operands 2^29, lazy sums of two 2^30, three 3 2^29, "any 32-bit limbs" 2^31 - 1.  Operand
# values are |V| <= 8 (R, N and products have |V| < 2, the lazy combinations add at most four of them), so top limbs <= 8 p / 2^232;
# an optional fourth entry gives a tighter |V| (the norm_terms sites, whose output must stay a product operand).
# None: the wrapper's own body, covered by its callers' rows.
VMAX = 8                                     # operand |V| at the reduce sites
VMAX_RN = Fraction(12, 10)                   # R / N operands (reduced |V| < 0.51, product outputs |V| < 1.2): the norm_terms sites
XI = lambda k, m: [(9 * k, k, m), (9 * k, -k, m)]
F, W = "bn254_f29.hpp", "bn254_pair29.hpp"
CALL_SITES = {
    ("call", F, "u2_lin2", "1", "-1"): ("reduce", 1 << 30, [(1, -1)]),
    ("call", F, "u2_lin2", "1", "1"): ("reduce", 1 << 30, [(1, 1)]),
    ("call", F, "u2_lin2", "3", "-2"): ("reduce", 1 << 30, [(3, -2)]),
    ("call", F, "u2_lin2", "3", "2"): ("reduce", 1 << 30, [(3, 2)]),
    ("call", F, "u2_xi_lin", "1", "1"): ("xi_lin", (1 << 31) - 1, [(1, 1)]),
    ("call", F, "u2_xi_lin", "3", "2"): ("xi_lin", (1 << 31) - 1, [(3, 2)]),
    ("call", W, "w2_lin2", "1", "-1"): ("reduce", 1 << 30, [(1, -1)]),
    ("call", W, "w2_lin2", "1", "-3"): ("reduce", 1 << 30, [(1, -3)]),
    ("call", W, "w2_lin2", "1", "1"): ("reduce", 1 << 30, [(1, 1)]),
    ("call", W, "w2_lin2", "6", "2"): ("reduce", 1 << 30, [(6, 2)]),
    ("call", W, "w2_xi_lin", "-1", "1"): ("reduce", 1 << 30, XI(-1, 1)),
    ("call", W, "w2_xi_lin", "1", "0"): ("reduce", 1 << 30, [(9, 1), (9, -1)]),
    ("call", W, "w2_xi_lin", "1", "1"): ("reduce", 1 << 30, XI(1, 1)),
    ("call", W, "w2_xi_lin", "6", "2"): ("reduce", 1 << 30, XI(6, 2)),
    ("call", F, "f29_lin2", "ka", "kb"): None,
    ("call", "runtime.hip", "f29_lin2", "k0", "k1"): None,              # the raw test hook: its coefficients are the tests' own
    ("call", "runtime.hip", "u2_xi_lin", "k0", "k1"): None,
    ("init", "runtime.hip", "bn_keep(k0), bn_keep(k1)"): None,
    ("init", "runtime.hip", "bn_keep(q[0]), bn_keep(q[1]), bn_keep(q[2]), bn_keep(q[3])"): None,
    ("call", W, "f29_lin2", "ka", "kb"): None,
    ("init", F, "bn_keep(ka), bn_keep(kb)"): None,
    ("init", W, "bn_keep(9 * k), bn_keep_v(lane_odd() ? k : -k)"): None,
    ("init", W, "bn_keep(9 * k), bn_keep_v(lane_odd() ? k : -k), bn_keep(m)"): None,
    ("init", W, "bn_keep(1)"): ("reduce", (1 << 31) - 1, [(1,)]),
    ("init", W, "bn_keep(-9), bn_keep_v(lane_odd() ? -1 : 1), bn_keep(1)"): ("norm", 1 << 29, [(-9, -1, 1), (-9, 1, 1)], VMAX_RN),
    ("init", W, "bn_keep(9), bn_keep_v(lane_odd() ? 1 : -1), bn_keep(1)"): ("norm", 1 << 29, [(9, 1, 1), (9, -1, 1)], VMAX_RN),
    ("init", W, "bn_keep(1), bn_keep(-1), bn_keep(-1)"): ("reduce", 3 << 29, [(1, -1, -1)]),
    ("init", W, "bn_keep(1), bn_keep_v(m)"): ("reduce", 1 << 30, [(1, 0), (1, 1)]),
    ("init", W, "bn_keep(27), bn_keep_v(lane_odd() ? -3 : 3)"): ("reduce", (1 << 31) - 1, [(27, -3), (27, 3)]),
    ("init", W, "bn_keep(3), bn_keep(30), bn_keep_v(lane_odd() ? 3 : -3), bn_keep(-2)"): ("reduce", 1 << 30, [(3, 30, 3, -2), (3, 30, -3, -2)]),
    ("init", W, "bn_keep(9), bn_keep_v(lane_odd() ? 1 : -1), bn_keep(1), bn_keep(1)"): ("reduce", 1 << 30, [(9, 1, 1, 1), (9, -1, 1, 1)]),
    ("init", W, "bn_keep(9), bn_keep_v(lane_odd() ? 1 : -1), bn_keep(1), bn_keep_v(u)"):
        ("reduce", 1 << 30, [(9, s, 1, u) for s in (1, -1) for u in (0, 1)]),
    ("init", W, "bn_keep(9), bn_keep_v(lane_odd() ? 1 : -1), bn_keep_v(m)"): ("reduce", 1 << 30, [(9, s, u) for s in (1, -1) for u in (0, 1)]),
    ("init", W, "bn_keep_v(9 * kx), bn_keep_v(lo ? kx : -kx), bn_keep_v(c == 0 ? 0 : 1), bn_keep_v(c == 0 ? 1 : -1), "
                "bn_keep_v(c == 0 ? 0 : c == 1 ? -1 : 1), bn_keep_v(c == 2 ? -1 : 0)"):
        ("reduce", 1 << 30, [(9, 1, 0, 1, 0, 0), (9, -1, 0, 1, 0, 0), (9, 1, 1, -1, -1, 0), (9, -1, 1, -1, -1, 0), (0, 0, 1, -1, 1, -1)]),
    ("init", W, "bn_keep_v(hi ? -1 : 1), bn_keep_v(hi ? -1 : o0 ? 9 : 1), bn_keep_v(o0 ? (lo ? 1 : -1) : 0), bn_keep_v(hi ? 1 : 0)"):
        ("reduce", 1 << 30, [(-1 if hi else 1, -1 if hi else 9 if o0 else 1, (1 if lo else -1) if o0 else 0, 1 if hi else 0)
                             for hi in (0, 1) for o0 in (0, 1) for lo in (0, 1)]),
    ("init", W, "bn_keep_v(hi ? 2 : -1), bn_keep_v(hi ? 0 : o0 ? -9 : -1), bn_keep_v(o0 ? (lo ? -1 : 1) : 0), bn_keep_v(hi ? 0 : 1)"):
        ("reduce", 1 << 30, [(2 if hi else -1, 0 if hi else -9 if o0 else -1, (-1 if lo else 1) if o0 else 0, 0 if hi else 1)
                             for hi in (0, 1) for o0 in (0, 1) for lo in (0, 1)]),
    ("init", W, "bn_keep_v(ta ? 3 : 0), bn_keep_v(ta ? -30 : tc ? 54 : 6), bn_keep_v(ta ? (lo ? -3 : 3) : tc ? (lo ? 6 : -6) : 0), "
                "bn_keep_v(ta ? -2 : 2)"):
        ("reduce", 1 << 30, [(3, -30, -3, -2), (3, -30, 3, -2), (0, 54, 6, 2), (0, 54, -6, 2), (0, 6, 0, 2)]),
}
TOP_V = int(VMAX * PT) + 1                   # the top limb of an operand with |V| <= 8


def _split_top(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "([{"
        depth -= ch in ")]}"
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def source_call_sites():
    """the keys of CALL_SITES, read from every kernel source"""
    found = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        text = re.sub(r"//[^\n]*", "", open(path).read())
        name = os.path.basename(path)
        for m in re.finditer(r"\b(w2_xi_lin|u2_xi_lin|w2_lin2|u2_lin2|f29_lin2)\(", text):
            i, depth = m.end(), 1
            while depth:
                depth += {"(": 1, ")": -1}.get(text[i], 0)
                i += 1
            args = _split_top(text[m.end():i - 1])
            if not args[0].startswith("const "):                      # skip the definitions
                found.add(("call", name, m.group(1), args[1], args[3]))
        for m in re.finditer(r"const i32 \w+\[\d\] = \{([^;]*bn_keep[^;]*)\};", text):
            found.add(("init", name, " ".join(m.group(1).split())))
    return found


def test_call_site_table_matches_the_sources():
    """a new call site, or a changed coefficient at an existing one, must be added to CALL_SITES (and so to the bound checks below)"""
    found = source_call_sites()
    assert found == set(CALL_SITES), ("not in the table:", sorted(found - set(CALL_SITES)), "gone from the sources:",
                                      sorted(set(CALL_SITES) - found))
    # f29_reduce_terms / f29_norm_terms get their coefficients only from the arrays above, plus the raw test hook's own
    users = set()
    for path in glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(CSRC, "*.hip")):
        if re.search(r"\bf29_(?:reduce|norm)_terms\(", re.sub(r"//[^\n]*", "", open(path).read())):
            users.add(os.path.basename(path))
    assert users == {"bn254_f29.hpp", "bn254_pair29.hpp", "runtime.hip"}, users


def site_operands(lim, top, kvec, sign):
    """operands at the bound with every column term of one sign: x_j limbs = sign sgn(k_j) lim (the alternation as a second case)"""
    out = []
    for k in kvec:
        s = sign * (1 if k >= 0 else -1)
        out.append([s * lim] * 8 + [s * top])
    return out


def test_call_site_coefficients_at_maximal_limbs():
    checked = 0
    for key, row in CALL_SITES.items():
        if row is None:
            continue
        kind, lim, variants = row[:3]
        top = int((row[3] if len(row) > 3 else VMAX) * PT) + 1
        for kvec in variants:
            if kind == "xi_lin":
                k, m = kvec
                assert (10 * abs(k) + abs(m)) * lim < 1 << 36, key
                top = ((1 << 31) - 1) // (10 * abs(k) + abs(m))
                for s in (1, -1):
                    x0 = [s * lim] * 8 + [s * top]
                    x1 = [-s * lim] * 8 + [-s * top]
                    c0, c1 = M.u2_xi_lin(x0, x1, x0, x1, k, m)
                    check_reduce(c0, k * (9 * M.value(x0) - M.value(x1)) + m * M.value(x0))
                    check_reduce(c1, k * (M.value(x0) + 9 * M.value(x1)) + m * M.value(x1))
                    checked += 1
                continue
            weight = sum(abs(k) for k in kvec)
            assert weight * lim < 1 << 36, (key, kvec)               # combined low limbs inside the reduce pass's 2^36
            assert weight * top < 1 << 31, (key, kvec)               # combined top limb inside its 2^31
            for sign in (1, -1):
                for alt in (False, True):
                    xs = site_operands(lim, top, kvec, sign)
                    if alt:
                        xs = [[v * (-1) ** i for i, v in enumerate(x[:8])] + [x[8]] for x in xs]
                    x = sum(k * M.value(v) for k, v in zip(kvec, xs))
                    if kind == "reduce":
                        check_reduce(M.reduce_terms(xs, list(kvec)), x)
                    else:
                        r = M.norm_terms(xs, list(kvec))
                        assert M.value(r) == x and all(0 <= v < B29 for v in r[:8]) and abs(r[8]) < 1 << 28
                    checked += 1
    assert checked > 200


def test_largest_call_site_weights():
    """the figures the header's comments quote: largest reduce weight sum |k| = 62, u2_xi_lin's 10 |k| + |m| = 32"""
    w = max(sum(abs(k) for k in v) for row in CALL_SITES.values() if row and row[0] != "xi_lin" for v in row[2])
    x = max(10 * abs(k) + abs(m) for row in CALL_SITES.values() if row and row[0] == "xi_lin" for k, m in row[2])
    assert (w, x) == (62, 32)
