"""A CPU model of the Fr arithmetic core (sylow_amd/csrc/bn254_fr.hpp, bn254_fr_acc.hpp, bn254_fr_euclid.hpp).  Not collected by pytest,
plain integers only, and it shares nothing with sylow_amd.

    barrett(T)   fr_reduce_wide limb by limb: the columns 7 .. 17 of T[7..15] x MU (the columns below are dropped, as on the device), q3 from
                 column 9 on, q3 r to 9 limbs, the low 256 bits of T - q3 r, then the conditional subtractions of 2r and r.  It returns the
                 result and the CLASS of T: how many times r fits into T - q3 r, i.e. how many corrections the input needs.
    euclid(a)    fr_euclid::inverse step by step: (a^-1 mod r, the steps taken).

and the inputs that force the branches random values do not take: products a b = s mod r with s next to 0 (every one needs the final
subtraction) or next to r (none does), sums of 16 products with the same property, and structured inputs for the inversion."""
import random

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
TOP = (1 << 256) - 1
MU = (1 << 512) // R                       # 9 limbs: BN_FR_MU
M32 = (1 << 32) - 1
MAX_STEPS = 1016                           # fr_euclid::MAX_STEPS
FLUSH = 16                                 # products between two folds of an unreduced accumulator (SPMV_FLUSH, LINCOMB_FLUSH, the PLONK gate sums)


def _limbs(x, n):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def _columns(a, b, lo, hi, a_max, b_max):
    """the column sums of a x b for the columns lo .. hi - 1 through the device's accumulator (64 bits and 32 of overflow): one limb a column,
    the carry of the last column returned beside them"""
    acc, out = 0, []
    for k in range(lo, hi):
        for i in range(max(0, k - b_max), min(k, a_max) + 1):
            acc += a[i] * b[k - i]
        assert acc < 1 << 96, "the column accumulator holds 96 bits"
        out.append(acc & M32)
        acc >>= 32
    return out, acc


def _cond_sub(x, c):
    return x - c if x >= c else x


def barrett(T, final_sub=True):
    """(T mod r as fr_reduce_wide forms it, cls) for 0 <= T < 2^512; cls = (T - q3 r) // r as exact integers, before any correction.
    final_sub False is the FAULT the directed inputs are there for: the last conditional subtraction of r left out."""
    assert 0 <= T < 1 << 512
    t = _limbs(T, 16)
    # q3: columns 7 .. 17 of T[7..15] x MU, kept from column 9 on; column 17 is T[15] MU[8] alone and its carry is dropped (it is zero)
    cols, carry = _columns(t[7:], _limbs(MU, 9), 7, 18, 8, 8)
    assert carry == 0, "q3 fits 9 limbs"
    q3 = cols[2:]
    assert len(q3) == 9
    # q3 r to 9 limbs (mod 2^288); only 8 of them meet T
    qp, _ = _columns(q3, _limbs(R, 8), 0, 9, 8, 7)
    c, low = 0, []
    for i in range(8):
        c += t[i] - qp[i]
        low.append(c & M32)
        c >>= 32                           # arithmetic shift: the borrow
    diff = sum(v << (32 * i) for i, v in enumerate(low))
    exact = T - sum(v << (32 * i) for i, v in enumerate(q3)) * R
    assert exact == diff, "the remainder before correction is the 256-bit difference: nothing wrapped"
    x = _cond_sub(diff, 2 * R)
    if final_sub:
        x = _cond_sub(x, R)
    return x, exact // R


def euclid(a, max_steps=MAX_STEPS):
    """(a^-1 mod r, steps) for a in [1, r) by the binary extended Euclid of fr_euclid::inverse; 0 when the step bound ends the loop.
    max_steps below the device's 1016 is the FAULT the structured inputs are there for: a bound that is too small."""
    assert 0 <= a < R
    u, v, x1, x2, steps = a, R, 1, 0, 0

    def half_mod(x):
        return (x + R if x & 1 else x) >> 1

    while steps < max_steps and u != 1 and v != 1:
        if not u & 1:
            u, x1 = u >> 1, half_mod(x1)
        elif not v & 1:
            v, x2 = v >> 1, half_mod(x2)
        elif u >= v:
            u, x1 = u - v, (x1 - x2) % R
        else:
            v, x2 = v - u, (x2 - x1) % R
        assert 0 <= u < 1 << 256 and 0 <= v < 1 << 256
        steps += 1
    return (x1 if u == 1 else x2 if v == 1 else 0), steps


def lifts(x):
    """every 256-bit word of the residue of x but the canonical one"""
    x %= R
    return [x + j * R for j in range(1, (TOP - x) // R + 1)]


def lift(x, rng=None):
    """the largest word of the residue of x, or with rng any but the canonical one"""
    words = lifts(x)
    return rng.choice(words) if rng else words[-1]


def product_pairs(rng, s, count, lift_mode=None):
    """count pairs (a, b) with a b = s mod r: a canonical and not 0, b = s a^-1.  lift_mode None leaves both canonical, "top" replaces each
    by the largest 256-bit word of its residue, "random" by any non-canonical one."""
    assert lift_mode in (None, "top", "random")
    out = []
    for _ in range(count):
        a = rng.randrange(1, R)
        b = s * pow(a, R - 2, R) % R
        assert a * b % R == s % R
        if lift_mode:
            a, b = (lift(v, rng if lift_mode == "random" else None) for v in (a, b))
        out.append((a, b))
    return out


def wide_terms(rng, s, terms, weights=None):
    """`terms` canonical pairs (w_j, a_j) with sum_j w_j a_j = s mod r; the last pair is solved from the others.  weights: the w_j to use
    (canonical, the last one not 0), for columns that share them."""
    w = list(weights) if weights is not None else [rng.randrange(1, R) for _ in range(terms)]
    assert len(w) == terms and all(0 <= v < R for v in w) and w[-1]
    a = [rng.randrange(R) for _ in range(terms - 1)]
    rest = sum(x * y for x, y in zip(w, a))
    a.append((s - rest) * pow(w[-1], R - 2, R) % R)
    assert sum(x * y for x, y in zip(w, a)) % R == s % R
    return list(zip(w, a))


def folds(pairs):
    """the 16-limb values an unreduced accumulator hands to fr_reduce_wide: FLUSH products on top of the residue of the round before"""
    out, res = [], 0
    for at in range(0, len(pairs), FLUSH):
        T = res + sum(w * a for w, a in pairs[at:at + FLUSH])
        out.append(T)
        res = T % R
    return out


def _dedup(words):
    out = []
    for w in words:
        assert 0 <= w <= TOP
        if w not in out:
            out.append(w)
    return out


EDGE = _dedup([k * R + d for k in range(6) for d in (-1, 0, 1) if 0 <= k * R + d <= TOP] +
              [2, (R - 1) // 2, (R + 1) // 2, 1 << 255, TOP - 1, TOP, P, P - 1] +
              [(1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 64, (1 << 224) - 1, 1 << 224, 1 << 253] +      # limb 7 is the cut of Barrett's q1
              [M32 << (32 * i) for i in range(8)])
STRUCTURED = _dedup([1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2] + [1 << k for k in range(1, 254)] + [(1 << k) - 1 for k in range(2, 254)] +
                    [R - (1 << k) for k in range(1, 253)])
assert all(0 < x < R for x in STRUCTURED)

FORCED_S = (0, 1, 2, R - 2, R - 1)
FORCED_PER_S = 64


def forced_pairs():
    """the pairs the device test multiplies, the same list on every call: for each s, 64 canonical pairs, then 64 lifted ones (the largest
    lift and random lifts by turns)"""
    rng = random.Random(0xF0C0)
    out = []
    for s in FORCED_S:
        out += product_pairs(rng, s, FORCED_PER_S)
        for i in range(FORCED_PER_S // 2):
            out += product_pairs(rng, s, 1, "top") + product_pairs(rng, s, 1, "random")
    return out


WIDE_TERMS = (FLUSH, FLUSH + 1, 2 * FLUSH + 1)     # one fold, a fold and a residue, two folds and a residue
WIDE_S = (0, 1, R - 1)


def wide_groups(columns):
    """the groups the device test folds, the same on every call: for every (terms, s) the shared weights [terms] and, for each of `columns`
    columns, the a_j [terms] whose products with the weights sum to s"""
    rng = random.Random(0xF0C1)
    out = []
    for terms in WIDE_TERMS:
        for s in WIDE_S:
            w = [rng.randrange(1, R) for _ in range(terms)]
            cols = [[a for _, a in wide_terms(rng, s, terms, w)] for _ in range(columns)]
            out.append((terms, s, w, cols))
    return out


def forced_squares():
    """every non-canonical word of the residues 1 and r - 1, and the canonical two: each square is 1 mod r"""
    return [1, R - 1] + lifts(1) + lifts(R - 1)
