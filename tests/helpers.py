"""Shared test helpers: deterministic inputs (SplitMix64-seeded xoshiro256**)."""
import os

import numpy as np

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
M64 = (1 << 64) - 1
SEED = int(os.environ.get("SYLOW_TEST_SEED", "0x53594C4F57"), 0)  # "SYLOW"; another seed re-draws every PRNG-built input of the suite


class Xoshiro:
    def __init__(self, seed):
        s = []
        x = seed & M64
        for _ in range(4):  # SplitMix64
            x = (x + 0x9E3779B97F4A7C15) & M64
            z = x
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            s.append(z ^ (z >> 31))
        self.s = s

    def next(self):
        s = self.s
        r = (((s[1] * 5) & M64) << 7 | ((s[1] * 5) & M64) >> 57) & M64
        r = (r * 9) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]
        s[2] ^= t
        s[3] = ((s[3] << 45) | (s[3] >> 19)) & M64
        return r

    def fp(self):
        """uniform in [0, p) by rejection of 256-bit draws"""
        while True:
            v = self.next() | (self.next() << 64) | (self.next() << 128) | (self.next() << 192)
            v &= (1 << 254) - 1
            if v < P:
                return v

    def u256(self):
        return self.next() | (self.next() << 64) | (self.next() << 128) | (self.next() << 192)


def limbs(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (int(v) >> (64 * k)) & M64
    return out


def pack(vals, width):
    return limbs(vals).reshape(-1, width)


def ints(arr):
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(arr[i, k]) << (64 * k) for k in range(4)) for i in range(arr.shape[0])]


def rand_fp_array(rng, n, width_fp):
    """n elements of width_fp Fp each -> (n, 4*width_fp) uint64"""
    return limbs([rng.fp() for _ in range(n * width_fp)]).reshape(n, 4 * width_fp)


def fast_rand_fp_array(seed, n, width_fp):
    """numpy-generated values < 2^253 (< p): for large batches where python-int loops are too slow"""
    g = np.random.default_rng(seed)
    a = g.integers(0, 1 << 63, size=(n, width_fp, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, size=(n, width_fp, 4), dtype=np.uint64)
    a[:, :, 3] &= np.uint64((1 << 61) - 1)
    return a.reshape(n, 4 * width_fp)


def _R():
    from oracle import pyref
    return pyref


def fp2_sqrt(a):
    """sqrt in Fp2 = Fp[u]/(u^2+1), p = 3 mod 4 (complex method); None if a is not a square"""
    a0, a1 = a
    if a1 == 0:
        s = _R().fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = _R().fp_sqrt((-a0) % P)
        return (0, s)
    n = _R().fp_sqrt((a0 * a0 + a1 * a1) % P)
    if n is None:
        return None
    for nn in (n, (-n) % P):
        h = (a0 + nn) * _R().fp_inv(2) % P
        x0 = _R().fp_sqrt(h)
        if x0 is not None and x0 != 0:
            x1 = a1 * _R().fp_inv(2 * x0 % P) % P
            if _R().fp2_square((x0, x1)) == (a0 % P, a1 % P):
                return (x0, x1)
    return None


# ---- crafted inputs: values whose INTERNAL 29-bit digits are extreme, Fp12 shapes, points off the usual random path -------------------
M29 = (1 << 29) - 1
RP_INV = pow(pow(2, 261, P), P - 2, P)           # the carry-free core holds x * 2^261 mod p
TOP_BOUND = P >> 233                             # |top limb| of a value near p / 2


def crafted_values():
    """canonical x whose internal representation v = x * 2^261 mod p (centred, |v| < p / 2) has extreme digits: low limbs all 2^29 - 1,
    zero, alternating, or 2^28, under top limbs from 0 to the bounds +-p / 2^234; then 1 and p - 1 (0 is the all-zero pattern)"""
    lows = [sum(M29 << (29 * i) for i in range(8)),                       # all ones
            0,                                                             # all zero
            sum((M29 if i % 2 else 0) << (29 * i) for i in range(8)),      # alternating
            sum((M29 if i % 2 == 0 else 1) << (29 * i) for i in range(8)),
            sum((1 << 28) << (29 * i) for i in range(8))]
    tops = [0, 1, -1, 1_400_000, -1_400_000, 700_001, -700_001]
    out = []
    for lo in lows:
        for t in tops:
            v = lo + (t << 232)
            assert abs(v) < 0.46 * P
            out.append(v * RP_INV % P)
    # the top limb at its bounds: -TOP_BOUND is reached as given; TOP_BOUND - 1 with these low limbs lies above p / 2 by less than the
    # reduce pass's rounding, which maps it to its negative representative (top limb -TOP_BOUND - 1 or - 2)
    for lo in lows:
        for t in (1_585_000, -TOP_BOUND, TOP_BOUND - 1):
            out.append((lo + (t << 232)) * RP_INV % P)
    return out + [1, P - 1]


def fp_cbrt(a):
    """a cube root of a in Fp, or None.  p = 1 mod 9, so the 3-Sylow part needs a discrete log (Adleman-Manders-Miller)"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 3, P) != 1:
        return None
    s, t = 0, P - 1
    while t % 3 == 0:
        t //= 3
        s += 1
    z = 2
    while pow(z, (P - 1) // 3, P) == 1:
        z += 1
    c = pow(z, t, P)                              # generates the subgroup of order 3^s
    x0 = pow(a, pow(3, -1, t), P)                 # x0^3 = a * b with b = a^(t m) in that subgroup
    b = pow(x0, 3, P) * pow(a, P - 2, P) % P
    g = pow(c, 3 ** (s - 1), P)                   # order 3
    j = 0
    for k in range(s):                            # b = c^j, digit by digit
        h = pow(b * pow(c, (3 ** s - j) % 3 ** s, P) % P, 3 ** (s - 1 - k), P)
        j += [1, g, g * g % P].index(h) * 3 ** k
    assert j % 3 == 0
    x = x0 * pow(c, (3 ** s - j // 3) % 3 ** s, P) % P
    assert pow(x, 3, P) == a
    return x


def crafted_g1_points(count=None):
    """affine G1 points (x, y) on y^2 = x^3 + 3 with a crafted x, and with a crafted y (x = cbrt(y^2 - 3)), alternating"""
    R = _R()
    vals = crafted_values()
    by_x, by_y = [], []
    for v in vals:
        y = R.fp_sqrt((v * v * v + 3) % P)
        if y is not None:
            by_x.append((v, y))
        x = fp_cbrt((v * v - 3) % P)
        if x is not None:
            by_y.append((x, v))
    out = [pt for pair in zip(by_x, by_y) for pt in pair]
    return out[:count] if count else out


def crafted_g2_points(count=None):
    """affine twist points (x, y), x = (c0, c1) from the crafted values, y = sqrt(x^3 + b'): on the curve, NOT in the r-torsion"""
    R = _R()
    vals = crafted_values()
    out = []
    for k, v in enumerate(vals):
        x = (v, vals[(7 * k + 3) % len(vals)])
        y = fp2_sqrt(R.fp2_add(R.fp2_mul(R.fp2_square(x), x), R.TWIST_B))
        if y is not None:
            out.append((x, y))
    return out[:count] if count else out


def crafted_g2_projective(count=None):
    """homogeneous (X, Y, Z) = (x Z, y Z, Z) over crafted twist points with a crafted Z in Fp2"""
    R = _R()
    vals = crafted_values()
    out = []
    for k, (x, y) in enumerate(crafted_g2_points()):
        z = (vals[(5 * k + 1) % len(vals)], vals[(11 * k + 2) % len(vals)])
        if z == (0, 0):
            z = (vals[k % len(vals)] or 1, 0)
        out.append((R.fp2_mul(x, z), R.fp2_mul(y, z), z))
    return out[:count] if count else out


def crafted_fp12_rows():
    """Fp12 elements (12 Fp coefficients each, in limb order c0.c0.c0, c0.c0.c1, ..., c1.c2.c1) of special shape: 0, 1, elements of the
    Fp, Fp2 and Fp6 subfields, c0 = 0, c1 = 0, one non-zero coefficient in each of the 12 slots, all 12 equal to one extreme value"""
    vals = crafted_values()
    ext = [v for v in vals if v not in (0, 1)]
    pick = lambda k: ext[(k * 13 + 5) % len(ext)]
    rows = [[0] * 12, [1] + [0] * 11]
    for k in range(3):
        rows.append([pick(k)] + [0] * 11)                                    # Fp
        rows.append([pick(k + 3), pick(k + 4)] + [0] * 10)                   # Fp2
        rows.append([pick(k + 6 + i) for i in range(6)] + [0] * 6)           # Fp6
        rows.append([0] * 6 + [pick(k + 12 + i) for i in range(6)])          # c0 = 0
        rows.append([pick(k + 18 + i) for i in range(6)] + [0] * 6)          # c1 = 0
    for slot in range(12):
        r = [0] * 12
        r[slot] = pick(slot + 24)
        rows.append(r)
    for v in (ext[0], ext[6], ext[-3], P - 1):
        rows.append([v] * 12)
    return rows


# ---- non-canonical representatives: the C ABI reduces inputs >= p like Fp::new (include/sylow_hip.h) ------------------------------
U256 = 1 << 256
REP_SPECIAL = [P, 2 * P, 5 * P, P + 1, U256 - 1]          # == 0, 0, 0, 1 and 2^256 - 1 - 5 p: the words a caller may pass raw
_KMAX5 = U256 - 5 * P                                      # x + 5 p fits 256 bits exactly when x < 2^256 - 5 p (5 p < 2^256 < 6 p)


def _add_limbs(a, b):
    """(N, 4) uint64 + (N, 4) uint64 with carries (no carry out: the callers stay below 2^256)"""
    out = np.empty_like(a)
    carry = np.zeros(a.shape[0], dtype=np.uint64)
    for k in range(4):
        s = a[:, k] + b[:, k]
        c1 = s < a[:, k]
        s2 = s + carry
        c2 = s2 < s
        out[:, k] = s2
        carry = (c1 | c2).astype(np.uint64)
    return out


def representatives(arr, seed=0, largest=False):
    """every 4-word Fp value x (canonical, < p) of a uint64 array of any shape replaced by x + k p, k >= 1: a random k in 1..4, or 1..5
    where x < 2^256 - 5 p (largest=False), or the largest k that fits (largest=True: 5 below 2^256 - 5 p, else 4, so the canonical
    value 2^256 - 1 - 5 p becomes 2^256 - 1).  Zeros take k = 1, 2, 5, 3, 4 in turn (p, 2p, 5p first) so that a handful of zero
    coordinates already meets the special words.  Same shape and dtype out."""
    a = np.ascontiguousarray(arr, dtype=np.uint64)
    x = a.reshape(-1, 4)
    assert ints_lt(x, P).all(), "representatives() needs canonical input"
    fits5 = ints_lt(x, _KMAX5)
    if largest:
        k = np.where(fits5, 5, 4)
    else:
        g = np.random.default_rng(seed)
        k = np.where(fits5, g.integers(1, 6, size=x.shape[0]), g.integers(1, 5, size=x.shape[0]))
        zero = ~x.any(axis=1)
        k[zero] = np.array([1, 2, 5, 3, 4])[np.arange(int(zero.sum())) % 5]
    kp = limbs([j * P for j in range(6)])
    return _add_limbs(x, kp[k]).reshape(a.shape)


def ints_lt(x, c):
    """row-wise x < c for (N, 4) little-endian uint64 limbs and an integer c < 2^256"""
    cl = limbs([c])[0]
    lt = np.zeros(x.shape[0], dtype=bool)
    eq = np.ones(x.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (x[:, k] < cl[k])
        eq &= x[:, k] == cl[k]
    return lt
