"""Exact host model of the carry-free field core (sylow_amd/csrc/bn254_f29.hpp): 9 signed limbs of 29 bits, value = sum v[i] 2^(29 i),
Montgomery factor R' = 2^261.  Every routine is transcribed step by step in plain Python integers -- the same column order, the same
i32 / u32 masking, the same arithmetic shifts -- so that its output limbs are exactly the device's.  Wherever the device holds an i64
accumulator or an i32 / u32 limb, the model checks that the value fits and raises Overflow instead of wrapping: a value that would wrap
on the device is a bounds violation, not a result.  tests/test_f29_model.py checks the routines against exact integer formulas at the
bounds the header states; tests/test_gpu_f29_bounds.py checks the device against this model through sylow_hip_f29_raw_hook_batch.

    python tools/f29_model.py            # prints the constants"""
import sys

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
M29 = (1 << 29) - 1
RP = 1 << 261                       # R', the Montgomery factor of this core
R = 1 << 256                        # the saturated core's Montgomery factor
P29 = [(P >> (29 * i)) & M29 for i in range(8)] + [P >> 232]
PINV29 = 0x04866389                 # -p^-1 mod 2^29 (BN_PINV29)
K = 5547168                         # quotient-estimate multiplier of f29_reduce_from / f29_reduce_terms
K64 = [((64 * P) >> (29 * i)) & M29 for i in range(8)] + [(64 * P) >> 232]     # digits of 64 p (f29_to_fp)
P4 = [((4 * P) >> (32 * i)) & 0xFFFFFFFF for i in range(8)]                      # 4p and 2p as 32-bit words (f29_to_fp)
P2 = [((2 * P) >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
P1 = [(P >> (32 * i)) & 0xFFFFFFFF for i in range(8)]

I32 = (-(1 << 31), 1 << 31)
U32 = (0, 1 << 32)
I64 = (-(1 << 63), 1 << 63)


class Overflow(ArithmeticError):
    """a device i32 / u32 / i64 value would wrap"""


def _fit(x, rng, what):
    if not rng[0] <= x < rng[1]:
        raise Overflow(f"{what}: {x} outside [{rng[0]}, {rng[1]})")
    return x


def i32(x, what="i32"): return _fit(x, I32, what)
def u32(x, what="u32"): return _fit(x, U32, what)
def i64(x, what="i64"): return _fit(x, I64, what)


def as_u32(x):
    """(u32)x of a signed value: the two's-complement low word (a cast, never an overflow)"""
    return x & 0xFFFFFFFF


def _vec(a):
    a = list(a)
    assert len(a) == 9, len(a)
    for i, x in enumerate(a):
        i32(x, f"input limb {i}")
    return a


# ---- describing a vector ------------------------------------------------------------------------------------------------
def value(a):
    return sum(x << (29 * i) for i, x in enumerate(a))


def L(a):
    """max_i<8 |a[i]| / 2^29 (the header's L)"""
    return max(abs(x) for x in a[:8]) / (1 << 29)


def V(a):
    """|value| / p (the header's V)"""
    return abs(value(a)) / P


def normalized(a):
    return all(0 <= x <= M29 for x in a[:8]) and abs(a[8]) < 1 << 28


def digits(x):
    """the normalized digits of an integer (top limb signed, may exceed 2^28 for |x| >= 2^260)"""
    d = [((x >> (29 * i)) & M29) for i in range(8)]
    return d + [x >> 232]


# ---- carry normalisation ---------------------------------------------------------------------------------------------------
def norm(a):
    a = _vec(a)
    r, c = [0] * 9, 0
    for i in range(8):
        t = i32(a[i] + c, f"norm t[{i}]")
        r[i] = t & M29
        c = t >> 29                                  # arithmetic shift
    r[8] = i32(a[8] + c, "norm top")
    return r


def norm_x8(a):
    a = _vec(a)
    r, c = [0] * 9, 0
    for i in range(8):
        t = u32((as_u32(a[i]) << 3) + c, f"norm_x8 t[{i}]")
        r[i] = t & M29
        c = t >> 29
    r[8] = i32(i32(a[8] * 8, "norm_x8 8 a[8]") + c, "norm_x8 top")
    return r


def norm_sub3(a, b):
    a, b = _vec(a), _vec(b)
    r, c = [0] * 9, 0
    for i in range(8):
        t = i32(i32(a[i] - i32(3 * b[i], f"norm_sub3 3 b[{i}]"), f"norm_sub3 a - 3b [{i}]") + c, f"norm_sub3 t[{i}]")
        r[i] = t & M29
        c = t >> 29
    r[8] = i32(i32(a[8] - i32(3 * b[8], "norm_sub3 3 b[8]"), "norm_sub3 a - 3b top") + c, "norm_sub3 top")
    return r


# ---- Montgomery products ----------------------------------------------------------------------------------------------------
def _mont_columns(column_products, name):
    """the shared column loop of f29_mul / f29_dot2 / f29_sqr: column_products(k, acc) adds the operand products of column k (with
    the device's overflow checks) and returns acc; the reduction products follow in the device's order"""
    m, r, acc = [0] * 9, [0] * 9, 0
    for k in range(17):
        lo, hi = (k - 8 if k > 8 else 0), (k if k < 8 else 8)
        acc = column_products(k, lo, hi, acc)
        for i in range(lo, hi + 1):
            if k < 9 and i == k:
                continue
            acc = i64(acc + m[i] * P29[k - i], f"{name} column {k} m[{i}] p[{k - i}]")
        if k < 9:
            m[k] = (as_u32(acc) * PINV29 & 0xFFFFFFFF) & M29
            acc = i64(acc + m[k] * P29[0], f"{name} column {k} m[{k}] p[0]")
        else:
            r[k - 9] = as_u32(acc) & M29
        acc >>= 29
    r[8] = i32(acc, f"{name} top")
    return r


def mul(a, b):
    """f29_mul and f29_mul_leaf: value(a) value(b) / 2^261 mod p"""
    a, b = _vec(a), _vec(b)

    def col(k, lo, hi, acc):
        for i in range(lo, hi + 1):
            acc = i64(acc + a[i] * b[k - i], f"mul column {k} a[{i}] b[{k - i}]")
        return acc
    return _mont_columns(col, "mul")


def dot2(a, b, c, d):
    """f29_dot2: (a b + c d) / 2^261, one column pass"""
    a, b, c, d = _vec(a), _vec(b), _vec(c), _vec(d)

    def col(k, lo, hi, acc):
        for i in range(lo, hi + 1):
            acc = i64(acc + a[i] * b[k - i], f"dot2 column {k} a[{i}] b[{k - i}]")
            acc = i64(acc + c[i] * d[k - i], f"dot2 column {k} c[{i}] d[{k - i}]")
        return acc
    return _mont_columns(col, "dot2")


def dot2_ilp(a, b, c, d):
    """f29_dot2_ilp: the same value as dot2, the column split over two accumulators x, y"""
    a, b, c, d = _vec(a), _vec(b), _vec(c), _vec(d)
    m, r, acc = [0] * 9, [0] * 9, 0
    for k in range(17):
        x, y = acc, 0
        lo, hi = (k - 8 if k > 8 else 0), (k if k < 8 else 8)
        for i in range(lo, hi + 1):
            x = i64(x + a[i] * b[k - i], f"dot2_ilp column {k} x a[{i}] b[{k - i}]")
            y = i64(y + c[i] * d[k - i], f"dot2_ilp column {k} y c[{i}] d[{k - i}]")
        for i in range(lo, hi + 1):
            if k < 9 and i == k:
                continue
            if (i - lo) & 1:
                x = i64(x + m[i] * P29[k - i], f"dot2_ilp column {k} x m[{i}]")
            else:
                y = i64(y + m[i] * P29[k - i], f"dot2_ilp column {k} y m[{i}]")
        acc = i64(x + y, f"dot2_ilp column {k} x + y")
        if k < 9:
            m[k] = (as_u32(acc) * PINV29 & 0xFFFFFFFF) & M29
            acc = i64(acc + m[k] * P29[0], f"dot2_ilp column {k} m[{k}] p[0]")
        else:
            r[k - 9] = as_u32(acc) & M29
        acc >>= 29
    r[8] = i32(acc, "dot2_ilp top")
    return r


def sqr(a):
    """f29_sqr: a^2 / 2^261 with the cross products taken once against the doubled operand"""
    a = _vec(a)
    a2 = [i32(x * 2, f"sqr 2 a[{i}]") for i, x in enumerate(a)]

    def col(k, lo, hi, acc):
        i = lo
        while 2 * i < k:
            acc = i64(acc + a[i] * a2[k - i], f"sqr column {k} a[{i}] 2a[{k - i}]")
            i += 1
        if k % 2 == 0:
            acc = i64(acc + a[k // 2] * a[k // 2], f"sqr column {k} a[{k // 2}]^2")
        return acc
    return _mont_columns(col, "sqr")


# ---- reduce-and-normalise passes ------------------------------------------------------------------------------------------
def quotient(t8):
    """q = round(t8 / (p / 2^232)) as the device estimates it: (t8 K + 2^43) >> 44"""
    return i64(i64(t8 * K, "reduce t8 K") + (1 << 43), "reduce t8 K + 2^43") >> 44


def reduce_from(limbs):
    """f29_reduce_from(limb): `limbs` are the nine i64 values limb(0..8)"""
    limbs = [i64(x, f"reduce_from limb({i})") for i, x in enumerate(limbs)]
    assert len(limbs) == 9
    t8 = limbs[8]
    q = quotient(t8)
    r, acc = [0] * 9, 0
    for i in range(8):
        acc = i64(acc + i64(limbs[i] - i64(q * P29[i], f"reduce_from q p[{i}]"), f"reduce_from limb({i}) - q p[{i}]"),
                  f"reduce_from acc[{i}]")
        r[i] = as_u32(acc) & M29
        acc >>= 29
    r[8] = i32(i64(i64(acc + t8, "reduce_from acc + t8") - i64(q * P29[8], "reduce_from q p[8]"), "reduce_from top"), "reduce_from top")
    return r


def reduce_terms(xs, ks):
    """f29_reduce_terms<N>: reduce(sum_j k_j x_j) as one multiply-add chain"""
    xs, ks = [_vec(x) for x in xs], [i32(k, "coefficient") for k in ks]
    assert len(xs) == len(ks)
    t8 = 0
    for x, k in zip(xs, ks):
        t8 = i64(t8 + x[8] * k, "reduce_terms t8")
    nq = i32(-i32(quotient(t8), "reduce_terms q"), "reduce_terms -q")
    r, acc = [0] * 9, 0
    for i in range(8):
        for j, (x, k) in enumerate(zip(xs, ks)):
            acc = i64(acc + x[i] * k, f"reduce_terms limb {i} term {j}")
        acc = i64(acc + nq * P29[i], f"reduce_terms limb {i} -q p")
        r[i] = as_u32(acc) & M29
        acc >>= 29
    r[8] = i32(i64(i64(acc + t8, "reduce_terms acc + t8") + nq * P29[8], "reduce_terms top"), "reduce_terms top")
    return r


def norm_terms(xs, ks):
    """f29_norm_terms<N>: carry normalisation of sum_j k_j x_j, no multiple of p subtracted"""
    xs, ks = [_vec(x) for x in xs], [i32(k, "coefficient") for k in ks]
    assert len(xs) == len(ks)
    r, acc = [0] * 9, 0
    for i in range(8):
        for j, (x, k) in enumerate(zip(xs, ks)):
            acc = i64(acc + x[i] * k, f"norm_terms limb {i} term {j}")
        r[i] = as_u32(acc) & M29
        acc >>= 29
    for j, (x, k) in enumerate(zip(xs, ks)):
        acc = i64(acc + x[8] * k, f"norm_terms top term {j}")
    r[8] = i32(acc, "norm_terms top")
    return r


def lin2(a, ka, b, kb):
    """f29_lin2 (u2_lin2 / w2_lin2 per coordinate): reduce(ka a + kb b)"""
    return reduce_terms([a, b], [ka, kb])


def xi_lin_limbs(x0, x1, y0, y1, k, m):
    """the two lambdas of u2_xi_lin: limb(i) of k xi x + m y, xi = 9 + u, as i64 values"""
    x0, x1, y0, y1 = _vec(x0), _vec(x1), _vec(y0), _vec(y1)
    c0 = [i64(i64(i64(x0[i] * 9 - x1[i], "xi_lin 9 x0 - x1") * k, "xi_lin (9 x0 - x1) k") + y0[i] * m, "xi_lin c0 limb")
          for i in range(9)]
    c1 = [i64(i64(i64(x0[i] + x1[i] * 9, "xi_lin x0 + 9 x1") * k, "xi_lin (x0 + 9 x1) k") + y1[i] * m, "xi_lin c1 limb")
          for i in range(9)]
    return c0, c1


def u2_xi_lin(x0, x1, y0, y1, k, m):
    """u2_xi_lin: reduce(k xi x + m y) -> (c0, c1)"""
    c0, c1 = xi_lin_limbs(x0, x1, y0, y1, k, m)
    return reduce_from(c0), reduce_from(c1)


# ---- conversions ----------------------------------------------------------------------------------------------------------------
def from_fp(words):
    """f29_from_fp: the digits of (X << 5) for X given as 8 little-endian u32 words"""
    x = [u32(w, "from_fp word") for w in words]
    assert len(x) == 8
    r = [(x[0] << 5) & M29] + [0] * 8
    for i in range(1, 9):
        bit = 29 * i - 5
        w, s = bit >> 5, bit & 31
        lo = x[w] >> s
        hi = ((x[w + 1] << (32 - s)) & 0xFFFFFFFF) if (s != 0 and w + 1 < 8) else 0
        r[i] = (lo | hi) & M29
    return r


RR = [0x059bac10, 0x0d1503a3, 0x018016b8, 0x10ab0ca8, 0x02632639, 0x02c0169f, 0x169bfd53, 0x11869d4c, 0x002a11a6]   # R'^2 mod p


def plain_digits(words):
    """the 29-bit digits f29_from_plain cuts from 8 little-endian u32 words (any 256-bit value: the top digit holds bits 232..255)"""
    x = [u32(w, "from_plain word") for w in words]
    assert len(x) == 8
    d = [x[0] & M29] + [0] * 8
    for i in range(1, 9):
        bit = 29 * i
        w, sh = bit >> 5, bit & 31
        lo = x[w] >> sh
        hi = ((x[w + 1] << (32 - sh)) & 0xFFFFFFFF) if (sh > 3 and w + 1 < 8) else 0
        d[i] = (lo | hi) & M29
    return d


def from_plain(words):
    """f29_from_plain (plk_multi.hip): X's digits times R'^2 mod p in one carry-free product -> X R' mod p, normalized"""
    return mul(plain_digits(words), RR)


def _cond_sub(r, c, o8=0):
    """the borrow chain of the device: r - c over 8 words (then o8 - 0 - borrow when o8 takes part); keep r when it borrows"""
    s, borrow = [], 0
    for i in range(8):
        t = r[i] - c[i] - borrow
        borrow = 1 if t < 0 else 0
        s.append(t & 0xFFFFFFFF)
    return r if borrow else s


def to_fp(a):
    """f29_to_fp -> 8 canonical u32 words of value(a) / 32 mod p (input normalized, value in (-64 p, 64 p))"""
    a = _vec(a)
    low = as_u32(i32(a[0] + K64[0], "to_fp low"))
    mm = (low * PINV29 & 0xFFFFFFFF) & 31
    acc, d = 0, [0] * 9
    for i in range(9):
        acc = i64(acc + a[i] + K64[i] + mm * P29[i], f"to_fp acc[{i}]")
        if i < 8:
            d[i] = as_u32(acc) & M29
            acc >>= 29
        else:
            d[i] = u32(acc, "to_fp top digit")
    o = [0] * 9
    for i in range(9):
        if i == 0:
            o[0] |= d[0] >> 5
            continue
        bit = 29 * i - 5
        w, s = bit >> 5, bit & 31
        o[w] |= (d[i] << s) & 0xFFFFFFFF
        if s > 3 and w + 1 < 9:
            o[w + 1] |= d[i] >> (32 - s)
    full = sum(x << (29 * i) for i, x in enumerate(d))
    if full & 31 or sum(x << (32 * i) for i, x in enumerate(o)) != full >> 5:
        raise Overflow("to_fp: the repacked words lose bits of (a + 64 p + m p) / 32")
    r = o[:8]
    # 4p against the nine words o[0..8]: v_subb into o[8] gives bor = o[8] - borrow; a non-zero bor keeps r
    s4, borrow = [], 0
    for i in range(8):
        t = r[i] - P4[i] - borrow
        borrow = 1 if t < 0 else 0
        s4.append(t & 0xFFFFFFFF)
    bor = (o[8] - borrow) & 0xFFFFFFFF
    r = r if bor != 0 else s4
    r = _cond_sub(r, P2)
    r = _cond_sub(r, P1)
    return r


def words_value(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def int_to_words(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


if __name__ == "__main__":
    print("p limbs   ", [hex(x) for x in P29])
    print("PINV29    ", hex(PINV29), (P * PINV29 + 1) % (1 << 29) == 0)
    print("K         ", K, " 2^276 / p =", (1 << 276) / P)
    print("k64       ", [hex(x) for x in K64])
    print("4p words  ", [hex(x) for x in P4])
    print("2p words  ", [hex(x) for x in P2])
    sys.exit(0)
