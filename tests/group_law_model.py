"""Limb-exact replay of the lazy group law (proj_add_lazy / proj_double_lazy, sylow_amd/csrc/bn254_pairing.hpp) on the host model of the
carry-free core (tools/f29_model.py), one class per device policy:

    OpsF29    G1 on the carry-free core (bn254_pairing.hpp); OpsF29I differs only in inlining, the same digits
    OpsW2     G2 on lane pairs, the twist E' (plk_group.hip): a coordinate is the pair (even lane's digits, odd lane's digits)
    OpsW2I    G2 on the isomorphic twist E'': y^2 = x^3 + (9 - u)

The two formulas are written once over the policy, line for line as the device's template; every limb-wise step goes through the model's
i32 check and every leaf through the model's i64 checks, so a schedule that would wrap on the device raises f29_model.Overflow here.
A point is a triple of coordinates in the core's Montgomery form (value 2^261 mod p); `from_model` takes a triple back to canonical integers.

`MUTATIONS` names three deliberate departures from the device's schedule for tests/test_group_law_model.py; no policy uses one by default."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import f29_model as M  # noqa: E402

P = M.P
RP_INV = pow(M.RP, P - 2, P)
ONE = [0x157ccc21, 0x141c2758, 0x185230d3, 0x014c0419, 0x0aa36fb9, 0x1d4240ce, 0x11d54c07, 0x052ac7a8, 0x000dc836]   # OpsF29::one()
ZERO = [0] * 9
# OpsW2::mul_b3: 3 b' 2^261 mod p as balanced lane-pair digits (k0: even lane, k1: odd lane)
B3_K0 = [0x10dfc87a, 0x0066b592, 0x16ad88c7, 0x02c15844, 0x158f2f8c, 0x09ad0e4d, 0x137cf714, 0x14872cdb, -1389659]
B3_K1 = [0x01e5cc12, 0x15bda508, 0x18588eb7, 0x00f3e938, 0x18f2b0b4, 0x03bffebe, 0x13752c37, 0x0ec49a37, 0x0017dd10]

MUTATIONS = ("norm_x8_negative_limb", "skip_norm_3t0", "skip_w2_norm_b3")


def internal_digits(x):
    """the nine limbs the device holds for the canonical x: reduce(from_fp(x 2^256 mod p)), as w2_from_s2 / f29_from_fp_reduced"""
    words = M.int_to_words(x * (1 << 256) % P)
    return M.reduce_terms([M.from_fp(words)], [1])


def _ladd(a, b):
    return [M.i32(x + y, f"ladd limb {i}") for i, (x, y) in enumerate(zip(M._vec(a), M._vec(b)))]


def _lsub(a, b):
    return [M.i32(x - y, f"lsub limb {i}") for i, (x, y) in enumerate(zip(M._vec(a), M._vec(b)))]


def _lneg(a):
    return [M.i32(-x, f"neg limb {i}") for i, x in enumerate(M._vec(a))]


class OpsF29:
    """one F29 per coordinate"""
    name = "OpsF29"
    bound = 2.1                                   # the |V| the comment above OpsF29 states for the outputs
    mutation = None

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.mutation = mutation

    def mul(self, a, b): return M.mul(a, b)
    def sqr(self, a): return M.sqr(a)
    def zero(self): return list(ZERO)
    def one(self): return list(ONE)
    def is_zero(self, a): return M.value(a) % P == 0                      # fp_is_zero(f29_to_fp(a))
    def select(self, a, b, c): return list(b) if c else list(a)
    def mul_b3(self, a): return M.reduce_from([M.i64(x * 9, "mul_b3 9 limb") for x in M._vec(a)])
    def ladd(self, a, b): return _ladd(a, b)
    def lsub(self, a, b): return _lsub(a, b)
    def neg(self, a): return M.norm(_lneg(a))
    def norm(self, a): return M.norm(a)
    def norm_x8(self, a): return M.norm_x8(a)
    def norm_sub3(self, a, b): return M.norm_sub3(a, b)
    def mul_b3_lazy(self, a): return self.mul_b3(a)

    # how the tests look at a coordinate
    def parts(self, a): return [a]
    def from_ints(self, x): return internal_digits(x)
    def to_int(self, a): return M.value(a) * RP_INV % P
    def coord(self, parts): return list(parts[0])


class OpsW2(OpsF29):
    """a coordinate is (c0, c1): what the even and the odd lane of the pair hold"""
    name = "OpsW2"
    bound = 2.3

    @staticmethod
    def _mul_ilp(a, b):
        # w2_exchange + f29_dot2_ilp(a, U, W, b): even lane X U + W V = a0 b0 + a1 (-b1), odd lane a1 b0 + a0 b1
        (a0, a1), (b0, b1) = a, b
        return (M.dot2_ilp(a0, b0, a1, _lneg(b1)), M.dot2_ilp(a1, b0, a0, b1))

    def mul(self, a, b): return self._mul_ilp(a, b)

    def sqr(self, a):
        # w2_sqr_leaf: even lane (a0 + a1)(a0 - a1), odd lane a0 * 2 a1 (f29_mul of sel9(odd, a + o, o), sel9(odd, a - o, 2 a))
        a0, a1 = a
        return (M.mul(_ladd(a0, a1), _lsub(a0, a1)), M.mul(a0, _ladd(a1, a1)))

    def zero(self): return (list(ZERO), list(ZERO))
    def one(self): return (list(ONE), list(ZERO))
    def is_zero(self, a): return M.value(a[0]) % P == 0 and M.value(a[1]) % P == 0
    def select(self, a, b, c): return (list(b[0]), list(b[1])) if c else (list(a[0]), list(a[1]))
    def mul_b3(self, a): return self._mul_ilp(a, (B3_K0, B3_K1))
    def ladd(self, a, b): return (_ladd(a[0], b[0]), _ladd(a[1], b[1]))
    def lsub(self, a, b): return (_lsub(a[0], b[0]), _lsub(a[1], b[1]))
    def neg(self, a): return (M.norm(_lneg(a[0])), M.norm(_lneg(a[1])))
    def norm(self, a): return (M.norm(a[0]), M.norm(a[1]))
    def norm_x8(self, a): return (M.norm_x8(a[0]), M.norm_x8(a[1]))
    def norm_sub3(self, a, b): return (M.norm_sub3(a[0], b[0]), M.norm_sub3(a[1], b[1]))

    def mul_b3_lazy(self, a):
        return self.mul_b3(a if self.mutation == "skip_w2_norm_b3" else self.norm(a))

    def parts(self, a): return [a[0], a[1]]
    def from_ints(self, x): return (internal_digits(x[0]), internal_digits(x[1]))
    def to_int(self, a): return (M.value(a[0]) * RP_INV % P, M.value(a[1]) * RP_INV % P)
    def coord(self, parts): return (list(parts[0]), list(parts[1]))


class OpsW2I(OpsW2):
    name = "OpsW2I"

    def mul_b3(self, a):
        # w2_mul_27m3u: reduce_terms over (own, partner) with (27, 3) on the even lane and (27, -3) on the odd lane
        a0, a1 = a
        return (M.reduce_terms([a0, a1], [27, 3]), M.reduce_terms([a1, a0], [27, -3]))

    def mul_b3_lazy(self, a): return self.mul_b3(a)


def proj_zero(O):
    return (O.zero(), O.one(), O.zero())


def proj_neg(O, p):
    return (p[0], O.neg(p[1]), p[2])


def proj_double_lazy(O, p):
    px, py, pz = p
    t0 = O.sqr(py)
    if O.mutation == "norm_x8_negative_limb":
        # the same value as a D-class vector: norm(2 t0) - t0 limb by limb (negative wherever norm(2 t0) carried out of the limb)
        z3 = O.norm_x8(O.lsub(O.norm(O.ladd(t0, t0)), t0))
    else:
        z3 = O.norm_x8(t0)
    t1 = O.mul(py, pz)
    t2 = O.mul_b3(O.sqr(pz))
    x3 = O.mul(t2, z3)
    y3 = O.norm(O.ladd(t0, t2))
    z3 = O.mul(t1, z3)
    t0 = O.norm_sub3(t0, t2)
    y3 = O.mul(t0, y3)
    y3 = O.norm(O.ladd(x3, y3))
    t1 = O.mul(px, py)
    x3 = O.mul(t0, t1)
    x3 = O.norm(O.ladd(x3, x3))
    z = O.is_zero(pz)
    return (O.select(x3, O.zero(), z), O.select(y3, O.one(), z), O.select(z3, O.zero(), z))


def first_layer_operands(O, p, q):
    """the six difference operands of an addition, in the order they are formed: x1 - y1, x2 - y2, y1 - z1, y2 - z2, x1 - z1, x2 - z2"""
    (px, py, pz), (qx, qy, qz) = p, q
    return [O.lsub(px, py), O.lsub(qx, qy), O.lsub(py, pz), O.lsub(qy, qz), O.lsub(px, pz), O.lsub(qx, qz)]


def proj_add_lazy(O, p, q):
    (px, py, pz), (qx, qy, qz) = p, q
    d = first_layer_operands(O, p, q)
    t0 = O.mul(px, qx)
    t1 = O.mul(py, qy)
    t2 = O.mul(pz, qz)
    t3 = O.norm(O.lsub(O.ladd(t0, t1), O.mul(d[0], d[1])))
    t4 = O.norm(O.lsub(O.ladd(t1, t2), O.mul(d[2], d[3])))
    y3 = O.lsub(O.ladd(t0, t2), O.mul(d[4], d[5]))
    t0 = O.ladd(O.ladd(t0, t0), t0)
    if O.mutation != "skip_norm_3t0":
        t0 = O.norm(t0)
    t2 = O.mul_b3(t2)
    z3 = O.norm(O.ladd(t1, t2))
    t1 = O.lsub(t1, t2)
    y3 = O.mul_b3_lazy(y3)
    x3 = O.norm(O.lsub(O.mul(t3, t1), O.mul(t4, y3)))
    y3 = O.norm(O.ladd(O.mul(t1, z3), O.mul(y3, t0)))
    z3 = O.norm(O.ladd(O.mul(z3, t4), O.mul(t0, t3)))
    return (x3, y3, z3)


def from_model(O, p):
    """canonical integers (Fp, or Fp2 pairs) of a model point"""
    return tuple(O.to_int(c) for c in p)


def to_model(O, p):
    """the digits the device holds after loading the canonical triple p"""
    return tuple(O.from_ints(c) for c in p)


def max_v(O, p):
    return max(M.V(v) for c in p for v in O.parts(c))


def n_class(O, p):
    return all(0 <= x <= M.M29 for c in p for v in O.parts(c) for x in v[:8])


# ---- the planted rows of tests/test_gpu_group_law_bounds.py, built here so that tests/test_group_law_model.py can prove on the CPU what they reach ----
def load_affine(O, pt, inf=False):
    """the digits load_g1w_flagged / load_g2q hand to the formulas for an affine point and its identity flag: Z is the policy's stored one"""
    if inf:
        return proj_zero(O)
    return (O.from_ints(pt[0]), O.from_ints(pt[1]), O.one())


def _neg(v):
    return (P - v) % P if isinstance(v, int) else tuple((P - c) % P for c in v)


def affine_neg(pt):
    return (pt[0], _neg(pt[1]))


def g1_points():
    """the 38 crafted points of y^2 = x^3 + 3 (helpers.crafted_g1_points): (x, y)"""
    from helpers import crafted_g1_points
    return crafted_g1_points()


def g2_points():
    """the 27 crafted points of the twist, outside the r-torsion (helpers.crafted_g2_points): ((x0, x1), (y0, y1))"""
    from helpers import crafted_g2_points
    return crafted_g2_points()


G2_SLICE = (0, 1, 2, 3, 5, 8, 13, 21)            # the columns of the 27 x 8 slice, spread over the set: eight rows of it are P + P


def add_rows(pts, cols=None):
    """rows (a, b, a_inf, b_inf) of the addition / subtraction tests over on-curve points: the cross product P_i o P_j (j over `cols`, or
    every j), which holds P o P; then P o (-P) and (-P) o P_(i+1) for every i; then identity flags on the left, the right and both sides"""
    n = len(pts)
    cols = range(n) if cols is None else cols
    rows = [(pts[i], pts[j], 0, 0) for i in range(n) for j in cols]
    rows += [(pts[i], affine_neg(pts[i]), 0, 0) for i in range(n)]
    rows += [(affine_neg(pts[i]), pts[(i + 1) % n], 0, 0) for i in range(n)]
    for i in range(0, n, 5):
        rows += [(pts[i], pts[(i + 2) % n], 1, 0), (pts[i], pts[(i + 2) % n], 0, 1), (pts[i], pts[(i + 2) % n], 1, 1)]
    return rows


def qualifying_pairs():
    """ordered pairs (a, b) of crafted values whose internal digits differ by at least 2^29 - 2 in every one of the eight low limbs: as x and
    y of one point they make x - y the worst operand a product leaf can meet.  No such pair is a point of either curve"""
    from helpers import crafted_values
    vals = crafted_values()
    dig = {v: internal_digits(v) for v in vals}
    return [(a, b) for a in vals for b in vals if all(abs(u - v) >= M.M29 - 1 for u, v in zip(dig[a][:8], dig[b][:8]))]


def offcurve_rows(group, count=96):
    """rows (a, b, 0, 0) of affine pairs that are NOT on the curve: both x - y operands of the addition have all eight low limbs (of both
    lanes for G2) at magnitude >= 2^29 - 2.  Legal only where one formula is evaluated once (add, sub, double, normalize)"""
    pairs = qualifying_pairs()
    m = len(pairs)
    rows = []
    for i in range(count):
        if group == "g1":
            (x1, y1), (x2, y2) = pairs[(7 * i) % m], pairs[(13 * i + 17) % m]
        else:
            a0, a1, b0, b1 = pairs[(7 * i) % m], pairs[(11 * i + 5) % m], pairs[(13 * i + 17) % m], pairs[(17 * i + 29) % m]
            (x1, y1), (x2, y2) = ((a0[0], a1[0]), (a0[1], a1[1])), ((b0[0], b1[0]), (b0[1], b1[1]))
        rows.append(((x1, y1), (x2, y2), 0, 0))
    return rows
