"""A CPU model of batched KZG opening verification on BN254 under one SRS.  Not collected by pytest, and it shares nothing with sylow_amd:
instances are made in Fr by a maker who knows tau (every point is a generator multiple whose discrete logarithm the maker knows), the points
and the pairings come from the C oracle (oracle.coracle, through the point helpers of groth16_model), and the expected booleans follow from
the equation alone.

    F = C - y G1gen + z pi            ok = [ e(F, G2gen) e(-pi, tau_g2) == 1 ]

Identities follow pairing() / EIP-197: a pair with an identity on either side contributes 1 (it is left out of the product).  z, y and
weights are any 256-bit integers, taken mod r."""
import copy
import os
import random
import sys
import types

import numpy as np

import groth16_model as G
from groth16_model import C, ONE48, P, R, ints, limbs  # noqa: F401  (re-exported for the tests)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import glv_model  # noqa: E402  (the limb-exact model of glv_decompose: the authority for choosing the crafted z)

DEFECTS = ("y_plus_one", "z_plus_one", "pi_swapped", "c_negated", "c_identity_valid", "pi_identity_valid", "pi_identity_invalid", "f_identity")
# what the boolean of a row carrying the defect must be
DEFECT_VALID = {"y_plus_one": False, "z_plus_one": False, "pi_swapped": False, "c_negated": False, "c_identity_valid": True,
                "pi_identity_valid": True, "pi_identity_invalid": False, "f_identity": False}
GARBAGE = limbs([0xDEADBEEF << 200 | 0x1234567, (1 << 256) - 1]).reshape(8)      # what a flagged point's coordinate words may hold


def inv(v):
    return pow(v % R, R - 2, R)


class Instance:
    """n openings under one SRS.  dlog: the maker's Fr values (tau, c [n], pi [n]); z, y: n Python ints (any 256-bit value); arrays: affine
    words and flags as the engine takes them."""

    def __init__(self, tau, c, z, y, pi=None):
        self.n = len(c)
        self.z, self.y = [int(v) for v in z], [int(v) for v in y]
        pi = [(c[i] - y[i]) * inv(tau - z[i]) % R for i in range(self.n)] if pi is None else pi
        self.dlog = {"tau": tau, "c": [v % R for v in c], "pi": [v % R for v in pi]}
        self.tau_g2 = G.g2_gen_mul([tau])[0]
        self.c_inf, self.pi_inf = np.zeros(self.n, dtype=np.uint8), np.zeros(self.n, dtype=np.uint8)
        self.planted = {}                                    # row -> defect name
        self.remake()

    def remake(self):
        """the point arrays from the discrete logarithms (rows whose logarithm is 0 come back as the identity: flagged by the caller)"""
        self.c = G.g1_gen_mul(self.dlog["c"])[0]
        self.pi = G.g1_gen_mul(self.dlog["pi"])[0]

    def z_words(self):
        return limbs(self.z)

    def y_words(self):
        return limbs(self.y)

    def take(self, idx):
        """the openings idx (a tiling or a selection) under the same SRS"""
        out = copy.copy(self)
        idx = np.asarray(idx, dtype=np.int64)
        out.n = len(idx)
        out.z, out.y = [self.z[i] for i in idx], [self.y[i] for i in idx]
        for k in ("c", "pi", "c_inf", "pi_inf"):
            setattr(out, k, np.ascontiguousarray(getattr(self, k)[idx]))
        out.planted = {j: self.planted[int(i)] for j, i in enumerate(idx) if int(i) in self.planted}
        out.dlog = None
        return out

    def expected(self):
        return np.array([DEFECT_VALID[self.planted[i]] if i in self.planted else True for i in range(self.n)], dtype=bool)


def make_instance(n, seed):
    """n VALID openings: c_i, z_i, y_i at random, the logarithm of pi_i = (c_i - y_i) / (tau - z_i) mod r"""
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)
    return Instance(fr(), [fr() for _ in range(n)], [fr() for _ in range(n)], [fr() for _ in range(n)])


def plant(inst, defects, seed=7):
    """a copy of a VALID instance (made by make_instance) with the defect classes planted: defects = {row: name}.  pi_swapped takes the next
    row's proof (both rows fail).  Flagged points keep garbage in their coordinate words."""
    assert inst.dlog is not None
    out = copy.deepcopy(inst)
    d, rng = out.dlog, random.Random(seed)
    tau = d["tau"]
    for i, name in defects.items():                          # the classes that remake a row's points
        assert name in DEFECTS
        z, y = out.z[i] % R, out.y[i] % R
        if name == "c_identity_valid":                       # C = 0, to be flagged: the proof is remade for it
            d["c"][i], d["pi"][i] = 0, (0 - y) * inv(tau - z) % R
        elif name == "pi_identity_valid":                    # a constant polynomial: C = y G1gen, pi = 0
            d["c"][i], d["pi"][i] = y, 0
        elif name == "f_identity":                           # F = C - y G + z pi = 0 although pi != 0
            p = rng.randrange(1, R)
            d["c"][i], d["pi"][i] = (y - z * p) % R, p
            assert (d["c"][i] - y) % R != (tau - z) * p % R
    out.remake()
    valid_pi = out.pi.copy()
    for i, name in defects.items():
        if name == "y_plus_one":
            out.y[i] += 1
        elif name == "z_plus_one":
            out.z[i] += 1
        elif name == "pi_swapped":
            j = (i + 1) % out.n
            assert j not in defects
            out.pi[i], out.pi[j] = valid_pi[j], valid_pi[i]
        elif name == "c_negated":
            out.c[i, 4:8] = limbs([P - ints(out.c[i, 4:8])[0]])[0]
        elif name == "c_identity_valid":
            out.c_inf[i] = 1
            out.c[i] = GARBAGE
        elif name in ("pi_identity_valid", "pi_identity_invalid"):
            out.pi_inf[i] = 1
            out.pi[i] = GARBAGE
    out.planted = dict(defects)
    out.planted.update({(i + 1) % out.n: "pi_swapped" for i, name in defects.items() if name == "pi_swapped"})
    return out


# ---- the model -------------------------------------------------------------------------------------------------------------------
def g1_gen_rows(n):
    return np.repeat(G.g1_proj(limbs(G.G1_GEN).reshape(1, 8)), n, 0)


def g1_sum(proj):
    """sum of the rows by a tree of oracle additions, one projective row [1, 12]"""
    rows = np.asarray(proj, dtype=np.uint64).reshape(-1, 12)
    if len(rows) == 0:
        return G.g1_proj(np.zeros((1, 8), dtype=np.uint64), [1])
    while len(rows) > 1:
        h = len(rows) // 2
        s = C.g1_add(rows[:h], rows[h:2 * h])
        rows = np.concatenate([s, rows[2 * h:]]) if len(rows) % 2 else s
    return rows.reshape(1, 12)


def model_fold(inst):
    """C - (y mod r) G1gen + (z mod r) pi by oracle scalar multiplications and additions: projective rows [n, 12]"""
    if inst.n == 0:
        return np.zeros((0, 12), dtype=np.uint64)
    yg = G.g1_mul(g1_gen_rows(inst.n), inst.y)
    zp = G.g1_mul(G.g1_proj(inst.pi, inst.pi_inf), inst.z)
    return C.g1_add(C.g1_add(G.g1_proj(inst.c, inst.c_inf), G.g1_neg(yg)), zp)


def row_pairs(inst):
    """per row the pairs of the equation left after identity skipping: lists of (P projective [12], Q projective [24])"""
    f = model_fold(inst)
    f_inf = G.is_identity(f) if inst.n else []
    fxy = C.g1_to_affine(f)[0] if inst.n else None
    npi = G.g1_neg(G.g1_proj(inst.pi))
    gen, tau = G.g2_proj(limbs(G.G2_GEN).reshape(1, 16))[0], G.g2_proj(inst.tau_g2)[0]
    rows = []
    for i in range(inst.n):
        pairs = []
        if not f_inf[i]:
            pairs.append((G.g1_proj(fxy[i:i + 1])[0], gen))
        if not inst.pi_inf[i]:
            pairs.append((npi[i], tau))
        rows.append(pairs)
    return rows


def model_verify(inst):
    gt = G.products(row_pairs(inst))
    return np.array([np.array_equal(g, ONE48) for g in gt], dtype=bool)


def model_weighted(inst, weights):
    """the two literal pairs of the weighted test, by oracle scalar multiplications and additions:
    (sum r_i C_i + sum (r_i z_i) pi_i - (sum r_i y_i) G1gen, G2gen), (-sum r_i pi_i, tau_g2).  -> (P [2, 12], Q [2, 24])"""
    w = [int(v) % R for v in weights]
    assert len(w) == inst.n
    s = sum(r * (y % R) for r, y in zip(w, inst.y)) % R
    pi, c = G.g1_proj(inst.pi, inst.pi_inf), G.g1_proj(inst.c, inst.c_inf)
    rc = g1_sum(G.g1_mul(c, w)) if inst.n else g1_sum([])
    rzp = g1_sum(G.g1_mul(pi, [r * (z % R) % R for r, z in zip(w, inst.z)])) if inst.n else g1_sum([])
    rp = g1_sum(G.g1_mul(pi, w)) if inst.n else g1_sum([])
    sg = G.g1_mul(g1_gen_rows(1), [s])
    p0 = C.g1_add(C.g1_add(rc, rzp), G.g1_neg(sg))
    p = np.concatenate([p0.reshape(1, 12), G.g1_neg(rp).reshape(1, 12)])
    q = np.concatenate([G.g2_proj(limbs(G.G2_GEN).reshape(1, 16)), G.g2_proj(inst.tau_g2)])
    return p, q


def weighted_product(inst, weights):
    """Gt words [48] of the product over the NON-IDENTITY literal pairs"""
    p, q = model_weighted(inst, weights)
    keep = ~G.is_identity(p)
    return G.products([[(p[k], q[k]) for k in range(2) if keep[k]]])[0]


# ---- crafted scalars for the two digit walks of the fold -------------------------------------------------------------------------
# z pi: z mod r splits into two magnitudes (glv_model.decompose_device); each is walked as 33 signed nibbles, digit i = nibble i of
# m + 0x88...8 (33 eights) minus 8.  y G1gen: y mod r as 32 signed bytes with a carry, digit d in [-128, 127], table entry |d| - 1.
GLV_BIAS = int("8" * 33, 16)
GLV_TOP = (1 << 128) - int("8" * 32, 16)                       # 0x77...78: the least magnitude whose window 32 is 1 (all other digits -8)
GLV_SEVENS = int("7" * 32, 16)                                 # every digit 7, window 32 zero


def glv_halves(z):
    """((|k1|, k1 < 0), (|k2|, k2 < 0)) of z mod r, as the device computes them"""
    return glv_model.decompose_device(int(z) % R)


def glv_window_digits(m):
    assert 0 <= m < 1 << 128
    b = m + GLV_BIAS
    return [((b >> (4 * i)) & 15) - 8 for i in range(33)]


def comb_digits(y):
    y, carry, out = int(y) % R, 0, []
    for w in range(32):
        d = ((y >> (8 * w)) & 255) + carry
        carry = int(d >= 128)
        out.append(d - (carry << 8))
    assert carry == 0
    return out


_CRAFTED = []


def crafted_fold_scalars():
    """A fixed list of (tag, value) for z and for y: ns.z, ns.y.  The z are FOUND with the model (seeded searches, a few thousand
    decompositions): a pair of chosen halves t1 + t2 lambda comes back as itself only when z lands where the model's rounding allows it, so
    every candidate is decomposed and kept only if it shows the property of its tag.

    What the model can and cannot reach (tests/test_kzg_model.py asserts the reachable part, and that the searches below found nothing of
    the rest).  With c_i = floor(z g_i / 2^256) both halves are k1 = e1 a1 + e2 a2 and k2 = e1 b1 - e2 a1 with rounding deficits
    e1 in [0, 1.09), e2 in [0, 1) (a1 ~ 2^63, a2 ~ b1 ~ 0x6f4d 2^112; e1 passes 1 because g_1 is cut to 66 bits and z / 2^256 < 0.19), so
      * k1 >= 0 always, k1 = 0 only for z = 0, and k1 < a2 + 1.09 a1 < 0x77...78: window 32 of the k1 half is never 1, the k1 half is never
        negative, and "k1 = 0, k2 != 0" does not exist;
      * k2 is negative only when e1 < 2^-63, and then |k2| < a1 < 2^64: flip2 (n1 != n2) is reachable, but never together with window 32;
      * k2 >= 0x77...78 needs e1 > 1.07: z in the top tenth of [0, r);
      * k2 = 0x77...78 and k2 = 0x77...77 exactly are not reachable (z = t1 + k2 lambda moves by less than 2^127 with t1, and neither lands
        in the top tenth): the list holds the nearest, one nibble above window 15 changed, 31 of 32 digits as asked."""
    if _CRAFTED:
        return _CRAFTED[0]
    import evm_model
    lam, z = glv_model.lam, []
    k2_of = lambda v: glv_halves(v)[1]
    rng = random.Random(0x61D)
    while sum(t == "k2_top" for t, _ in z) < 6:                # window 32 of the k2 half (digit 31 is then -8)
        v = R - 1 - rng.randrange(R >> 4)
        if k2_of(v)[0] >= GLV_TOP:
            z.append(("k2_top", v))
    for tag, half, lo, hi in (("k1_digit31_7", 0, 7 << 124, 1 << 128), ("k2_digit31_7", 1, 7 << 124, GLV_TOP)):
        found = 0
        while found < 2:
            v = R - 1 - rng.randrange(R >> 4)
            if lo <= glv_halves(v)[half][0] < hi:
                z.append((tag, v))
                found += 1

    def nearest(base, sign):                                   # base with ONE nibble (16..30) changed, as the k2 half
        for j in range(16, 31):
            for d in range(1, 16):
                t2 = base + sign * d * 16 ** j
                for t1 in (3 << 124, 0x64 << 120, 1 << 120):
                    v = (t1 + t2 * lam) % R
                    if k2_of(v) == (t2, False):
                        return v
    z.append(("k2_near_all_minus_8", nearest(GLV_TOP, 1)))
    z.append(("k2_near_all_7", nearest(GLV_SEVENS, -1)))
    z += [("k2_zero", v) for v in (1, 0xFFFFFFFFFFFFFFFF, (1 << 125) + 0x123456789ABCDEF)]
    for j in (1, 2, 3, 5, 0xC0FFEE, 0xC0FFEF, (1 << 62) + 12345, (1 << 62) + 12346):      # z g_1 just above j 2^256: e1 ~ 0, k2 < 0
        v = -((-j << 256) // glv_model.g1c)
        if v < R and k2_of(v)[1]:
            z.append(("k2_negative", v))
    z += [("edge", v % R) for v in evm_model.glv_edge_scalars()]
    below = lambda byte, top: top << 248 | int.from_bytes(bytes([byte]) * 31, "big")
    y = [("all_80", below(0x80, 0x2F)), ("all_7f", below(0x7F, 0x2F)), ("all_ff", below(0xFF, 0x2F)), ("all_80_top_0", below(0x80, 0)),
         ("alternating", int("30" + "7f80" * 15 + "80", 16)),     # >= r: the kernel reduces it
         ("alternating_807f", int("2f" + "807f" * 15 + "80", 16)),
         ("alternating_7f80", int("2f" + "7f80" * 15 + "80", 16)), ("r_minus_1", R - 1), ("top_digit_max", 0x30 << 248),
         ("top_digit_max_by_carry", below(0xFF, 0x2F) - 0x7F)]
    _CRAFTED.append(types.SimpleNamespace(z=z, y=y))
    return _CRAFTED[0]


def crafted_instance(seed=0xC4AF):
    """Openings that pair every crafted z with a random y and every crafted y with a random z (the edge scalars once, the others twice), pi
    cycling through random generator multiples, G1gen and -G1gen; the maker knows tau and makes about half of the rows valid openings
    (C = y G1gen + (tau - z) pi), the others carry a random C.  No row is flagged.  -> (Instance, the maker's booleans)"""
    cs, rng = crafted_fold_scalars(), random.Random(seed)
    fr = lambda: rng.randrange(1, R)
    zs, ys = [], []
    for tag, v in cs.z:
        for _ in range(1 if tag == "edge" else 2):
            zs.append(v)
            ys.append(fr())
    for tag, v in cs.y:
        for _ in range(2):
            zs.append(fr())
            ys.append(v)
    tau, n = fr(), len(zs)
    pi = [(fr(), 1, fr(), R - 1)[i % 4] for i in range(n)]
    valid = np.array([(i // 4 + i) % 2 == 0 for i in range(n)], dtype=bool)
    c = [(ys[i] + (tau - zs[i]) * pi[i]) % R if valid[i] else fr() for i in range(n)]
    assert all(v != 0 for v in c)
    return Instance(tau, c, zs, ys, pi), valid


def collapse_weights(idx, weights, pool_n):
    """A batch tiled from a pool (row i is pool row idx[i]) under weights r_i is, for the weighted test, the pool itself under the sums of
    the weights that fall on each pool row: the two literal pairs are linear in r_i with C, z, y and pi fixed per pool row.  -> pool_n ints"""
    out = [0] * pool_n
    for i, w in zip(np.asarray(idx).tolist(), weights):
        out[i] = (out[i] + int(w)) % R
    return out
