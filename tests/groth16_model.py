"""A CPU model of batched Groth16 verification on BN254 under one verifying key.  Not collected by pytest, and it shares nothing with
sylow_amd: instances are made in Fr (every point is a generator multiple whose discrete logarithm the maker knows), the points and the
pairings come from the C oracle (oracle.coracle), and the expected booleans follow from the equation alone.

    vk_x = IC_0 + sum_j x_j IC_j          ok = [ e(-A, B) e(alpha, beta) e(vk_x, gamma) e(C, delta) == 1 ]

Identities follow EIP-197: a pair with an identity on either side contributes 1 (it is left out of the product)."""
import copy
import random

import numpy as np

from oracle import coracle as C

P = C.P_INT
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
G1_GEN = (1, 2)
G2_GEN = (0x1800DEEF121F1E76426A00665E5C4479674322D4F75EDADD46DEBD5CD992F6ED, 0x198E9393920D483A7260BFB731FB5D25F1AA493335A9E71297E485B7AEF312C2,
          0x12C85EA5DB8C6DEB4AAB71808DCB408FE3D1E7690C43D37B4CE6CC0166FA7DAA, 0x090689D0585FF075EC9E99AD690C3395BC4B313370B38EF355ACDADCD122975B)
ONE48 = np.zeros(48, dtype=np.uint64)
ONE48[0] = 1

DEFECTS = ("c_swapped", "input_plus_one", "a_negated", "b_swapped", "a_identity", "a_c_identity_valid", "vk_x_identity")
# what the boolean of a row carrying the defect must be
DEFECT_VALID = {"c_swapped": False, "input_plus_one": False, "a_negated": False, "b_swapped": False, "a_identity": False,
                "a_c_identity_valid": True, "vk_x_identity": True}


def limbs(vals):
    return C.to_limbs([int(v) for v in vals])


def ints(a):
    return C.from_limbs(a)


# ---- points from the oracle ------------------------------------------------------------------------------------------------------
def g1_proj(xy, inf=None):
    """affine words [n, 8] (+ flags) -> the oracle's projective [n, 12]; a flagged row is (0, 1, 0)"""
    xy = np.asarray(xy, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros((xy.shape[0], 12), dtype=np.uint64)
    out[:, :8] = xy
    out[:, 8] = 1
    if inf is not None:
        z = np.asarray(inf).astype(bool)
        out[z] = 0
        out[z, 4] = 1
    return out


def g2_proj(xy):
    xy = np.asarray(xy, dtype=np.uint64).reshape(-1, 16)
    out = np.zeros((xy.shape[0], 24), dtype=np.uint64)
    out[:, :16] = xy
    out[:, 16] = 1
    return out


def g1_gen_mul(ks):
    """k_i G1 for Fr values k_i: affine words [n, 8], flags [n]"""
    gen = np.repeat(g1_proj(limbs(G1_GEN).reshape(1, 8)), len(ks), 0)
    return C.g1_to_affine(C.g1_scalar_mul(gen, limbs([k % R for k in ks])))


def g2_gen_mul(ks):
    gen = np.repeat(g2_proj(limbs(G2_GEN).reshape(1, 16)), len(ks), 0)
    return C.g2_to_affine(C.g2_scalar_mul(gen, limbs([k % R for k in ks])))


def g1_mul(proj, ks):
    """(k_i mod r) P_i on projective rows"""
    return C.g1_scalar_mul(proj, limbs([k % R for k in ks]))


def g1_neg(proj):
    out = np.array(proj, dtype=np.uint64).reshape(-1, 12).copy()
    y = ints(out[:, 4:8])
    out[:, 4:8] = limbs([(P - v) % P for v in y])
    return out


def g1_fold(proj):
    """sum of the rows, one projective row"""
    acc = g1_proj(np.zeros((1, 8), dtype=np.uint64), [1])
    for row in np.asarray(proj).reshape(-1, 12):
        acc = C.g1_add(acc, row.reshape(1, 12))
    return acc


def is_identity(proj):
    return C.g1_to_affine(proj)[1].astype(bool)


# ---- instances -------------------------------------------------------------------------------------------------------------------
class Instance:
    """n proofs with l inputs under one key.  dlog: the maker's Fr values (alpha, beta, gamma, delta, ic [l + 1], a [n], b [n]);
    inputs: n rows of l Python ints (any 256-bit value); arrays: affine words and flags as the engine takes them."""

    def __init__(self, dlog, inputs):
        self.dlog, self.inputs = dlog, [list(map(int, row)) for row in inputs]
        self.n, self.l = len(self.inputs), len(dlog["ic"]) - 1
        d = dlog
        self.alpha = g1_gen_mul([d["alpha"]])[0]
        self.beta, self.gamma, self.delta = (g2_gen_mul([d[k]])[0] for k in ("beta", "gamma", "delta"))
        self.ic = g1_gen_mul(d["ic"])[0]
        self.a, _ = g1_gen_mul(d["a"])
        self.b, _ = g2_gen_mul(d["b"])
        self.c, _ = g1_gen_mul(self.c_dlogs())
        self.a_inf, self.b_inf, self.c_inf = (np.zeros(self.n, dtype=np.uint8) for _ in range(3))
        self.planted = {}                                   # row -> defect name

    def vk_x_dlog(self, i):
        d = self.dlog
        return (d["ic"][0] + sum(x * w for x, w in zip(self.inputs[i], d["ic"][1:]))) % R

    def c_dlogs(self):
        d = self.dlog
        inv_delta = pow(d["delta"], R - 2, R)
        return [(d["a"][i] * d["b"][i] - d["alpha"] * d["beta"] - self.vk_x_dlog(i) * d["gamma"]) * inv_delta % R for i in range(self.n)]

    def vk(self):
        return self.alpha, self.beta, self.gamma, self.delta, self.ic

    def input_words(self):
        """[n, l, 4] uint64"""
        return limbs([x for row in self.inputs for x in row]).reshape(self.n, self.l, 4)

    def take(self, idx):
        """the proofs idx (a tiling or a selection) under the same key"""
        out = copy.copy(self)
        idx = np.asarray(idx)
        out.n = len(idx)
        out.inputs = [list(self.inputs[i]) for i in idx]
        for k in ("a", "b", "c", "a_inf", "b_inf", "c_inf"):
            setattr(out, k, np.ascontiguousarray(getattr(self, k)[idx]))
        out.planted = {j: self.planted[int(i)] for j, i in enumerate(idx) if int(i) in self.planted}
        out.dlog = None
        return out

    def expected(self):
        return np.array([DEFECT_VALID[self.planted[i]] if i in self.planted else True for i in range(self.n)], dtype=bool)


def make_instance(n, l, seed):
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)
    dlog = {"alpha": fr(), "beta": fr(), "gamma": fr(), "delta": fr(), "ic": [fr() for _ in range(l + 1)],
            "a": [fr() for _ in range(n)], "b": [fr() for _ in range(n)]}
    return Instance(dlog, [[fr() for _ in range(l)] for _ in range(n)])


def plant(inst, defects):
    """a copy of a VALID instance (made by make_instance, l >= 1) with the defect classes planted: defects = {row: name}.  The rows of
    the two classes that change an input are remade as valid proofs first; c_swapped / b_swapped take the next row's point."""
    assert inst.dlog is not None and inst.l >= 1
    out = copy.deepcopy(inst)
    d = out.dlog
    inv = lambda v: pow(v % R, R - 2, R)
    for i, name in defects.items():                         # the classes that pick the row's input: the proof is remade for it
        if name in ("a_c_identity_valid", "vk_x_identity"):
            rest = (d["ic"][0] + sum(x * w for x, w in zip(out.inputs[i][1:], d["ic"][2:]))) % R
            target = 0 if name == "vk_x_identity" else (-d["alpha"] * d["beta"] * inv(d["gamma"])) % R
            out.inputs[i][0] = (target - rest) * inv(d["ic"][1]) % R
            assert out.vk_x_dlog(i) == target
    out.c, _ = g1_gen_mul(out.c_dlogs())
    valid_c, valid_b = out.c.copy(), out.b.copy()
    for i, name in defects.items():
        assert name in DEFECTS
        if name == "c_swapped":
            out.c[i] = valid_c[(i + 1) % out.n]
        elif name == "input_plus_one":
            out.inputs[i][0] += 1
        elif name == "a_negated":
            out.a[i, 4:8] = limbs([P - ints(out.a[i, 4:8])[0]])[0]
        elif name == "b_swapped":                           # both rows of the swap fail
            j = (i + 1) % out.n
            assert j not in defects
            out.b[i], out.b[j] = valid_b[j], valid_b[i]
        elif name == "a_identity":
            out.a_inf[i] = 1
        elif name == "a_c_identity_valid":
            out.a_inf[i] = 1
            out.c_inf[i] = 1
    out.planted = dict(defects)
    out.planted.update({(i + 1) % out.n: "b_swapped" for i, name in defects.items() if name == "b_swapped"})
    return out


# ---- the model -------------------------------------------------------------------------------------------------------------------
def model_vk_x(inst):
    """IC_0 + sum_j (x_ij mod r) IC_j by oracle scalar multiplications and additions: projective rows [n, 12]"""
    ic = g1_proj(inst.ic)
    acc = np.repeat(ic[:1], inst.n, 0)
    for j in range(inst.l):
        acc = C.g1_add(acc, g1_mul(np.repeat(ic[j + 1:j + 2], inst.n, 0), [row[j] for row in inst.inputs]))
    return acc


def row_pairs(inst, vk_x=None):
    """per row the pairs of the equation left after EIP-197 skipping: lists of (P projective [12], Q projective [24])"""
    vk_x = model_vk_x(inst) if vk_x is None else vk_x
    vk_x_inf = is_identity(vk_x) if inst.n else []
    vxy, _ = C.g1_to_affine(vk_x) if inst.n else (None, None)
    na = g1_neg(g1_proj(inst.a))
    alpha, c = g1_proj(inst.alpha)[0], g1_proj(inst.c)
    beta, gamma, delta, b = g2_proj(inst.beta)[0], g2_proj(inst.gamma)[0], g2_proj(inst.delta)[0], g2_proj(inst.b)
    rows = []
    for i in range(inst.n):
        pairs = []
        if not inst.a_inf[i] and not inst.b_inf[i]:
            pairs.append((na[i], b[i]))
        pairs.append((alpha, beta))
        if not vk_x_inf[i]:
            pairs.append((g1_proj(vxy[i:i + 1])[0], gamma))
        if not inst.c_inf[i]:
            pairs.append((c[i], delta))
        rows.append(pairs)
    return rows


def products(jobs):
    """the Gt words of the product of every job's pairs ([n_jobs, 48]; an empty job is one): ONE call of the oracle's glued_pairing"""
    flat = [pq for j in jobs for pq in j]
    out = np.repeat(ONE48[None], len(jobs), 0)
    if not flat:
        return out
    live = [k for k, j in enumerate(jobs) if j]
    p = np.array([pq[0] for pq in flat], dtype=np.uint64)
    q = np.array([pq[1] for pq in flat], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum([len(jobs[k]) for k in live])]).astype(np.uint64)
    out[live] = C.glued_pairing(p, q, off)
    return out


def model_verify(inst):
    gt = products(row_pairs(inst))
    return np.array([np.array_equal(g, ONE48) for g in gt], dtype=bool)


def model_weighted(inst, weights):
    """the n + 3 literal pairs of the weighted test, by oracle scalar multiplications and additions:
    (r_i A_i, B_i), (-s alpha, beta), (-sum_i r_i vk_x_i, gamma), (-sum_i r_i C_i, delta).  -> (P [n + 3, 12], Q [n + 3, 24])"""
    w = [int(v) % R for v in weights]
    s = sum(w) % R
    ra = g1_mul(g1_proj(inst.a, inst.a_inf), w)
    rx = g1_fold(g1_mul(model_vk_x(inst), w)) if inst.n else g1_fold(np.zeros((0, 12)))
    rc = g1_fold(g1_mul(g1_proj(inst.c, inst.c_inf), w)) if inst.n else g1_fold(np.zeros((0, 12)))
    sa = g1_mul(g1_proj(inst.alpha), [s])
    p = np.concatenate([ra.reshape(-1, 12), g1_neg(sa), g1_neg(rx), g1_neg(rc)])
    q = np.concatenate([g2_proj(inst.b).reshape(-1, 24), g2_proj(inst.beta), g2_proj(inst.gamma), g2_proj(inst.delta)])
    return p, q


def weighted_product(inst, weights):
    """(Gt words [48] of the product over the NON-IDENTITY literal pairs, whether every literal pair was kept)"""
    p, q = model_weighted(inst, weights)
    keep = ~is_identity(p)
    keep[:inst.n] &= ~np.asarray(inst.b_inf[:inst.n]).astype(bool)
    gt = products([[(p[k], q[k]) for k in range(len(p)) if keep[k]]])[0]
    return gt, bool(keep.all())
