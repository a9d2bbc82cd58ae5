"""GPU: the group law on points whose INTERNAL 29-bit digits sit at their bounds, through the public entry points only, bit-exact against
the C oracle (its projective routine, then g?_to_affine).  Every other group test draws random generator multiples, whose internal digits
are uniform; here the points are the crafted ones of tests/helpers.py (low limbs all 2^29 - 1, all zero, alternating, 2^28, under extreme
top limbs), so the first-layer operands x - y, y - z, x - z of proj_add_lazy and the window tables 1P..8P start from extreme digits.
tests/test_group_law_model.py proves on the CPU what these rows reach (they come from one place, tests/group_law_model.py) and replays the
formulas on the limb-exact model.

Three kinds of rows:
  * on-curve crafted points (38 of G1, 27 of the twist, outside the r-torsion), their negatives, identity flags: every entry point;
  * projective words with a crafted Z: normalize, ct_eq, projective_new;
  * OFF-curve affine pairs whose x - y has all eight low limbs at +-(2^29 - 1): the worst column sum of a product leaf.  The formulas are
    polynomial maps, so the oracle's routine on the same words is the expected value -- but only for the entry points that evaluate one
    formula once (add, sub, double, normalize).  Scalar multiplication, sums and MSM use the endomorphism and a fold order of their own,
    which are only valid on the curve."""
import numpy as np
import pytest

import group_law_model as GM
import ntt_model as N
from helpers import P, SEED, Xoshiro, crafted_g2_projective, crafted_values, limbs
from oracle import pyref as PR

pytestmark = pytest.mark.gpu

R = PR.R_ORDER
ROUTES = {"bucket": 0, "small": 1 << 40}
LAMBDA = next(v for v in (pow(g, (R - 1) // 3, R) for g in range(2, 20)) if v != 1)        # a cube root of unity mod r: the GLV eigenvalue or its square
SCALARS = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, R - 1, R, R + 1, P - 1, LAMBDA, 1 << 127, (1 << 128) - 1]
ID12 = limbs([0, 1, 0]).reshape(12)
ID24 = limbs([0, 0, 1, 0, 0, 0]).reshape(24)


class Group:
    """the packing of one group's rows and its oracle routines"""

    def __init__(self, C, name):
        g1 = name == "g1"
        self.name, self.w, self.ident = name, 8 if g1 else 16, ID12 if g1 else ID24
        self.id_xy = limbs([0, 1] if g1 else [0, 0, 1, 0]).reshape(self.w)
        for op in ("add", "sub", "double", "to_affine", "scalar_mul", "ct_eq", "projective_new"):
            setattr(self, op, getattr(C, f"{name}_{op}"))

    def flat(self, pt):
        return list(pt) if self.name == "g1" else [c for coord in pt for c in coord]

    def pack(self, pts):
        return limbs([v for pt in pts for v in self.flat(pt)]).reshape(len(pts), self.w)

    def proj(self, xy, inf=None):
        """affine words (+ flags) -> the oracle's projective rows, Z = 1; a flagged row is the identity"""
        xy = np.asarray(xy, dtype=np.uint64).reshape(-1, self.w)
        z = np.zeros((xy.shape[0], self.w // 2), dtype=np.uint64)
        z[:, 0] = 1
        out = np.concatenate([xy, z], axis=1)
        if inf is not None:
            out[np.asarray(inf).astype(bool)] = self.ident
        return out

    def affine(self, proj):
        """the oracle's affine form with the library's identity: (0, 1) and the flag"""
        xy, inf = self.to_affine(proj)
        xy = xy.copy()
        xy[inf.astype(bool)] = self.id_xy
        return xy, inf

    def fold(self, proj):
        """pairwise fold with the oracle's complete addition -> one projective row"""
        acc = np.asarray(proj, dtype=np.uint64).reshape(-1, 3 * self.w // 2)
        if acc.shape[0] == 0:
            return self.ident.reshape(1, -1).copy()
        while acc.shape[0] > 1:
            h = acc.shape[0] // 2
            acc = np.concatenate([self.add(acc[:h], acc[h:2 * h]), acc[2 * h:]], axis=0)
        return acc

    def lincomb(self, xy, inf, ks):
        """sum_i k_i P_i by the oracle: canonical scalars (Fp::new) into its 256-step routine, then the fold"""
        return self.fold(self.scalar_mul(self.proj(xy, inf), limbs([k % P for k in ks])))


def same(got, exp):
    w = np.asarray(exp[0]).shape[-1]
    return np.array_equal(np.asarray(got[0]).reshape(-1, w), np.asarray(exp[0]).reshape(-1, w)) and \
        np.array_equal(np.asarray(got[1]).reshape(-1), np.asarray(exp[1]).reshape(-1))


def first_difference(got, exp):
    """the first row where (words, flag) differ, for the assertion message"""
    w = np.asarray(exp[0]).shape[-1]
    bad = (np.asarray(got[0]).reshape(-1, w) != np.asarray(exp[0]).reshape(-1, w)).any(axis=1) | \
        (np.asarray(got[1]).reshape(-1) != np.asarray(exp[1]).reshape(-1))
    return int(np.argmax(bad)) if bad.any() else None


@pytest.fixture(scope="module")
def g1(coracle):
    return Group(coracle, "g1")


@pytest.fixture(scope="module")
def g2(coracle):
    return Group(coracle, "g2")


def points_of(name):
    return GM.g1_points() if name == "g1" else GM.g2_points()


def with_negatives(G, name):
    """every crafted point, then every negative: (affine words, all-zero flags)"""
    pts = points_of(name)
    return G.pack(pts + [GM.affine_neg(p) for p in pts])


def rows_of(G, rows):
    a, b = G.pack([r[0] for r in rows]), G.pack([r[1] for r in rows])
    ai, bi = np.array([r[2] for r in rows], dtype=np.uint8), np.array([r[3] for r in rows], dtype=np.uint8)
    return a, b, ai, bi


# ---- one formula, once: add, sub, double -----------------------------------------------------------------------------------------------
def check_add_sub_double(engine, G, rows, on_curve):
    a, b, ai, bi = rows_of(G, rows)
    pa, pb = G.proj(a, ai), G.proj(b, bi)
    eng = {op: getattr(engine, f"{G.name}_{op}") for op in ("add", "sub", "double")}
    for op in ("add", "sub"):
        got, exp = eng[op](a, b, ai, bi), G.affine(getattr(G, op)(pa, pb))
        assert same(got, exp), (G.name, op, first_difference(got, exp))
    got, exp = eng["double"](a, ai), G.affine(G.double(pa))
    assert same(got, exp), (G.name, "double", first_difference(got, exp))
    if on_curve:                                                  # two different polynomial maps: they agree on the curve only
        assert same(got, G.affine(G.add(pa, pa))), (G.name, "double against add(P, P)")


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_add_sub_double_on_crafted_points(engine, g1, g2, name):
    """the cross product P_i o P_j (all of it for G1, a 27 x 8 slice for G2) with P + P, P + (-P), P - P and identity flags on either side"""
    G = g1 if name == "g1" else g2
    rows = GM.add_rows(points_of(name), None if name == "g1" else GM.G2_SLICE)
    check_add_sub_double(engine, G, rows, on_curve=True)
    a, b, ai, bi = rows_of(G, rows)
    n = len(points_of(name))
    cols = list(range(n)) if name == "g1" else list(GM.G2_SLICE)
    _, inf = getattr(engine, f"{name}_add")(a, b, ai, bi)
    assert inf[n * len(cols):n * len(cols) + n].all()             # the block P + (-P)
    _, inf = getattr(engine, f"{name}_sub")(a, b, ai, bi)
    diag = [i * len(cols) + j for i in range(n) for j, c in enumerate(cols) if c == i]
    assert inf[diag].all() and len(diag) == len(cols)             # P - P


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_add_sub_double_off_curve(engine, g1, g2, name):
    """x1 - y1 and x2 - y2 with all eight low limbs at +-(2^29 - 1) (both lanes on the twist): one formula evaluated once, as a polynomial
    map, against the oracle's routine on the same words"""
    check_add_sub_double(engine, g1 if name == "g1" else g2, GM.offcurve_rows(name), on_curve=False)


# ---- scalar multiplication: the window table 1P .. 8P is built from crafted digits ---------------------------------------------------------
def scalar_rows(G, name):
    pts = G.pack(points_of(name))
    xy = np.repeat(pts, len(SCALARS), axis=0)
    ks = SCALARS * pts.shape[0]
    return xy, ks


def test_g1_scalar_mul_both_routes(engine, g1):
    """the eight-lane route (the default for a small batch) and, with SIGN_WIDE_MAX = 0, the one-lane schedule on the same batch: word for
    word equal, and equal to the oracle"""
    from sylow_amd import _lib
    assert "SIGN_WIDE_MAX" in _lib.OPTIONS
    xy, ks = scalar_rows(g1, "g1")
    k = limbs(ks)
    exp = g1.affine(g1.scalar_mul(g1.proj(xy), k))
    assert xy.shape[0] <= engine.get_option("SIGN_WIDE_MAX") or engine.get_option("SIGN_WIDE_MAX") < 0
    wide = engine.g1_scalar_mul(xy, k)
    engine.set_option("SIGN_WIDE_MAX", 0)
    try:
        lane = engine.g1_scalar_mul(xy, k)
    finally:
        engine.set_option("SIGN_WIDE_MAX", -1)
    assert same(wide, lane), first_difference(wide, lane)
    assert same(wide, exp), first_difference(wide, exp)
    zero_rows = [i for i, v in enumerate(ks) if v % R == 0]
    assert wide[1][zero_rows].all() and wide[1].sum() == len(zero_rows)


def test_g2_scalar_mul_generic_route(engine, g2):
    """the crafted twist points are outside the r-torsion (the subgroup check says 2), so only the generic route applies: exact on the whole
    twist, no reduction mod r"""
    xy, ks = scalar_rows(g2, "g2")
    pts = g2.pack(points_of("g2"))
    assert (engine.g2_subgroup_check(pts) == 2).all()
    k = limbs(ks)
    got, exp = engine.g2_scalar_mul(xy, k), g2.affine(g2.scalar_mul(g2.proj(xy), k))
    assert same(got, exp), first_difference(got, exp)
    assert got[1].sum() == sum(v == 0 for v in ks)                # r P is not the identity out there


# ---- many points into one -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_sum_over_crafted_points(engine, g1, g2, name):
    """on the curve the fold order is immaterial: the staged sum against the oracle's pairwise fold; with the negatives the sum is the identity"""
    G = g1 if name == "g1" else g2
    pts = G.pack(points_of(name))
    inf = np.zeros(pts.shape[0], dtype=np.uint8)
    inf[3::7] = 1
    eng_sum = getattr(engine, f"{name}_sum")
    assert same(eng_sum(pts, inf), G.affine(G.fold(G.proj(pts, inf))))
    assert same(eng_sum(pts), G.affine(G.fold(G.proj(pts))))
    both = with_negatives(G, name)
    got = eng_sum(both)
    assert got[1][0] == 1 and same(got, G.affine(G.fold(G.proj(both))))
    got = eng_sum(both[:-1])                                      # all but the last negative: the last point itself
    assert same(got, (pts[-1:], np.zeros(1, dtype=np.uint8)))


def crafted_scalars(rng, n, c):
    pool = [0, 1, (1 << c) - 1, 1 << c, R - 1]
    return [pool[i % len(pool)] if i % 3 else rng.fp() for i in range(n)]


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_lincomb_on_crafted_points(engine, g1, g2, name):
    """5 jobs x 7 terms, term-major: row t * 5 + j is term t of job j"""
    G = g1 if name == "g1" else g2
    nj, nt = 5, 7
    both = with_negatives(G, name)
    xy = both[:nj * nt].copy()
    rng = Xoshiro(SEED + 910)
    ks = crafted_scalars(rng, nj * nt, 4)
    inf = np.zeros(nj * nt, dtype=np.uint8)
    inf[11] = 1
    got = getattr(engine, f"{name}_lincomb")(xy, limbs(ks), nj, nt, inf)
    exp = [G.lincomb(xy[j::nj], inf[j::nj], ks[j::nj]) for j in range(nj)]
    exp = G.affine(np.concatenate(exp, axis=0))
    assert same(got, exp), first_difference(got, exp)


@pytest.mark.parametrize("name", ["g1", "g2"])
@pytest.mark.parametrize("route,window", [("small", -1), ("bucket", 4), ("bucket", 6)])
def test_msm_on_crafted_points(engine, g1, g2, name, route, window):
    """crafted points and their negatives under scalars from {0, 1, 2^c - 1, 2^c, r - 1} and random ones; then EVERY scalar equal, so that
    one bucket per window adds the crafted points to each other as they were loaded, Z = 1"""
    G = g1 if name == "g1" else g2
    xy = with_negatives(G, name)[:-1]                             # without the last negative: the equal-scalar sum is not the identity
    n = xy.shape[0]
    msm = getattr(engine, f"{name}_msm")
    rng = Xoshiro(SEED + 911 + max(window, 0))
    inf = np.zeros(n, dtype=np.uint8)
    inf[5] = 1
    c = max(window, 4)
    for ks, flags in ((crafted_scalars(rng, n, c), inf), ([(1 << c) - 1] * n, None), ([R - 1] * n, None), ([rng.fp()] * n, None)):
        got = msm(xy, limbs(ks), flags, window=window, min_n=ROUTES[route])
        exp = G.affine(G.lincomb(xy, flags, ks))
        assert same(got, exp), (name, route, window, ks[:3])
        assert got[1][0] == 0


def test_g1_ntt_on_crafted_points(engine, g1):
    """out_i = sum_k w^(ik) P_k by the oracle's scalar multiplication and fold, forward and inverse, n = 8 and 32, an identity flag inside"""
    pts = g1.pack(GM.g1_points())
    for log_n in (3, 5):
        n = 1 << log_n
        xy = pts[:n] if log_n == 5 else pts[30:38]
        inf = np.zeros(n, dtype=np.uint8)
        inf[n // 2 + 1] = 1
        for inverse in (False, True):
            w = N.inv(N.omega(log_n)) if inverse else N.omega(log_n)
            scale = N.n_inverse(log_n) if inverse else 1
            rows = [g1.lincomb(xy, inf, [pow(w, i * k, R) * scale % R for k in range(n)]) for i in range(n)]
            exp = g1.affine(np.concatenate(rows, axis=0))
            got = engine.g1_ntt(xy, inf, inverse=inverse)
            assert same(got, exp), (log_n, inverse, first_difference(got, exp))
        back = engine.g1_ntt(*engine.g1_ntt(xy, inf), inverse=True)
        assert np.array_equal(back[1], inf) and np.array_equal(back[0][inf == 0], xy[inf == 0])


def test_kzg_fold_with_crafted_points(engine, g1):
    """F = C - y G1gen + z pi with crafted C and pi"""
    both = with_negatives(g1, "g1")
    n = 38
    c_xy, pi_xy = both[:n], np.roll(both, 9, axis=0)[:n]
    rng = Xoshiro(SEED + 912)
    z, y = crafted_scalars(rng, n, 4), [rng.fp() % R for _ in range(n)]
    y[0], y[1], z[2] = 0, R - 1, LAMBDA
    c_inf, pi_inf = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    c_inf[4], pi_inf[6] = 1, 1
    got = engine.kzg_fold(c_xy, limbs(z), limbs(y), pi_xy, c_inf, pi_inf)
    gen = np.repeat(limbs([1, 2]).reshape(1, 8), n, axis=0)
    yg = g1.scalar_mul(g1.proj(gen), limbs([(R - v) % R for v in y]))
    zp = g1.scalar_mul(g1.proj(pi_xy, pi_inf), limbs([v % R for v in z]))
    exp = g1.affine(g1.add(g1.add(g1.proj(c_xy, c_inf), yg), zp))
    assert same(got, exp), first_difference(got, exp)


def test_groth16_vk_x_with_crafted_bases(engine, g1):
    """vk_x = IC_0 + sum_j x_j IC_j, l = 3, the four bases crafted points"""
    pts = g1.pack(GM.g1_points())
    rng = Xoshiro(SEED + 913)
    small = [0, 1, 15, 16, R - 1, LAMBDA]
    for first in (0, 17, 34):
        ic = pts[first:first + 4]
        inputs = [[small[(i + j) % len(small)] if (i + j) % 2 else rng.fp() % R for j in range(3)] for i in range(24)]
        got = engine.groth16_vk_x(ic, limbs([v for row in inputs for v in row]).reshape(len(inputs), 3, 4))
        rows = [g1.lincomb(ic, None, [1] + row) for row in inputs]
        exp = g1.affine(np.concatenate(rows, axis=0))
        assert same(got, exp), (first, first_difference(got, exp))


# ---- projective words with a crafted Z ----------------------------------------------------------------------------------------------------
def crafted_g1_projective():
    """homogeneous (X, Y, Z) = (x Z, y Z, Z) over the crafted G1 points with a crafted Z: the twin of helpers.crafted_g2_projective"""
    vals = crafted_values()
    out = []
    for k, (x, y) in enumerate(GM.g1_points()):
        z = vals[(5 * k + 1) % len(vals)] or vals[(11 * k + 2) % len(vals)] or 1
        out.append((x * z % P, y * z % P, z))
    return out


def other_z(name):
    """the same points under a second crafted Z"""
    vals = crafted_values()
    if name == "g1":
        zs = [vals[(7 * k + 4) % len(vals)] or 1 for k in range(len(GM.g1_points()))]
        return [(x * z % P, y * z % P, z) for (x, y), z in zip(GM.g1_points(), zs)]
    zs = [(vals[(7 * k + 4) % len(vals)], vals[(3 * k + 1) % len(vals)] or 1) for k in range(len(GM.g2_points()))]
    return [(PR.fp2_mul(x, z), PR.fp2_mul(y, z), z) for (x, y), z in zip(GM.g2_points(), zs)]


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_projective_words_with_a_crafted_z(engine, g1, g2, name):
    G = g1 if name == "g1" else g2
    first = crafted_g1_projective() if name == "g1" else crafted_g2_projective()
    second = other_z(name)
    a, b = limbs([v for t in first for v in G.flat(t)]).reshape(len(first), -1), limbs([v for t in second for v in G.flat(t)]).reshape(len(second), -1)
    assert a.shape == b.shape == (len(points_of(name)), 3 * G.w // 2)
    affine = (G.pack(points_of(name)), np.zeros(a.shape[0], dtype=np.uint8))
    # normalize: back to the crafted affine points, whatever the Z
    normalize = getattr(engine, f"{name}_normalize")
    for words in (a, b):
        got = normalize(words)
        assert same(got, G.affine(words)) and same(got, affine)
    # ct_eq: the same point under two crafted Z; two different points; Z = 0 against Z = 0 (whatever X and Y hold)
    ct_eq = getattr(engine, f"{name}_ct_eq")
    assert np.array_equal(ct_eq(a, b), G.ct_eq(a, b)) and ct_eq(a, b).all()
    shifted = np.roll(b, 1, axis=0)
    assert np.array_equal(ct_eq(a, shifted), G.ct_eq(a, shifted)) and not ct_eq(a, shifted).any()
    za, zb = a.copy(), shifted.copy()
    za[:, G.w:] = 0
    zb[:, G.w:] = 0
    assert np.array_equal(ct_eq(za, zb), G.ct_eq(za, zb)) and ct_eq(za, zb).all()
    assert np.array_equal(ct_eq(za, b), G.ct_eq(za, b)) and not ct_eq(za, b).any()
    # projective_new: on the curve; the twist points are outside the r-torsion (status 2)
    new = getattr(engine, f"{name}_projective_new")
    for words in (a, b, za):
        exp = G.projective_new(words)
        exp = np.where(exp == 3, 1, exp).astype(np.uint8)         # the reference panics there: NOT_ON_CURVE in the library (documented)
        assert np.array_equal(new(words), exp)
    assert (new(a) == (0 if name == "g1" else 2)).all()


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_normalize_off_curve(engine, g1, g2, name):
    """(X, Y, Z) with X - Y at the worst digits and a crafted Z: normalisation is one inversion and two products, valid off the curve"""
    G = g1 if name == "g1" else g2
    vals = crafted_values()
    rows = []
    for k, (a, _, _, _) in enumerate(GM.offcurve_rows(name)):
        z = vals[(5 * k + 1) % len(vals)] or 1
        rows.append((a[0], a[1], z if name == "g1" else (z, vals[(11 * k + 2) % len(vals)])))
    words = limbs([v for t in rows for v in G.flat(t)]).reshape(len(rows), -1)
    got = getattr(engine, f"{name}_normalize")(words)
    assert same(got, G.affine(words)), first_difference(got, G.affine(words))
    assert not got[1].any()
