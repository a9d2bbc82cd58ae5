"""The carry-free Fp12 / Miller-loop tower on every compiled layout, one routine at a time, on random rows and on rows whose internal
29-bit digits are extreme (helpers.crafted_values / crafted_fp12_rows).  Layouts (sylow_hip_fp12_hook_batch, op = base + offset):
  16  lane pair (one pair of lanes per element: k_pairing's layout)
  32  lane quad (plk_quad.hip: leaf pairs split over two lane pairs and exchanged by DPP)
  48  one wavefront per element (EPW = 1, the *_wide routines)
  64  one wavefront per two elements (EPW = 2)
Every result equals the oracle, and the lane-pair layout's -- the layouts claim the same digits, and results leave canonical.  Then the
public entry points (miller_loop_batch, final_exp_batch, pairing_batch, the one-pair and multi-pair products) on every route, forced in
process, on crafted points and crafted Fp12 rows."""
import numpy as np
import pytest

from helpers import P, SEED, Xoshiro, crafted_fp12_rows, crafted_g1_points, crafted_g2_points, crafted_g2_projective, crafted_values
from oracle import pyref as R
from test_gpu_lane_pair_tower import unit_lines
from test_gpu_multi_pairing import G2

pytestmark = pytest.mark.gpu
LP, QUAD, WIDE1, WIDE2 = 16, 32, 48, 64
OFF = {"mul": 0, "sqr": 1, "sparse": 2, "cycsqr": 3, "frob1": 4, "frob2": 5, "frob3": 6, "expz": 7, "final_exp": 8, "inv": 10, "conj": 12,
       "sparse_unit": 13, "dbl": 14, "add": 15}
OPS = {QUAD: ["mul", "sqr", "sparse", "cycsqr", "frob1", "frob2", "frob3", "sparse_unit"],
       WIDE1: ["mul", "sqr", "sparse", "cycsqr", "frob1", "frob2", "frob3", "inv"]}
OPS[WIDE2] = OPS[WIDE1]
LAYOUTS = [QUAD, WIDE1, WIDE2]
NAME = {LP: "lane_pair", QUAD: "quad", WIDE1: "wide1", WIDE2: "wide2"}


def rows(coracle, vals):
    return coracle.to_limbs([v for r in vals for v in r]).reshape(len(vals), 48)


def fp12_inputs(coracle, seed, n_random):
    """random rows, then every crafted shape, then rows of random picks from the crafted values; b: the same kinds, shifted"""
    rng = Xoshiro(seed)
    vals = crafted_values()
    pick = lambda: vals[rng.next() % len(vals)]
    shapes = crafted_fp12_rows()
    a = [[rng.fp() for _ in range(12)] for _ in range(n_random)] + shapes + [[pick() for _ in range(12)] for _ in range(24)]
    b = [[pick() for _ in range(12)] for _ in range(n_random)] + shapes[3:] + shapes[:3] + [[rng.fp() for _ in range(12)] for _ in range(24)]
    return rows(coracle, a), rows(coracle, b)


def expected(coracle, name, a, b):
    if name == "mul":
        return coracle.fp12_op("mul", a, b)
    if name in ("sqr", "inv"):
        return coracle.fp12_op(name, a)
    if name == "cycsqr":
        return coracle.fp12_op("cyclotomic_squared", a)
    if name.startswith("frob"):
        return coracle.fp12_op("frobenius", a, arg=int(name[-1]))
    if name == "sparse":
        return coracle.fp12_sparse_mul(a, b[:, :24])
    if name == "sparse_unit":
        return coracle.fp12_sparse_mul(a, unit_lines(coracle, b))
    raise KeyError(name)


def hook(engine, base, name, a, b=None):
    return engine.fp12_hook(base + OFF[name], a, b)


@pytest.mark.parametrize("base", LAYOUTS, ids=[NAME[x] for x in LAYOUTS])
def test_layout_ops_match_oracle_and_lane_pair(engine, coracle, base):
    a, b = fp12_inputs(coracle, SEED + 700 + base, 37)          # 37 + 33 + 24 = 94 rows: odd
    for name in OPS[base]:
        got = hook(engine, base, name, a, b)
        assert np.array_equal(got, expected(coracle, name, a, b)), (NAME[base], name)
        if name != "inv":                                         # the lane-pair layer's inverse is the saturated one (op 26)
            assert np.array_equal(got, hook(engine, LP, name, a, b)), (NAME[base], name)
    if base != QUAD:
        # the line kind is the product by (l0, 0, l2; 0, l4, 0), the same element as the dense form
        line = np.zeros_like(b)
        line[:, 0:8], line[:, 16:24], line[:, 32:40] = b[:, 0:8], b[:, 16:24], b[:, 8:16]
        assert np.array_equal(hook(engine, base, "sparse", a, b), hook(engine, base, "mul", a, line))
        assert np.array_equal(hook(engine, base, "inv", a), engine.fp12_hook(26, a))
        # x * inv(x) = 1 for every non-zero row; inv(0) = 0 as the reference has it
        prod = coracle.fp12_op("mul", a, hook(engine, base, "inv", a))
        one = np.zeros(48, dtype=np.uint64); one[0] = 1
        zero_rows = ~a.any(axis=1)
        assert zero_rows.any() and (prod[~zero_rows] == one).all() and not prod[zero_rows].any()


@pytest.mark.parametrize("base", LAYOUTS, ids=[NAME[x] for x in LAYOUTS])
def test_layout_dependent_chain(engine, coracle, base):
    """12 dependent rounds of square, product, cyclotomic square: outputs fed back as inputs"""
    a, b = fp12_inputs(coracle, SEED + 710 + base, 5)
    x, ex = a.copy(), a.copy()
    for _ in range(12):
        x, ex = hook(engine, base, "sqr", x), coracle.fp12_op("sqr", ex)
        x, ex = hook(engine, base, "mul", x, b), coracle.fp12_op("mul", ex, b)
        x, ex = hook(engine, base, "cycsqr", x), coracle.fp12_op("cyclotomic_squared", ex)
    assert np.array_equal(x, ex), NAME[base]


def test_wide_pack_halves_do_not_leak(engine, coracle):
    """EPW = 2: an extreme element beside a zero or a one in the same wavefront, in both orders, odd n (the last half idles)"""
    vals = crafted_values()
    ext = [[vals[(5 * k + i) % len(vals)] for i in range(12)] for k in range(4)] + [[vals[0]] * 12, [P - 1] * 12]
    zero, one = [0] * 12, [1] + [0] * 11
    a_rows = []
    for e in ext:
        for other in (zero, one):
            a_rows += [e, other, other, e]
    a_rows.append(ext[0])                                         # n = 49
    a = rows(coracle, a_rows)
    b = rows(coracle, a_rows[7:] + a_rows[:7])
    for name in OPS[WIDE2] + ["final_exp"]:
        got = hook(engine, WIDE2, name, a, b)
        assert np.array_equal(got, hook(engine, WIDE1, name, a, b)), name
        if name == "final_exp":
            assert np.array_equal(got, coracle.final_exponentiation(a))
        else:
            assert np.array_equal(got, expected(coracle, name, a, b)), name
    for name in ("dbl", "add"):
        assert np.array_equal(hook(engine, WIDE2, name, a, b), hook(engine, WIDE1, name, a, b)), name


def cyclotomic(coracle, f):
    easy = coracle.fp12_op("mul", coracle.fp12_op("conj", f), coracle.fp12_op("inv", f))
    return coracle.fp12_op("mul", coracle.fp12_op("frobenius", easy, arg=2), easy)      # f^((p^6 - 1)(p^2 + 1))


def test_layout_expz(engine, coracle):
    """exp_by_neg_z on quads and on the wavefront, on cyclotomic elements made from crafted f, against ops 23 and 11 and the oracle's power"""
    a, _ = fp12_inputs(coracle, SEED + 720, 4)
    a = a[a.any(axis=1)][:41]
    cyc = cyclotomic(coracle, a)
    ref = engine.fp12_hook(LP + OFF["expz"], cyc)
    assert np.array_equal(ref, engine.fp12_hook(11, cyc))
    for base in LAYOUTS:
        assert np.array_equal(hook(engine, base, "expz", cyc), ref), NAME[base]
    for row in (0, 5, 17, 40):
        f = R.fp12_unflatten(coracle.from_limbs(cyc[row]))
        assert coracle.from_limbs(ref[row]) == R.fp12_flatten(R.fp12_unitary_inverse(R.gt_pow(f, R.BLS_X)))


def test_wide_final_exp_op(engine, coracle):
    a, _ = fp12_inputs(coracle, SEED + 730, 3)
    exp = coracle.final_exponentiation(a)
    for base in (WIDE1, WIDE2):
        assert np.array_equal(hook(engine, base, "final_exp", a), exp), NAME[base]


def miller_step_inputs(coracle, seed):
    """R = (X, Y, Z) with crafted Z, Q = (bx, by) crafted twist points, P crafted G1 points; then rows of random values (the formulas
    do not need the points on their curves, and neither does the oracle)"""
    rng = Xoshiro(seed)
    r_pts, q_pts, p_pts = crafted_g2_projective(), crafted_g2_points(), crafted_g1_points()
    n = len(r_pts)
    a_rows, p_rows = [], []
    for k in range(n):
        x, y, z = r_pts[k]
        bx, by = q_pts[(k * 5 + 3) % len(q_pts)]
        a_rows.append(list(x) + list(y) + list(z) + list(bx) + list(by) + [0, 0])
        p_rows.append(list(p_pts[k % len(p_pts)]))
    for k in range(10):
        a_rows.append([rng.fp() for _ in range(10)] + [0, 0])
        p_rows.append([rng.fp(), rng.fp()])
    a = rows(coracle, a_rows)
    b = np.zeros_like(a)
    b[:, :8] = coracle.to_limbs([v for r in p_rows for v in r]).reshape(-1, 8)
    return a, b


def test_miller_steps_every_layout(engine, coracle):
    a, b = miller_step_inputs(coracle, SEED + 740)
    assert a.shape[0] % 2 == 1
    want = {"dbl": coracle.g2_doubling_step(a[:, :24], b[:, :8]), "add": coracle.g2_addition_step(a[:, :24], a[:, 24:40], b[:, :8])}
    for name in ("dbl", "add"):
        for base in (LP, QUAD, WIDE1, WIDE2):
            assert np.array_equal(hook(engine, base, name, a, b), want[name]), (NAME[base], name)


ROUTES = {"wide1": {"WIDE_PACK": 0}, "wide2": {"WIDE_PACK": 1}, "quad": {"QUAD_MAX": 1 << 20, "WIDE_TAIL": 0},
          "lane_pair": {"QUAD_MAX": 0, "WIDE_TAIL": 0}}


def on_route(engine, route, fn):
    opts = ROUTES[route]
    prev = {k: engine.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        return fn()
    finally:
        for k, v in prev.items():
            engine.set_option(k, v)


def crafted_pairs(coracle, n):
    g1, g2 = crafted_g1_points(), crafted_g2_points()
    p = coracle.to_limbs([v for k in range(n) for v in g1[k % len(g1)]]).reshape(n, 8)
    q = coracle.to_limbs([c for k in range(n) for xy in g2[(3 * k + 1) % len(g2)] for c in xy]).reshape(n, 16)
    return p, q


def proj(p, q):
    n = p.shape[0]
    one4 = np.zeros((n, 4), dtype=np.uint64); one4[:, 0] = 1
    return np.concatenate([p, one4], axis=1), np.concatenate([q, one4, np.zeros((n, 4), dtype=np.uint64)], axis=1)


@pytest.mark.parametrize("route", list(ROUTES))
def test_entry_points_every_route(engine, coracle, route):
    n = 27
    p, q = crafted_pairs(coracle, n)
    f_rows, _ = fp12_inputs(coracle, SEED + 750, 0)
    f_rows = f_rows[:33]                                          # every crafted shape: 0, 1, subfields, half-zero rows, ...
    raw = on_route(engine, route, lambda: engine.miller_loop(p, q))
    assert np.array_equal(raw, coracle.miller_loop(p, q))
    f = np.concatenate([f_rows, raw[:8]])                         # 41 rows
    assert np.array_equal(on_route(engine, route, lambda: engine.final_exp(f)), coracle.final_exponentiation(f))
    pp, qp = proj(p, q)
    assert np.array_equal(on_route(engine, route, lambda: engine.pairing(p, q, pipelined=False)), coracle.pairing(pp, qp))


@pytest.fixture(scope="module")
def g2_multiples(engine):
    rng = Xoshiro(SEED + 760)
    q, _ = engine.g2_scalar_mul(np.repeat(np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for v in G2 for k in range(4)]], dtype=np.uint64), 9, 0),
                                np.array([[rng.next(), rng.next(), rng.next(), rng.next() >> 4] for _ in range(9)], dtype=np.uint64))
    return q


@pytest.mark.parametrize("tables", [0, 1])
def test_products_crafted_g1(engine, coracle, g2_multiples, tables):
    """crafted G1 points with multiples of the G2 generator: one pair (k_miller_single_wide) and ecPairing-shaped jobs of 1 .. 3 pairs"""
    q = g2_multiples
    n = q.shape[0]
    p, _ = crafted_pairs(coracle, n)
    pp, qp = proj(p, q)
    gt, _ = engine.pairing_product(p[:1], q[:1], skip_infinity=True)
    assert np.array_equal(gt, coracle.pairing(pp[:1], qp[:1]))
    off = np.array([0, 1, 3, 6, 9], dtype=np.uint64)
    prev = engine.get_option("MULTI_TABLES")
    try:
        engine.set_option("MULTI_TABLES", tables)
        got, _ = engine.multi_pairing(p, q, off, skip_infinity=True)
    finally:
        engine.set_option("MULTI_TABLES", prev)
    assert np.array_equal(got, coracle.glued_pairing(pp, qp, off))


def test_public_cyclotomic_sqr(engine, coracle):
    a, _ = fp12_inputs(coracle, SEED + 770, 21)
    assert np.array_equal(engine.fp12_cyclotomic_sqr(a), coracle.fp12_op("cyclotomic_squared", a))


def test_hook_rejects_ops_a_layout_lacks(engine, coracle):
    a, _ = fp12_inputs(coracle, SEED + 780, 1)
    for op in (QUAD + OFF["inv"], QUAD + OFF["final_exp"], WIDE1 + OFF["conj"], WIDE2 + 9, 80, 12):
        with pytest.raises(Exception):
            engine.fp12_hook(op, a[:2])
    with pytest.raises(Exception):
        engine.fp12_hook(WIDE1 + OFF["dbl"], a[:2])               # the Miller steps need P in b
