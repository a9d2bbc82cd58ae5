"""GPU: sylow_hip_g2_sum_batch, sylow_hip_g2_lincomb_batch, sylow_hip_g2_msm / _tuned (g2_msm.hpp): many G2 points into one.  Everything is
bit-exact against the oracle (coracle.g2_scalar_mul with canonical scalars k mod p, folded with its complete addition); both routes of the
multi-scalar multiplication -- the bucket method forced with min_n = 0, the composed route (a scalar multiplication per lane pair + the
segmented sum) forced with a huge min_n.  The scalar rule is that of sylow_hip_g2_scalar_mul_batch: exact on the whole twist, no mod r."""
import os
import sys

import numpy as np
import pytest

from helpers import P, SEED, Xoshiro, crafted_g2_points, fp2_sqrt, limbs, pack
from oracle import pyref as PR

pytestmark = pytest.mark.gpu

R = PR.R_ORDER
ROUTES = {"bucket": 0, "small": 1 << 40}
ID24 = limbs([0, 0, 1, 0, 0, 0]).reshape(24)
ID_XY = pack([0, 0, 1, 0], 16).reshape(16)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def gen_points(engine, a):
    """a_i * G2 through the fixed-base table ([n, 16] affine words, flags)"""
    return engine.g2_generator_mul(limbs(a))


def proj(xy, inf=None):
    n = xy.shape[0]
    z = np.zeros((n, 8), dtype=np.uint64)
    z[:, 0] = 1
    out = np.concatenate([xy, z], axis=1)
    if inf is not None:
        out[np.asarray(inf).astype(bool)] = ID24
    return out


def fold(C, acc):
    """pairwise fold with the oracle's complete addition -> (affine [1, 16], flag [1])"""
    if acc.shape[0] == 0:
        return C.g2_to_affine(ID24.reshape(1, 24))
    while acc.shape[0] > 1:
        h = acc.shape[0] // 2
        acc = np.concatenate([C.g2_add(acc[:h], acc[h:2 * h]), acc[2 * h:]], axis=0)
    return C.g2_to_affine(acc)


def oracle_msm(C, xy, inf, k):
    """the oracle takes canonical scalars: apply Fp::new (k mod p) here, as the library does -- and nothing else"""
    if xy.shape[0] == 0:
        return fold(C, np.zeros((0, 24), dtype=np.uint64))
    return fold(C, C.g2_scalar_mul(proj(xy, inf), limbs([v % P for v in C.from_limbs(k)])))


def affine_of(C, e):
    """e * G2 affine (oracle), e < p"""
    return C.g2_to_affine(C.g2_scalar_mul(proj(pack(PR_G2(), 16)), limbs([e])))


def PR_G2():
    from test_gpu_multi_pairing import G2
    return G2


def same(got, exp):
    return np.array_equal(np.asarray(got[0]).reshape(-1, 16), np.asarray(exp[0]).reshape(-1, 16)) and np.array_equal(got[1], exp[1])


def check(engine, C, xy, k, inf=None, route=None, window=-1):
    exp = oracle_msm(C, xy, inf, k)
    got = engine.g2_msm(xy, k, inf, window=window, min_n=-1 if route is None else ROUTES[route])
    assert same(got, exp), (route, xy.shape[0])
    return got


def is_identity(got):
    return got[1][0] == 1 and np.array_equal(np.asarray(got[0]).reshape(16), ID_XY)


def neg_points(xy):
    out = xy.copy()
    y = [sum(int(xy[i, 8 + j]) << (64 * j) for j in range(8)) for i in range(xy.shape[0])]
    for i, v in enumerate(y):
        c0, c1 = v & ((1 << 256) - 1), v >> 256
        out[i, 8:16] = limbs([(P - c0) % P, (P - c1) % P]).reshape(8)
    return out


@pytest.fixture(scope="module")
def base_points(engine):
    """1000 generator multiples, shared (never modified)"""
    rng = Xoshiro(SEED + 800)
    a = [rng.fp() % R or 1 for _ in range(1000)]
    xy, _ = gen_points(engine, a)
    return a, xy


@pytest.fixture(scope="module")
def small_order_points(engine, coracle):
    """twist points of order 10069 (tests/test_gpu_groups.py: S = [r (2p - r) / 10069] T for random twist points T)"""
    h2 = 2 * P - R
    assert h2 % 10069 == 0
    rng = Xoshiro(SEED + 29)
    tw = []
    while len(tw) < 6:
        x = (rng.fp(), rng.fp())
        y = fp2_sqrt(PR.fp2_add(PR.fp2_mul(PR.fp2_square(x), x), PR.TWIST_B))
        if y is not None:
            tw.append(list(x) + list(y))
    t = pack([v for q in tw for v in q], 16)
    s1, i1 = engine.g2_scalar_mul(t, limbs([h2 // 10069] * 6))
    s, si = engine.g2_scalar_mul(s1, limbs([R] * 6), i1)
    sl = s[np.flatnonzero(si == 0)]
    assert sl.shape[0] >= 1
    chk, chi = coracle.g2_to_affine(coracle.g2_scalar_mul(proj(sl), limbs([10069] * sl.shape[0])))
    assert chi.all()                                            # order divides 10069 (a prime), and the points are not the identity
    return sl


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 127, 128, 129, 1000])
def test_small_n_against_the_oracle_fold(engine, coracle, base_points, n, route):
    rng = Xoshiro(SEED + 810 + n)
    k = limbs([rng.u256() for _ in range(n)])                   # full 256-bit words: many are >= p
    check(engine, coracle, base_points[1][:n], k, route=route)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
SPECIAL = [R - 1, R, R + 1, 2 * R, P - 1, P, P + 1, (1 << 255) - 1, (1 << 256) - 1, 3 * P + 7]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_scalar_rule_holds_on_the_whole_twist(engine, coracle, base_points, small_order_points, route):
    so = small_order_points
    # k = r on a point of order 10069 is NOT the identity (r is no multiple of 10069): a route that reduced mod r would return it
    assert R % 10069 != 0
    exp_r = coracle.g2_to_affine(coracle.g2_scalar_mul(proj(so[:1]), limbs([R])))
    assert exp_r[1][0] == 0
    got = check(engine, coracle, so[:1], limbs([R]), route=route)
    assert not is_identity(got)
    crafted = np.array([limbs([*x, *y]).reshape(16) for x, y in crafted_g2_points(8)])
    pts = np.concatenate([so, base_points[1][:12], crafted], axis=0)
    n = pts.shape[0]
    rng = Xoshiro(SEED + 820)
    order = [int(rng.next() % n) for _ in range(3 * n)]
    mixed = pts[order]
    check(engine, coracle, mixed, limbs([SPECIAL[i % len(SPECIAL)] for i in range(3 * n)]), route=route)      # together
    for s in SPECIAL:                                                                                   # one at a time
        check(engine, coracle, pts, limbs([s] * n), route=route)
        check(engine, coracle, so[:1], limbs([s]), route=route)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_edge_cases_at_n_300(engine, coracle, base_points, route):
    rng = Xoshiro(SEED + 830)
    n = 300
    xy = base_points[1][:n]
    k = limbs([rng.fp() for _ in range(n)])
    got = engine.g2_msm(np.zeros((0, 16), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), min_n=ROUTES[route])
    assert is_identity(got)
    # every flag set over garbage coordinates / every scalar zero
    garbage = limbs([rng.u256() for _ in range(4 * n)]).reshape(n, 16)
    assert is_identity(check(engine, coracle, garbage, k, np.ones(n, dtype=np.uint8), route))
    assert is_identity(check(engine, coracle, xy, np.zeros_like(k), route=route))
    # one point repeated (doublings inside a bucket), with random and with equal scalars
    rep = np.repeat(xy[:1], n, 0)
    check(engine, coracle, rep, k, route=route)
    check(engine, coracle, rep, np.repeat(k[:1], n, 0), route=route)
    # Q and -Q under one scalar, alone: every bucket cancels
    h = n // 2
    neg = neg_points(xy[:h])
    kk = np.concatenate([k[:h], k[:h]], axis=0)
    assert is_identity(check(engine, coracle, np.concatenate([xy[:h], neg], axis=0), kk, route=route))
    # the same, mixed with other terms and flags
    inf = np.zeros(n + h, dtype=np.uint8)
    inf[5] = inf[n + 3] = 1
    check(engine, coracle, np.concatenate([xy, neg], axis=0), np.concatenate([k, k[:h]], axis=0), inf, route)


@pytest.mark.parametrize("n", [2, 129])
def test_identity_result_from_non_identity_terms(engine, coracle, base_points, n):
    """sum k_i a_i = 0 mod r over generator multiples a_i G2 with every term non-zero"""
    rng = Xoshiro(SEED + 840 + n)
    a, xy = base_points[0][:n], base_points[1][:n]
    k = [rng.fp() % R or 1 for _ in range(n - 1)]
    k.append((-sum(x * y for x, y in zip(k, a)) * pow(a[-1], -1, R)) % R)
    assert k[-1] != 0
    for route in sorted(ROUTES):
        assert is_identity(check(engine, coracle, xy, limbs(k), route=route))


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_points(engine):
    """8193 generator multiples and their discrete logarithms, shared"""
    rng = np.random.default_rng(SEED + 850)
    aw = rng.integers(0, 1 << 63, size=(8193, 4), dtype=np.uint64)
    aw[:, 3] &= np.uint64((1 << 60) - 1)                      # a_i < 2^252 < r
    xy, inf = engine.g2_generator_mul(aw)
    w = aw.astype(object)
    return list(w[:, 0] + (w[:, 1] << 64) + (w[:, 2] << 128) + (w[:, 3] << 192)), xy


@pytest.mark.parametrize("n", [32, 33, 256, 257, 300, 8193])
def test_equal_scalars_segment_and_join_boundaries(engine, coracle, many_points, n):
    """one bucket per window holds every point: one segment, two segments, the last bucket joined by one lane pair (8 segments), the first joined
    by the block (9 segments), a wide join whose strided loop runs more than once (257 segments > 128 lane pairs)"""
    a, xy = many_points[0][:n], many_points[1][:n]
    rng = Xoshiro(SEED + 860 + n)
    for kv in (rng.u256(), 1, P - 1):
        exp = affine_of(coracle, ((kv % P) * (sum(a) % R)) % R)
        got = engine.g2_msm(xy, np.repeat(limbs([kv]), n, 0), min_n=0)
        assert same(got, exp), (n, kv)
    assert same(engine.g2_msm(xy, np.repeat(limbs([kv]), n, 0), min_n=1 << 40), exp)


def test_zero_one_scalars_window_4(engine, coracle, many_points):
    n = 4097
    a, xy = many_points[0][:n], many_points[1][:n]
    bits = np.random.default_rng(SEED + 870).integers(0, 2, size=n)
    k = np.zeros((n, 4), dtype=np.uint64)
    k[:, 0] = bits.astype(np.uint64)
    exp = affine_of(coracle, sum(ai for ai, b in zip(a, bits) if b) % R)
    assert same(engine.g2_msm(xy, k, window=4, min_n=0), exp)


# ---- 5 / 6 ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def n4097(engine, many_points):
    n = 4097
    rng = Xoshiro(SEED + 880)
    xy = many_points[1][:n]
    k = limbs([rng.u256() for _ in range(n)])
    inf = np.zeros(n, dtype=np.uint8)
    inf[::97] = 1
    ref = engine.g2_msm(xy, k, inf, min_n=1 << 40)
    return xy, k, inf, ref


def test_every_window_width_at_2049(engine, n4097):
    import sylow_amd
    xy, k, inf = (a[:2049] for a in n4097[:3])
    ref = engine.g2_msm(xy, k, inf, min_n=1 << 40)
    for c in range(4, 17):
        assert same(engine.g2_msm(xy, k, inf, window=c, min_n=0), ref), c
    for bad in (3, 17):
        with pytest.raises(sylow_amd._lib.SylowHipError):
            engine.g2_msm(xy[:10], k[:10], window=bad)


def test_scratch_limit_forces_chunks(engine, n4097):
    import msm_model as M
    xy, k, inf, ref = n4097
    n = xy.shape[0]
    c = M.g2_default_window(n)
    try:
        for parts in (2, 7):
            budget = M.g2_scratch_bytes(c, n // parts)
            nc, _ = M.g2_plan(n, c, budget)
            assert nc < n and -(-n // nc) > 1                  # the model plans more than one chunk
            engine.set_scratch_limit(budget)
            assert same(engine.g2_msm(xy, k, inf, min_n=0), ref), parts
        assert M.g2_plan(n, c, M.g2_fixed_bytes(c)) is None
        engine.set_scratch_limit(M.g2_fixed_bytes(c))           # not even one chunk: the composed route, same point
        assert same(engine.g2_msm(xy, k, inf, min_n=0), ref)
    finally:
        engine.set_scratch_limit(0)


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------
def test_msm_is_bit_identical_to_lincomb_with_one_job(engine, n4097):
    xy, k, inf, ref = n4097
    exp = engine.g2_lincomb(xy, k, 1, xy.shape[0], inf)
    assert same(ref, exp)
    for min_n in (-1, 0):                                       # the default route for this n, then the bucket route forced
        assert same(engine.g2_msm(xy, k, inf, min_n=min_n), exp), min_n


@pytest.mark.parametrize("shape", [(1, 1), (5, 0), (33, 7), (3, 130)])
def test_lincomb_against_the_oracle_per_job(engine, coracle, base_points, shape):
    nj, nt = shape
    n = nj * nt
    rng = Xoshiro(SEED + 890 + n)
    xy = base_points[1][:n]
    k = limbs([rng.u256() for _ in range(n)]).reshape(n, 4)
    inf = np.zeros(n, dtype=np.uint8)
    inf[3::11] = 1
    gxy, gi = engine.g2_lincomb(xy, k, nj, nt, inf)
    assert gxy.shape == (nj, 16) and gi.shape == (nj,)
    for j in range(nj):                                         # term-major: term i of job j is row i * n_jobs + j
        exp = oracle_msm(coracle, xy[j::nj], inf[j::nj], k[j::nj])
        assert same((gxy[j:j + 1], gi[j:j + 1]), exp), j
    if nt == 0:
        assert gi.all() and all(np.array_equal(gxy[j], ID_XY) for j in range(nj))


@pytest.mark.parametrize("n", [0, 1, 2, 33, 1000])
def test_sum_against_the_oracle_fold(engine, coracle, base_points, n):
    xy = base_points[1][:n]
    inf = np.zeros(n, dtype=np.uint8)
    inf[4::13] = 1
    assert same(engine.g2_sum(xy, inf), fold(coracle, proj(xy, inf)))
    got = engine.g2_sum(xy)
    assert same(got, fold(coracle, proj(xy)))
    if n == 0:
        assert is_identity(got)


def test_sum_with_a_point_its_negative_and_flags(engine, coracle, base_points):
    xy = base_points[1][:40]
    pts = np.concatenate([xy, neg_points(xy[:17]), xy[:3]], axis=0)
    inf = np.zeros(pts.shape[0], dtype=np.uint8)
    inf[[2, 41, 58]] = 1
    assert same(engine.g2_sum(pts, inf), fold(coracle, proj(pts, inf)))
    both = np.concatenate([xy[:9], neg_points(xy[:9])], axis=0)
    assert is_identity(engine.g2_sum(both))


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------
def test_api_round_trip(engine, coracle, base_points):
    from sylow_amd import api
    rng = Xoshiro(SEED + 900)
    n = 777
    xy = base_points[1][:n]
    inf = np.zeros(n, dtype=np.uint8)
    inf[3] = 1
    pts = api.G2Affine(xy, inf)
    w = api.Fr(limbs([rng.fp() % R for _ in range(n)]))
    q = api.msm(pts, w)
    assert isinstance(q, api.G2Affine) and len(q) == 1
    agg = api.aggregate(pts, w, 1, n)
    assert isinstance(agg, api.G2Affine) and np.array_equal(q.xy, agg.xy) and np.array_equal(q.infinity, agg.infinity)
    exp_xy, exp_inf = oracle_msm(coracle, xy, inf, w.v)
    assert np.array_equal(q.xy, exp_xy.reshape(1, 16)) and q.infinity[0] == exp_inf[0]
    s = api.point_sum(pts)
    assert isinstance(s, api.G2Affine) and same((s.xy, s.infinity), fold(coracle, proj(xy, inf)))
    with pytest.raises(ValueError):
        api.msm(pts, api.Fr(w.v[:-1]))
    g1, g1i = engine.g1_generator_mul(w.v[:50])
    p1 = api.G1Affine(g1, g1i)
    for r in (api.msm(p1, api.Fr(w.v[:50])), api.aggregate(p1, api.Fr(w.v[:50]), 1, 50), api.point_sum(p1)):
        assert isinstance(r, api.G1Affine) and len(r) == 1
    assert bool((api.msm(p1, api.Fr(w.v[:50])) == api.aggregate(p1, api.Fr(w.v[:50]), 1, 50))[0])


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------
def test_short_buffer_is_refused_before_the_launch(engine):
    import sylow_amd
    n = 64
    out, oi = engine.empty((16, 1)), engine.empty((1,), np.uint8)
    p, kk = engine.empty((16, n)), engine.empty((4, n - 1))
    p_short, kf = engine.empty((16, n - 1)), engine.empty((4, n))
    for sym, extra in (("sylow_hip_g2_msm", ()), ("sylow_hip_g2_msm_tuned", (-1, 0))):
        with pytest.raises(sylow_amd._lib.SylowHipError, match="k holds"):
            engine._call(sym, p.ptr, None, kk.ptr, n, *extra, out.ptr, oi.ptr)
        with pytest.raises(sylow_amd._lib.SylowHipError, match="p_xy holds"):
            engine._call(sym, p_short.ptr, None, kf.ptr, n, *extra, out.ptr, oi.ptr)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="q_xy holds"):
        engine._call("sylow_hip_g2_sum_batch", p_short.ptr, None, n, out.ptr, oi.ptr)
    outs, ois = engine.empty((16, 4)), engine.empty((4,), np.uint8)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="k holds"):
        engine._call("sylow_hip_g2_lincomb_batch", p.ptr, None, kk.ptr, outs.ptr, ois.ptr, 4, 16)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="out_xy holds"):
        engine._call("sylow_hip_g2_lincomb_batch", p.ptr, None, kf.ptr, out.ptr, ois.ptr, 4, 16)
