"""GPU: sylow_hip_g1_msm (msm.hip), sum_i k_i P_i as one point.  Small n against the oracle's fold of scalar multiplications, both
routes (the bucket method forced with min_n = 0, the per-lane scalar multiplication + sum forced with a huge min_n, both through
sylow_hip_g1_msm_tuned); larger n bit-identical to sylow_hip_g1_lincomb_batch(n_jobs = 1); 2^20 (+ 77) against one big-int sum and one oracle scalar multiplication."""
import numpy as np
import pytest

from helpers import SEED, Xoshiro, limbs, pack

pytestmark = pytest.mark.gpu

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
G1 = [1, 2]
ROUTES = {"bucket": 0, "small": 1 << 40}


def gen_points(engine, a):
    """a_i * G through the fixed-base table ([n, 8] affine words, flags)"""
    return engine.g1_generator_mul(limbs(a))


def oracle_msm(C, xy, inf, k):
    n = xy.shape[0]
    if n == 0:
        return C.g1_to_affine(C.to_limbs([0, 1, 0]).reshape(1, 12))
    z = np.zeros((n, 4), dtype=np.uint64)
    z[:, 0] = 1
    proj = np.concatenate([xy, z], axis=1)
    proj[inf.astype(bool)] = C.to_limbs([0, 1, 0]).reshape(12)
    # the oracle takes canonical Fp scalars (it reduces raw words straight mod r): apply Fp::new here, as the library does
    acc = C.g1_scalar_mul(proj, limbs([v % P for v in C.from_limbs(k)]))
    while acc.shape[0] > 1:                                  # pairwise fold with the oracle's complete addition
        h = acc.shape[0] // 2
        s = C.g1_add(acc[:h], acc[h:2 * h])
        acc = np.concatenate([s, acc[2 * h:]], axis=0)
    return C.g1_to_affine(acc)


def check(engine, C, xy, k, inf=None, route=None):
    infa = np.zeros(xy.shape[0], dtype=np.uint8) if inf is None else inf
    exp_xy, exp_inf = oracle_msm(C, xy, infa, k)
    got_xy, got_inf = engine.g1_msm(xy, k, inf, min_n=-1 if route is None else ROUTES[route])
    assert np.array_equal(got_xy.reshape(1, 8), exp_xy.reshape(1, 8)) and got_inf[0] == exp_inf[0]
    return got_xy, got_inf


def affine_of(C, e):
    """e * G affine (oracle)"""
    return C.g1_to_affine(C.g1_scalar_mul(C.to_limbs([1, 2, 1]).reshape(1, 12), C.to_limbs([e])))


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000, 4097])
def test_small_n_against_the_oracle(engine, coracle, n, route):
    rng = Xoshiro(SEED + 700 + n)
    xy, _ = gen_points(engine, [rng.fp() for _ in range(n)])
    k = limbs([rng.u256() for _ in range(n)])                 # full 256-bit words: many are >= p
    check(engine, coracle, xy, k, route=route)


@pytest.mark.parametrize("n", [(1 << 13) + 1, (1 << 16) + 3])
def test_bit_identical_to_lincomb(engine, n):
    rng = Xoshiro(SEED + 710 + n)
    xy, _ = gen_points(engine, [rng.fp() for _ in range(n)])
    k = limbs([rng.fp() for _ in range(n)])
    inf = np.zeros(n, dtype=np.uint8)
    inf[::97] = 1
    exp_xy, exp_inf = engine.g1_lincomb(xy, k, 1, n, inf)
    for min_n in (-1, 0):                                    # the default route for this n, then the bucket route forced
        got_xy, got_inf = engine.g1_msm(xy, k, inf, min_n=min_n)
        assert np.array_equal(got_xy, exp_xy) and np.array_equal(got_inf, exp_inf), min_n


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_edge_cases_against_the_oracle(engine, coracle, route):
    rng = Xoshiro(SEED + 720)
    n = 300
    xy, _ = gen_points(engine, [rng.fp() for _ in range(n)])
    k = limbs([rng.fp() for _ in range(n)])
    # n = 0: the identity
    ex, ei = engine.g1_msm(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), min_n=ROUTES[route])
    assert ei[0] == 1 and np.array_equal(ex.reshape(8), pack([0, 1], 8).reshape(8))
    # every point at infinity (garbage coordinates under the flag) / every scalar zero: the identity
    _, gi = check(engine, coracle, limbs([rng.u256() for _ in range(2 * n)]).reshape(n, 8), k, np.ones(n, dtype=np.uint8), route)
    assert gi[0] == 1
    _, gi = check(engine, coracle, xy, np.zeros_like(k), route=route)
    assert gi[0] == 1
    # the scalar rule: 1, r - 1, r, p - 1 and values >= p up to 2^256 - 1 (Fp::new first, then mod r)
    special = [1, R - 1, R, R + 1, P - 1, P, P + 1, 2 * R, (1 << 255) - 1, (1 << 256) - 1, (1 << 256) - 2, 3 * P + 7]
    ks = limbs([special[i % len(special)] for i in range(n)])
    check(engine, coracle, xy, ks, route=route)
    for s in special:                                          # one scalar at a time on one point
        check(engine, coracle, xy[:1], limbs([s]), route=route)
    # the same point repeated (doublings inside a bucket), with equal and with random scalars
    rep = np.repeat(xy[:1], n, 0)
    check(engine, coracle, rep, k, route=route)
    check(engine, coracle, rep, np.repeat(k[:1], n, 0), route=route)
    # P and -P with one scalar: every bucket cancels to the identity
    neg = xy[:n // 2].copy()
    neg[:, 4:8] = limbs([P - v for v in _ints_y(xy[:n // 2])])
    kk = np.concatenate([k[:n // 2], k[:n // 2]], axis=0)
    _, gi = check(engine, coracle, np.concatenate([xy[:n // 2], neg], axis=0), kk, route=route)
    assert gi[0] == 1
    # the same, mixed with other terms and flags
    inf = np.zeros(n + n // 2, dtype=np.uint8)
    inf[5] = inf[n + 3] = 1
    check(engine, coracle, np.concatenate([xy, neg], axis=0), np.concatenate([k, k[:n // 2]], axis=0), inf, route)


def _ints_y(xy):
    return [sum(int(xy[i, 4 + j]) << (64 * j) for j in range(4)) for i in range(xy.shape[0])]


def _bucket_and_small(engine, xy, k, inf=None):
    outs = []
    for route in sorted(ROUTES):
        outs.append(engine.g1_msm(xy, k, inf, min_n=ROUTES[route]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


def test_identity_result_from_non_identity_terms(engine, coracle):
    """sum k_i a_i = 0 mod r with every term non-zero"""
    rng = Xoshiro(SEED + 730)
    for n in (2, 129, 5000):
        a = [rng.fp() % R or 1 for _ in range(n)]
        k = [rng.fp() % R or 1 for _ in range(n - 1)]
        k.append((-sum(x * y for x, y in zip(k, a)) * pow(a[-1], -1, R)) % R)
        assert k[-1] != 0
        xy, _ = gen_points(engine, a)
        gxy, gi = _bucket_and_small(engine, xy, limbs(k))
        assert gi[0] == 1 and np.array_equal(gxy.reshape(8), pack([0, 1], 8).reshape(8))
    check(engine, coracle, xy[:129], limbs(k[:129]), route="bucket")


def test_all_equal_scalars_hot_bucket(engine, coracle):
    """every point in ONE bucket per window, n = 2^16: sum = k * (sum a_i) G"""
    rng = Xoshiro(SEED + 740)
    n = 1 << 16
    a = [rng.fp() for _ in range(n)]
    xy, _ = gen_points(engine, a)
    kv = rng.u256()
    k = np.repeat(limbs([kv]), n, 0)
    exp_xy, exp_inf = affine_of(coracle, ((kv % P) * (sum(a) % R)) % R)
    gxy, gi = _bucket_and_small(engine, xy, k)
    assert np.array_equal(gxy.reshape(1, 8), exp_xy.reshape(1, 8)) and gi[0] == exp_inf[0] == 0
    for kv in (1, R - 1, (1 << 255) + 3):                    # a single non-zero digit / all digits equal / k >= p
        exp_xy, _ = affine_of(coracle, ((kv % P) * (sum(a) % R)) % R)
        gxy, gi = engine.g1_msm(xy, np.repeat(limbs([kv]), n, 0), min_n=0)
        assert np.array_equal(gxy.reshape(1, 8), exp_xy.reshape(1, 8)) and gi[0] == 0


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 77])
def test_full_size(engine, coracle, n):
    rng = np.random.default_rng(SEED + n)
    aw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    aw[:, 3] &= np.uint64((1 << 60) - 1)                     # a_i < 2^252 < p
    kw = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)   # k_i up to 2^256 - 1
    xy, inf = engine.g1_generator_mul(aw)
    a = _words_to_ints(aw)
    k = _words_to_ints(kw)
    e = sum((ki % P) * ai for ki, ai in zip(k, a)) % R
    exp_xy, exp_inf = affine_of(coracle, e)
    gxy, gi = engine.g1_msm(xy, kw, inf)
    assert np.array_equal(gxy.reshape(1, 8), exp_xy.reshape(1, 8)) and gi[0] == exp_inf[0]


@pytest.mark.parametrize("kind", ["all_equal", "zero_one"])
def test_full_size_hot_buckets(engine, coracle, kind):
    """2^20 on the default (bucket) route with hot buckets: every scalar equal (one bucket per window holds every point) and scalars from
    {0, 1} (half the points in one bucket of window 0)"""
    n = 1 << 20
    rng = np.random.default_rng(SEED + 7 + len(kind))
    aw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    aw[:, 3] &= np.uint64((1 << 60) - 1)
    if kind == "all_equal":
        kw = np.repeat(rng.integers(0, 1 << 64, size=(1, 4), dtype=np.uint64), n, 0)
    else:
        kw = np.zeros((n, 4), dtype=np.uint64)
        kw[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint64)
    xy, inf = engine.g1_generator_mul(aw)
    e = sum((ki % P) * ai for ki, ai in zip(_words_to_ints(kw), _words_to_ints(aw))) % R
    exp_xy, exp_inf = affine_of(coracle, e)
    gxy, gi = engine.g1_msm(xy, kw, inf)
    assert np.array_equal(gxy.reshape(1, 8), exp_xy.reshape(1, 8)) and gi[0] == exp_inf[0]


def _words_to_ints(w):
    w = w.astype(object)
    return list(w[:, 0] + (w[:, 1] << 64) + (w[:, 2] << 128) + (w[:, 3] << 192))


@pytest.fixture(scope="module")
def n16(engine):
    rng = Xoshiro(SEED + 750)
    n = 1 << 16
    xy, _ = gen_points(engine, [rng.fp() for _ in range(n)])
    k = limbs([rng.u256() for _ in range(n)])
    inf = np.zeros(n, dtype=np.uint8)
    inf[7::1001] = 1
    ref = engine.g1_msm(xy, k, inf, min_n=1 << 40)
    return xy, k, inf, ref


def test_scratch_limit_forces_chunks(engine, n16):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import msm_model as M
    xy, k, inf, ref = n16
    n = xy.shape[0]
    c = M.default_window(n)
    try:
        for parts in (2, 7):
            budget = M.scratch_bytes(c, n // parts)
            nc, _ = M.plan(n, c, budget)
            assert nc < n
            engine.set_scratch_limit(budget)
            got = engine.g1_msm(xy, k, inf, min_n=0)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), parts
        engine.set_scratch_limit(M.fixed_bytes(c))             # not even one chunk: the per-lane route, same point
        got = engine.g1_msm(xy, k, inf, min_n=0)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    finally:
        engine.set_scratch_limit(0)


def test_every_window_width_and_the_small_route(engine, n16):
    xy, k, inf, ref = n16
    for c in range(4, 17):
        got = engine.g1_msm(xy, k, inf, window=c, min_n=0)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), c
    got = engine.g1_msm(xy, k, inf)                             # defaults
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    import sylow_amd
    for bad in (3, 17):
        with pytest.raises(sylow_amd._lib.SylowHipError):
            engine.g1_msm(xy[:10], k[:10], window=bad)


def test_api_round_trip(engine, coracle):
    from sylow_amd import api
    rng = Xoshiro(SEED + 760)
    n = 777
    xy, inf = gen_points(engine, [rng.fp() for _ in range(n)])
    inf = inf.copy()
    inf[3] = 1
    pts = api.G1Affine(xy, inf)
    w = api.Fr(limbs([rng.fp() % R for _ in range(n)]))
    q = api.msm(pts, w)
    assert isinstance(q, api.G1Affine) and len(q) == 1
    agg = api.aggregate(pts, w, 1, n)
    assert bool((q == agg)[0])
    exp_xy, exp_inf = oracle_msm(coracle, xy, inf, w.v)
    assert np.array_equal(q.xy, exp_xy.reshape(1, 8)) and q.infinity[0] == exp_inf[0]
    assert bool(api.msm(api.G1Affine(xy[:0]), api.Fr(np.zeros((0, 4), dtype=np.uint64))).is_zero()[0])
    with pytest.raises(ValueError):
        api.msm(pts, api.Fr(w.v[:-1]))


def test_short_buffer_is_refused_before_the_launch(engine):
    import sylow_amd
    n = 64
    p, kk = engine.empty((8, n)), engine.empty((4, n - 1))
    out, oi = engine.empty((8, 1)), engine.empty((1,), np.uint8)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="k holds"):
        engine._call("sylow_hip_g1_msm", p.ptr, None, kk.ptr, n, out.ptr, oi.ptr)
    p_short, kf = engine.empty((8, n - 1)), engine.empty((4, n))
    with pytest.raises(sylow_amd._lib.SylowHipError, match="p_xy holds"):
        engine._call("sylow_hip_g1_msm", p_short.ptr, None, kf.ptr, n, out.ptr, oi.ptr)
