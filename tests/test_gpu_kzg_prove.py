"""GPU: the prover's half of KZG under one SRS -- sylow_hip_kzg_quotient_batch, sylow_hip_kzg_commit_batch(_tuned) and sylow_hip_kzg_open_batch
(kzg_prove.hip) against the integer model of tests/kzg_prove_model.py.  Everything is exact: the quotient word for word against the
recurrence, the points word for word against the oracle's generator multiples f(tau) G1gen and q(tau) G1gen, and the round trip
commit -> open -> KzgVerifier.verify.  Sizes come from kzg_prove_plan.hpp (a lane's coefficients L, a chunk CH = 256 L); the SRS (2049
points) and the model's values are made once per module."""
import ctypes
import random

import numpy as np
import pytest

import kzg_prove_model as M
from kzg_prove_model import P, R, TOP

pytestmark = pytest.mark.gpu
E_ARG = -2
K = M.plan_constants()
L, BLOCK, CH = K["KZG_POLY_LANE_COEFFS"], K["KZG_POLY_BLOCK"], K["KZG_POLY_CHUNK"]
TAU = 0x1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA987654321 % R
EDGE_WORDS = [0, R, R + 1, P, TOP, R - 1, 1]
IDENTITY = M.limbs([0, 1]).reshape(8)


@pytest.fixture(scope="module")
def srs():
    return M.srs_points(TAU, CH + 1)


def rand_poly(rng, n, edges=True):
    f = [rng.randrange(R) for _ in range(n)]
    if edges:                                                   # the special words at both ends and wherever they fit
        for i, w in enumerate(EDGE_WORDS):
            if 2 * i < n:
                f[(i * 37) % n if i % 2 else n - 1 - (i * 11) % n] = w
    return f


def check_quotient(engine, polys, zs):
    q, y = engine.kzg_quotient(M.poly_words(polys), M.limbs(zs))
    want = [M.quotient(f, z) for f, z in zip(polys, zs)]
    assert np.array_equal(y, M.limbs([w[1] for w in want])), "y"
    for j, (wq, _) in enumerate(want):
        assert np.array_equal(q[j], M.limbs(wq)), f"q of polynomial {j}: {int((q[j] != M.limbs(wq)).any(axis=1).sum())} coefficients differ"
    return q, y


# ---- the quotient ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, L - 1, L + 1, CH - 1, CH, CH + 1, 2 * CH + 1, 3 * CH + L + 1])
def test_quotient_one_polynomial(engine, n):
    rng = random.Random(0xA0 + n)
    q, _ = check_quotient(engine, [rand_poly(rng, n)], [rng.randrange(R)])
    assert not q[0, n - 1].any()                                # q[len - 1] = 0 is written
    assert all(v < R for v in M.ints(q[0]))                     # canonical, whatever words the coefficients were


def test_quotient_grid_indexes_the_polynomial(engine):
    rng = random.Random(0xA1)
    check_quotient(engine, [rand_poly(rng, CH + 1) for _ in range(5)], [rng.randrange(R) for _ in range(5)])


def test_quotient_crosses_a_tile_of_the_carry_level(engine):
    """The carry level has no capacity: a block walks the chunk totals in tiles of 256 chunks and hands the running carry on.  256 chunks
    are one tile; this polynomial has 257."""
    n = BLOCK * CH + 1
    rng = random.Random(0xA2)
    words = np.frombuffer(rng.randbytes(32 * n), dtype=np.uint64).reshape(1, n, 4).copy()      # any 256-bit words
    z = rng.randrange(R)
    q, y = engine.kzg_quotient(words, M.limbs([z]))
    wq, wy = M.quotient(M.ints(words[0]), z)
    assert np.array_equal(y, M.limbs([wy])) and np.array_equal(q[0], M.limbs(wq))


def test_quotient_edge_points(engine):
    rng = random.Random(0xA3)
    zs = [0, 1, R - 1, R, R + 1, TOP, rng.randrange(R)]
    for n in (L + 1, 2 * CH + 1):                               # one launch; totals, carry and the chunks again
        check_quotient(engine, [rand_poly(rng, n) for _ in zs], zs)


def test_quotient_either_output_alone(engine):
    rng = random.Random(0xA4)
    for n in (65, CH + 1):
        polys, zs = [rand_poly(rng, n) for _ in range(3)], [rng.randrange(R) for _ in range(3)]
        q, y = check_quotient(engine, polys, zs)
        q1, none = engine.kzg_quotient(M.poly_words(polys), M.limbs(zs), want_y=False)
        none2, y1 = engine.kzg_quotient(M.poly_words(polys), M.limbs(zs), want_q=False)
        assert none is None and none2 is None and np.array_equal(q1, q) and np.array_equal(y1, y)


def test_quotient_argument_errors_and_empty_batch(engine):
    lib = engine.lib
    fill = np.full((4, 8), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    dc, dz, dq, dy = (engine.to_device(fill) for _ in range(4))
    call = lambda *a: lib.sylow_hip_kzg_quotient_batch(*a, engine.stream)
    assert call(dc.ptr, 8, 1, dz.ptr, None, None) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    assert call(dc.ptr, 0, 1, dz.ptr, dq.ptr, dy.ptr) == E_ARG
    assert call(None, 8, 1, dz.ptr, dq.ptr, dy.ptr) == E_ARG and call(dc.ptr, 8, 1, None, dq.ptr, dy.ptr) == E_ARG
    assert call(dc.ptr, 8, 0, dz.ptr, dq.ptr, dy.ptr) == 0      # m = 0: OK, nothing launched
    engine.sync()
    assert np.array_equal(dq.download(), fill) and np.array_equal(dy.download(), fill)
    ds, do, doi = engine.to_device(np.zeros((8, 8), dtype=np.uint64)), engine.to_device(fill), engine.to_device(np.full(8, 7, np.uint8))
    commit = lambda *a: lib.sylow_hip_kzg_commit_batch(*a, engine.stream)
    assert commit(ds.ptr, dc.ptr, 0, 1, do.ptr, doi.ptr) == E_ARG and commit(None, dc.ptr, 8, 1, do.ptr, doi.ptr) == E_ARG
    assert commit(ds.ptr, dc.ptr, 8, 1, None, doi.ptr) == E_ARG and commit(ds.ptr, dc.ptr, 8, 1, do.ptr, None) == E_ARG
    assert lib.sylow_hip_kzg_commit_batch_tuned(ds.ptr, dc.ptr, 8, 1, 3, -1, do.ptr, doi.ptr, engine.stream) == E_ARG     # window 3
    assert commit(ds.ptr, dc.ptr, 8, 0, do.ptr, doi.ptr) == 0
    opn = lambda *a: lib.sylow_hip_kzg_open_batch(*a, engine.stream)
    assert opn(ds.ptr, dc.ptr, 0, 1, dz.ptr, dy.ptr, do.ptr, doi.ptr) == E_ARG and opn(ds.ptr, dc.ptr, 8, 1, dz.ptr, None, do.ptr, doi.ptr) == E_ARG
    assert opn(ds.ptr, dc.ptr, 8, 1, None, dy.ptr, do.ptr, doi.ptr) == E_ARG and opn(ds.ptr, dc.ptr, 8, 0, dz.ptr, dy.ptr, do.ptr, doi.ptr) == 0
    engine.sync()
    assert np.array_equal(do.download(), fill) and (doi.download() == 7).all() and np.array_equal(dy.download(), fill)


# ---- the commitment ----------------------------------------------------------------------------------------------------------------
def check_commit(engine, srs, polys, **kw):
    n = len(polys[0])
    xy, inf = engine.kzg_commit(srs[:n], M.poly_words(polys), **kw)
    wxy, winf = M.expected_commit(polys, TAU)
    assert np.array_equal(inf, winf) and np.array_equal(xy, wxy), (len(polys), n, kw)
    return xy, inf


@pytest.mark.parametrize("m,n", [(1, 1), (1, 2), (7, 5), (3, 257), (64, 16)])
def test_commit_short_route(engine, srs, m, n):
    rng = random.Random(0xB0 + m + n)
    check_commit(engine, srs, [rand_poly(rng, n) for _ in range(m)])


def test_commit_bucket_route_and_both_routes_agree(engine, srs):
    rng = random.Random(0xB1)
    polys = [rand_poly(rng, 300) for _ in range(3)]
    bucket = check_commit(engine, srs, polys, min_len=1)
    windowed = check_commit(engine, srs, polys, window=6, min_len=0)
    short = check_commit(engine, srs, polys)
    for a, b in zip(bucket + windowed, short + short):
        assert np.array_equal(a, b)


def test_commit_identity_cases(engine, srs):
    rng = random.Random(0xB2)
    n = 33
    g = [rng.randrange(R) for _ in range(n - 1)]
    through_tau = [(-TAU * g[0]) % R] + [(g[k - 1] - TAU * g[k]) % R for k in range(1, n - 1)] + [g[n - 2]]      # (X - tau) g(X): f(tau) = 0
    assert M.evaluate(through_tau, TAU) == 0 and all(through_tau)
    polys = [[0] * n, through_tau, [R] * n, [R, 0, R] + [0] * (n - 3), rand_poly(rng, n)]
    for kw in ({}, {"min_len": 1}):
        xy, inf = check_commit(engine, srs, polys, **kw)
        assert list(inf) == [1, 1, 1, 1, 0] and all(np.array_equal(xy[j], IDENTITY) for j in range(4))


def test_commit_in_chunks_under_a_scratch_limit(engine, srs):
    rng = random.Random(0xB3)
    m, n = 64, 16
    polys = [rand_poly(rng, n) for _ in range(m)]
    whole = check_commit(engine, srs, polys)
    try:
        engine.set_scratch_limit(10 * n * K["KZG_SHORT_BYTES_PER_TERM"])      # the plan holds 10 of the 64 polynomials per chunk: 7 chunks, the last of 4
        chunked = check_commit(engine, srs, polys)
        engine.set_scratch_limit(n * K["KZG_SHORT_BYTES_PER_TERM"] - 1)       # not even one fits: each through sylow_hip_g1_msm
        each = check_commit(engine, srs, polys)
    finally:
        engine.set_scratch_limit(0)
    for a, b, c in zip(whole, chunked, each):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_commit_in_short_chunks_of_polynomials_longer_than_one_fold(engine, srs):
    """17 coefficients, one more than a lane of the segmented sum folds, so the sum runs in two stages and takes its words of the lease; a
    limit that holds two of the five polynomials, so the chunks are 2, 2 and a last one of 1 and the sums pass through scratch: every region
    of the short route's lease is in use."""
    rng = random.Random(0xB4)
    m, n = 5, 17
    polys = [rand_poly(rng, n) for _ in range(m)]
    whole = check_commit(engine, srs, polys)
    try:
        engine.set_scratch_limit(2 * n * K["KZG_SHORT_BYTES_PER_TERM"])
        chunked = check_commit(engine, srs, polys)
    finally:
        engine.set_scratch_limit(0)
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)


# ---- the opening -------------------------------------------------------------------------------------------------------------------
def check_open(engine, srs, polys, zs):
    n = len(polys[0])
    y, pi, pi_inf = engine.kzg_open(srs[:n], M.poly_words(polys), M.limbs(zs))
    wy, wpi, winf = M.expected_open(polys, zs, TAU)
    assert np.array_equal(y, M.limbs(wy)) and np.array_equal(pi_inf, winf) and np.array_equal(pi, wpi), (len(polys), n)
    return y, pi, pi_inf


@pytest.mark.parametrize("m,n", [(1, 2), (4, CH + 1), (16, 33)])
def test_open_matches_the_oracle(engine, srs, m, n):
    rng = random.Random(0xC0 + m)
    check_open(engine, srs, [rand_poly(rng, n) for _ in range(m)], [rng.randrange(R) for _ in range(m)])


def test_open_constant_polynomial_and_z_equal_tau(engine, srs):
    rng = random.Random(0xC1)
    n = 17
    polys = [[rng.randrange(1, R)] + [0] * (n - 1), [R + 5] + [R] * (n - 1), rand_poly(rng, n), rand_poly(rng, n)]
    y, pi, pi_inf = check_open(engine, srs, polys, [rng.randrange(R), TOP, TAU, TAU + R])
    assert list(pi_inf) == [1, 1, 0, 0] and np.array_equal(pi[0], IDENTITY) and np.array_equal(pi[1], IDENTITY)
    assert M.ints(y)[:2] == [polys[0][0], 5] and np.array_equal(y[2:], M.limbs([M.evaluate(f, TAU) for f in polys[2:]]))


def test_round_trip_through_the_verifier(engine, srs):
    import groth16_model as G
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0xC2)
    m, n = 12, 40
    prover = api.KzgProver(api.G1Affine(srs[:n]))
    verifier = api.KzgVerifier(api.G2Affine(G.g2_gen_mul([TAU])[0]))
    polys = [rand_poly(rng, n) for _ in range(m - 2)] + [[7] + [0] * (n - 1), [0] * n]      # a constant and the zero polynomial among them
    zs = [rng.randrange(R) for _ in range(m - 1)] + [TOP]
    c = prover.commit(polys)
    y, pi = prover.open(polys, zs)
    assert list(c.infinity) == [0] * (m - 1) + [1] and list(pi.infinity) == [0] * (m - 2) + [1, 1]
    assert verifier.verify((c, zs, y, pi)).all()
    assert verifier.verify_weighted((c, zs, y, pi), [rng.randrange(1, 1 << 128) for _ in range(m)])
    bad = [(v + (j == 3)) % R for j, v in enumerate(M.ints(y))]
    ok = verifier.verify((c, zs, bad, pi))
    assert list(ok) == [j != 3 for j in range(m)]
    assert not verifier.verify_weighted((c, zs, bad, pi), [rng.randrange(1, 1 << 128) for _ in range(m)])
    # words in, words out: the [m, len, 4] form of polys gives the same commitment
    assert (prover.commit(M.poly_words(polys)) == c).all()
