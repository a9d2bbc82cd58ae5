"""GPU: KZG from evaluation form -- sylow_hip_kzg_quotient_evals_batch and sylow_hip_kzg_open_evals_batch (kzg_evals.hip) -- word for word
against the integer model of tests/kzg_evals_model.py at small sizes, and at larger ones against the library's own other route to the same
words: fr_ntt_batch(inverse), kzg_quotient_batch, fr_ntt_batch(forward).  The opening runs under a Lagrange-basis SRS made from the model's
L_i(tau) through g1_scalar_mul_batch, against KzgProver under the monomial SRS of the same tau, and through KzgVerifier.  Sizes come from
kzg_evals_plan.hpp (a lane's elements L, a chunk CH = 256 L).  The SRS pair of 2^12 points is made once per module.

The bucket route of the commitment starts at 2^18 points, too long an SRS to make in a test that takes seconds: the opening's tests run the
short route, and at log_n = 12 the bucket route is PINNED through kzg_commit_batch_tuned over the same quotient values instead."""
import random

import numpy as np
import pytest

import kzg_evals_model as E
import kzg_prove_model as KP
from groth16_model import ints, limbs
from kzg_evals_model import EDGE_WORDS, R, TOP

pytestmark = pytest.mark.gpu
K = E.plan_constants()
L, BLOCK, CH = K["EVALS_LANE_ELEMS"], K["EVALS_BLOCK"], K["EVALS_CHUNK"]
TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
IDENTITY = limbs([0, 1]).reshape(8)
LOG_MAX = 12


def rand_evals(rng, n, edges=True):
    f = [rng.randrange(1 << 256) for _ in range(n)]
    if edges:
        for i, w in enumerate(EDGE_WORDS):
            if 2 * i < n:
                f[(i * 37) % n if i % 2 else n - 1 - (i * 11) % n] = w
    return f


def check_model(engine, evals, zs, ks=None):
    log_n = len(evals[0]).bit_length() - 1
    q, y = engine.kzg_quotient_evals(KP.poly_words(evals), limbs(zs))
    ks = ks or [None] * len(zs)
    want = [E.quotient(f, log_n, z, k) for f, z, k in zip(evals, zs, ks)]
    assert np.array_equal(y, limbs([w[1] for w in want])), "y"
    for j, (wq, _) in enumerate(want):
        assert np.array_equal(q[j], limbs(wq)), f"q of polynomial {j}: values {list(np.flatnonzero((q[j] != limbs(wq)).any(axis=1)))[:8]} differ"
    return q, y


def ntt_route(engine, words, z):
    """the same words by the calls the library had: interpolate, divide, evaluate"""
    q, y = engine.kzg_quotient(engine.fr_ntt(words, inverse=True), z)
    return engine.fr_ntt(q), y


# ---- against the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(8))
def test_quotient_against_the_model(engine, log_n):
    rng = random.Random(0xF0 + log_n)
    n, w = 1 << log_n, E.omega(log_n)
    k = rng.randrange(n)
    zs, ks = [rng.randrange(R), pow(w, k, R), rng.randrange(1 << 256)], [None, k, None]      # outside, inside, any word
    q, _ = check_model(engine, [rand_evals(rng, n) for _ in zs], zs, ks)
    assert all(v < R for v in ints(q.reshape(-1, 4)))          # canonical, whatever words the values were


# ---- against the transform route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("log_n", [11, 12, 13, 20])
def test_quotient_against_the_transform_route(engine, log_n, m):
    """One, two and four chunks, and 512; on the device throughout (the arrays are random words in the device layout [m][4][n]).  Of five
    rows the last has z inside the domain, in the last chunk: its repaired q_k comes from sums over every chunk."""
    rng = random.Random(0xF1 + 10 * log_n + m)
    n = 1 << log_n
    zs = [rng.randrange(1 << 256) for _ in range(m)]
    k = n - 1 - rng.randrange(L)
    if m > 1:
        zs[-1] = pow(E.omega(log_n), k, R) + R
    dev = np.frombuffer(rng.randbytes(32 * n * m), dtype=np.uint64).reshape(m, 4, n)
    de, dz = engine.to_device(dev), engine.to_device_soa(limbs(zs), 4)
    dc, dq, dqv, dy = engine.empty((m, 4, n)), engine.empty((m, 4, n)), engine.empty((m, 4, n)), engine.empty((4, m))
    engine._call("sylow_hip_fr_ntt_batch", de.ptr, log_n, m, 1, None, dc.ptr)
    engine._call("sylow_hip_kzg_quotient_batch", dc.ptr, n, m, dz.ptr, dq.ptr, dy.ptr)
    engine._call("sylow_hip_fr_ntt_batch", dq.ptr, log_n, m, 0, None, dqv.ptr)
    gq, gy = engine.empty((m, 4, n)), engine.empty((4, m))
    engine._call("sylow_hip_kzg_quotient_evals_batch", de.ptr, log_n, m, dz.ptr, gq.ptr, gy.ptr)
    want_q, got_q = dqv.download(), gq.download()
    assert np.array_equal(gy.download(), dy.download()), "y"
    assert np.array_equal(got_q, want_q), f"{int((got_q != want_q).any(axis=1).sum())} of {m * n} values differ"
    if m > 1:
        fk = int.from_bytes(dev[m - 1, :, k].tobytes(), "little") % R
        assert ints(np.ascontiguousarray(gy.download().T))[-1] == fk, "z = w^k: y = f_k"


# ---- z inside the domain -----------------------------------------------------------------------------------------------------------
def test_z_inside_the_domain(engine):
    """k at both ends of the domain, of a lane and of a chunk, z = -1 (k = n/2), z written as w^k + r, and rows outside the domain among them:
    against the model and against the transform route."""
    rng = random.Random(0xF2)
    log_n = LOG_MAX
    n, w = 1 << log_n, E.omega(log_n)
    assert n == 2 * CH
    ks = [0, 1, n // 2, n - 1, L - 1, L, CH - 1, CH, None, CH + 5 * L + 3, None]
    zs = [rng.randrange(R) if k is None else pow(w, k, R) for k in ks]
    assert zs[2] == R - 1
    zs[1] += R
    zs[6] += R
    zs[9] += 4 * R                                              # still below 2^256
    evals = [rand_evals(rng, n, edges=j % 2 == 0) for j in range(len(ks))]
    q, y = check_model(engine, evals, zs, ks)
    for j, k in enumerate(ks):
        if k is not None:
            assert ints(y[j:j + 1]) == [evals[j][k] % R]
    rq, ry = ntt_route(engine, KP.poly_words(evals), limbs(zs))
    assert np.array_equal(ry, y) and np.array_equal(rq, q)


@pytest.mark.parametrize("log_n", [1, 3, 4])
def test_every_point_of_a_small_domain(engine, log_n):
    rng = random.Random(0xF3 + log_n)
    n, w = 1 << log_n, E.omega(log_n)
    ks = list(range(n))
    check_model(engine, [rand_evals(rng, n) for _ in ks], [pow(w, k, R) + (R if k % 2 else 0) for k in ks], ks)


# ---- edge cases ----------------------------------------------------------------------------------------------------------------------
def test_edge_words_zero_point_and_constants(engine):
    rng = random.Random(0xF4)
    for log_n in (0, 5, LOG_MAX):
        n = 1 << log_n
        zs = (EDGE_WORDS if log_n <= 5 else [0, 2 * R, TOP]) + [rng.randrange(R)]      # z = 0 mod r three ways among them; z = 1 and r - 1 are in the domain
        evals = [rand_evals(rng, n) for _ in zs]
        evals[-1] = [(7 + R * (i % 3)) for i in range(n)]      # a constant polynomial, written three ways: q = 0
        q, y = check_model(engine, evals, zs)
        assert ints(y[-1:]) == [7] and not q[-1].any()
    q, y = check_model(engine, [[5], [R + 6], [TOP]], [1, 9, 0])      # log_n = 0: y = f_0 and q_0 = 0 for every z
    assert not q.any() and ints(y) == [5, 6, TOP % R]


def test_either_output_alone(engine):
    rng = random.Random(0xF5)
    for log_n in (6, LOG_MAX):
        n = 1 << log_n
        evals = [rand_evals(rng, n) for _ in range(3)]
        zs = [rng.randrange(R), pow(E.omega(log_n), n - 2, R), rng.randrange(R)]
        words, z = KP.poly_words(evals), limbs(zs)
        q, y = engine.kzg_quotient_evals(words, z)
        q1, none = engine.kzg_quotient_evals(words, z, want_y=False)
        none2, y1 = engine.kzg_quotient_evals(words, z, want_q=False)
        assert none is None and none2 is None and np.array_equal(q1, q) and np.array_equal(y1, y)
        assert np.array_equal(y, limbs([E.quotient(f, log_n, zz, k)[1] for f, zz, k in zip(evals, zs, [None, n - 2, None])]))


# ---- the opening -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def srs_pair(engine):
    """(monomial [n, 8], {log_n: Lagrange [2^log_n, 8]}) for TAU: tau^k G1gen through the fixed-base call, L_i(tau) G1gen through
    g1_scalar_mul_batch on copies of the generator"""
    n = 1 << LOG_MAX
    mono, inf = engine.g1_generator_mul(limbs(KP.srs_logs(TAU, n)))
    assert not inf.any()
    lag = {}
    for log_n in (6, LOG_MAX):
        xy, inf = engine.g1_scalar_mul(np.tile(limbs([1, 2]).reshape(1, 8), (1 << log_n, 1)), limbs(E.lagrange_at(log_n, TAU)))
        assert not inf.any()
        lag[log_n] = xy
    return mono, lag


@pytest.mark.parametrize("log_n", [6, LOG_MAX])
def test_open_evals(engine, srs_pair, log_n):
    import groth16_model as G
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0xF6 + log_n)
    n, w = 1 << log_n, E.omega(log_n)
    mono, lag = srs_pair
    by_evals, by_coeffs = api.KzgEvalProver(api.G1Affine(lag[log_n])), api.KzgProver(api.G1Affine(mono[:n]))
    evals = [rand_evals(rng, n), rand_evals(rng, n, edges=False), [R + 9] * n, rand_evals(rng, n)]      # the third is constant
    k = n - L - 1
    zs = [rng.randrange(R), pow(w, k, R) + R, rng.randrange(1 << 256), TOP]
    words = KP.poly_words(evals)
    # the commitment over the Lagrange SRS is the commitment from evaluations under the monomial one
    c = by_evals.commit(evals)
    c_mono = by_coeffs.commit_evals(evals)
    assert np.array_equal(c.xy, c_mono.xy) and np.array_equal(c.infinity, c_mono.infinity) and not c.infinity.any()
    # the opening is the opening of the interpolated coefficients
    y, pi = by_evals.open(evals, zs)
    wy, wpi = by_coeffs.open(api.intt(words), zs)
    assert np.array_equal(y, wy) and np.array_equal(pi.xy, wpi.xy) and np.array_equal(pi.infinity, wpi.infinity)
    assert ints(y)[1:3] == [evals[1][k] % R, 9]
    assert list(pi.infinity) == [0, 0, 1, 0] and np.array_equal(pi.xy[2], IDENTITY), "the identity exactly for the constant polynomial"
    assert np.array_equal(by_evals.evaluate(evals, zs), y) and np.array_equal(by_evals.quotient(words, zs)[1], y)
    verifier = api.KzgVerifier(api.G2Affine(G.g2_gen_mul([TAU])[0]))
    assert verifier.verify((c, zs, y, pi)).all()
    bad = [(v + 1) % R for v in ints(y)]
    assert not verifier.verify((c, zs, bad, pi)).any()
    if log_n == LOG_MAX:                                        # the bucket route, pinned: the same points from the same quotient values
        q, _ = by_evals.quotient(evals, zs)
        bxy, binf = engine.kzg_commit(lag[log_n], q, min_len=0)
        assert np.array_equal(bxy, pi.xy) and np.array_equal(binf, pi.infinity)
        cxy, cinf = engine.kzg_commit(lag[log_n], words, min_len=0)
        assert np.array_equal(cxy, c.xy) and np.array_equal(cinf, c.infinity)


def test_eval_prover_refuses_a_bad_srs_or_shape(engine, srs_pair):
    from sylow_amd import api
    _, lag = srs_pair
    with pytest.raises(ValueError):
        api.KzgEvalProver(api.G1Affine(lag[6][:48]))           # not a power of two
    prover = api.KzgEvalProver(api.G1Affine(lag[6]))
    with pytest.raises(ValueError):
        prover.commit([[1] * 32])
