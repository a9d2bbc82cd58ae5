"""GPU: the batched transform over Fr -- sylow_hip_fr_ntt_batch(_tuned) (ntt.hip) -- and sylow_hip_kzg_commit_evals_batch against the integer
model of tests/ntt_model.py.  Everything is exact: word for word against the radix-2 recursion (which tests/test_ntt_model.py ties to the
O(n^2) definition and to the kernel's pass decomposition), against pow() at sampled outputs of the large transform, against the library's
own polynomial evaluation, and against the oracle's generator multiples for the commitments.  T is the default number of stages of a pass,
read from ntt_plan.hpp; inputs and references are made once per (size, seed)."""
import ctypes
import functools
import random

import numpy as np
import pytest

import kzg_prove_model as KM
import ntt_model as N
from kzg_prove_model import P, TOP
from ntt_model import R

pytestmark = pytest.mark.gpu
E_ARG = -2
K = N.plan_constants()
T, S_MAX = K["NTT_STAGES_DEFAULT"], K["NTT_STAGES_MAX"]
EDGE_WORDS = [0, 1, R - 1, R, R + 1, P, TOP]
TAU = 0x1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA987654321 % R
IDENTITY = KM.limbs([0, 1]).reshape(8)
SENTINEL = 0x5A5A5A5A5A5A5A5A


@functools.lru_cache(maxsize=None)
def array(log_n, seed=0):
    """2^log_n values below r with the edge words at both ends (as many as fit)"""
    rng = random.Random(0x4E77 + 64 * seed + log_n)
    n = 1 << log_n
    a = [rng.randrange(R) for _ in range(n)]
    for i, w in enumerate(EDGE_WORDS):
        if i < n:
            a[i] = w
        if n >= 2 * len(EDGE_WORDS):
            a[n - 1 - i] = EDGE_WORDS[len(EDGE_WORDS) - 1 - i]
    return tuple(a)


@functools.lru_cache(maxsize=None)
def reference(log_n, seed=0, inverse=False, shift=None):
    return KM.limbs(N.ntt_radix2(list(array(log_n, seed)), log_n, inverse, shift))


def words(a):
    return KM.limbs(list(a))


def shift_words(g):
    return None if g is None else KM.limbs([g])[0]


def run(engine, log_n, seeds=(0,), inverse=False, shift=None, stages=-1):
    got = engine.fr_ntt(np.stack([words(array(log_n, s)) for s in seeds]), inverse=inverse, shift=shift_words(shift), stages=stages)
    for j, s in enumerate(seeds):
        want = reference(log_n, s, inverse, shift)
        assert np.array_equal(got[j], want), f"log_n {log_n} array {j} stages {stages}: {int((got[j] != want).any(axis=1).sum())} of {1 << log_n} values differ"
    return got


# ---- the default plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", sorted({0, 1, 2, 3, 5, 6, 7, T - 1, T, T + 1, T + 2}))
def test_default_plan_one_array(engine, log_n):
    got = run(engine, log_n)
    assert all(v < R for v in KM.ints(got[0]))                  # canonical, whatever words came in (the edge words are among them)


@pytest.mark.parametrize("log_n", [1, 3, T, T + 1])
def test_probes(engine, log_n):
    n, w = 1 << log_n, N.omega(log_n)
    delta0, delta1 = [1] + [0] * (n - 1), [0, 1] + [0] * (n - 2)
    got = engine.fr_ntt(np.stack([words(delta0), words(delta1), words([1] * n), words([0] * n), words([R] * n)]))
    assert np.array_equal(got[0], words([1] * n)), "delta at 0 -> all ones"
    powers = [1]
    for _ in range(n - 1):
        powers.append(powers[-1] * w % R)
    assert np.array_equal(got[1], words(powers)), "delta at 1 -> w^i: the root and the natural order"
    assert np.array_equal(got[2], words([n] + [0] * (n - 1))), "all ones -> n at index 0"
    assert not got[3].any() and not got[4].any(), "the zero array (as 0 and as r)"


# the stages the issue names, and beside them the deepest pass the tile admits (one group per tile) with the one below it
PINNED = sorted({(s, min(l, 13)) for s in (1, 2, 3, T - 1, S_MAX - 1, S_MAX) for l in (1, s, s + 1, 2 * s, 2 * s + 1, 3 * s + 1)})


@pytest.mark.parametrize("stages,log_n", PINNED)
def test_pinned_stages(engine, stages, log_n):
    """one to many passes and the uneven last pass: the model's values, and bit-equal to the default plan"""
    pinned = run(engine, log_n, stages=stages)
    assert np.array_equal(pinned, engine.fr_ntt(words(array(log_n))[None]))
    inv = run(engine, log_n, inverse=True, stages=stages)
    assert np.array_equal(inv, engine.fr_ntt(words(array(log_n))[None], inverse=True))


@pytest.mark.parametrize("m,log_n", [(5, T + 1), (3, 3)])
def test_batches_index_the_array(engine, m, log_n):
    run(engine, log_n, seeds=tuple(range(m)))
    run(engine, log_n, seeds=tuple(range(m)), inverse=True)


@pytest.mark.parametrize("log_n", [4, T + 1])
def test_edge_words_at_both_ends(engine, log_n):
    a = array(log_n)
    assert list(a[:7]) == EDGE_WORDS and list(a[-7:]) == EDGE_WORDS
    for inverse in (False, True):
        got = run(engine, log_n, inverse=inverse)
        assert all(v < R for v in KM.ints(got[0]))


# ---- the inverse ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 2, 5])
def test_inverse_against_the_definition(engine, log_n):
    a = list(array(log_n))
    got = engine.fr_ntt(words(a), inverse=True)
    assert np.array_equal(got, words(N.ntt_direct(a, log_n, inverse=True)))
    got = engine.fr_ntt(words(a), inverse=True, shift=shift_words(5))
    assert np.array_equal(got, words(N.ntt_direct(a, log_n, inverse=True, shift=5)))


@pytest.mark.parametrize("log_n", [3, T, T + 1])
def test_round_trips(engine, log_n):
    a = words(array(log_n))
    canonical = words([v % R for v in array(log_n)])
    assert np.array_equal(engine.fr_ntt(engine.fr_ntt(a), inverse=True), canonical), "intt(ntt(a)) == a mod r"
    assert np.array_equal(engine.fr_ntt(engine.fr_ntt(a, inverse=True)), canonical), "ntt(intt(a)) == a mod r"


# ---- the coset shift -----------------------------------------------------------------------------------------------------------------
SHIFTS = [1, 5, R - 1, R, R + 1, TOP, 0x2B5C7E1F00D4A6C3F19E8D7B6A5C4E3D2F1A0B9C8D7E6F5A4B3C2D1E0F9A8B7C]


@pytest.mark.parametrize("log_n", [3, T + 1])
def test_shifts(engine, log_n):
    a = words(array(log_n))
    canonical = words([v % R for v in array(log_n)])
    for g in SHIFTS:
        fwd = run(engine, log_n, shift=g)[0]
        if g % R:
            assert np.array_equal(engine.fr_ntt(fwd, inverse=True, shift=shift_words(g)), canonical), hex(g)
            run(engine, log_n, inverse=True, shift=g)
    # g = 0 mod r: g^-1 is inv(0) = 0, so only k = 0 survives: out_0 = n^-1 sum_i a_i
    for g in (0, R):
        got = engine.fr_ntt(a, inverse=True, shift=shift_words(g))
        want = [N.n_inverse(log_n) * sum(array(log_n)) % R] + [0] * ((1 << log_n) - 1)
        assert np.array_equal(got, words(want)) and np.array_equal(got, reference(log_n, 0, True, g))


# ---- one large transform on the default plan -----------------------------------------------------------------------------------------
LARGE = min(2 * T + 1, 21)
LARGE_SIZES = sorted({LARGE, 2 * S_MAX})                        # and one size at which even the deepest pass would run more than once


def raw_ntt(engine, din, log_n, m, inverse):
    dout = engine.empty((m, 4, 1 << log_n))
    engine._call("sylow_hip_fr_ntt_batch", din.ptr, log_n, m, int(inverse), None, dout.ptr)
    return dout


@pytest.fixture(scope="module", params=LARGE_SIZES)
def large(engine, request):
    """(log_n, input [4, n] canonical words, its device copy [1][4][n], the device result, the result's words [4, n])"""
    log_n = request.param
    n = 1 << log_n
    rng = np.random.default_rng(0x4E7721)
    a = rng.integers(0, 1 << 64, size=(4, n), dtype=np.uint64)
    a[3] &= np.uint64((1 << 61) - 1)                             # below 2^253 < r: canonical without a Python conversion
    din = engine.to_device(a[None])
    dout = raw_ntt(engine, din, log_n, 1, False)
    return log_n, a, din, dout, dout.download()[0]


def test_large_round_trip(engine, large):
    log_n, a, _, dout, _ = large
    back = raw_ntt(engine, dout, log_n, 1, True).download()[0]
    assert np.array_equal(back, a)


@pytest.mark.parametrize("log_n", LARGE_SIZES)
def test_large_sparse_input_at_sampled_outputs(engine, log_n):
    n, w = 1 << log_n, N.omega(log_n)
    rng = random.Random(0x4E7722)
    at = [0, 1, n // 2, n - 1, rng.randrange(2, n // 2)]
    coeff = {k: rng.randrange(1, R) for k in at}
    a = np.zeros((4, n), dtype=np.uint64)
    for k, c in coeff.items():
        a[:, k] = KM.limbs([c])[0]
    out = raw_ntt(engine, engine.to_device(a[None]), log_n, 1, False).download()[0]
    idx = [0, 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(4096)]
    want = [sum(c * pow(w, i * k, R) for k, c in coeff.items()) % R for i in idx]
    assert np.array_equal(np.ascontiguousarray(out[:, idx].T), KM.limbs(want))


def test_large_dense_output_against_polynomial_evaluation(engine, large):
    """out_i = a(w^i): the quotient kernels' evaluation (want_q = False) is an independent route on the GPU, pinned to its own model"""
    log_n, _, din, _, out = large
    n, w = 1 << log_n, N.omega(log_n)
    rng = random.Random(0x4E7723)
    for i in [0, 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(4)]:
        dz, dy = engine.to_device_soa(KM.limbs([pow(w, i, R)]), 4), engine.empty((4, 1))
        engine._call("sylow_hip_kzg_quotient_batch", din.ptr, n, 1, dz.ptr, None, dy.ptr)
        assert np.array_equal(engine.from_device_soa(dy)[0], out[:, i]), i


# ---- the transform at work -----------------------------------------------------------------------------------------------------------
def test_convolution(engine):
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0x4E7724)
    f, g = [rng.randrange(R) for _ in range(32)], [rng.randrange(R) for _ in range(32)]
    prod = [0] * 64
    for i, x in enumerate(f):
        for j, y in enumerate(g):
            prod[i + j] = (prod[i + j] + x * y) % R
    ev = api.ntt([f + [0] * 32, g + [0] * 32])
    got = api.intt(engine.fr_mul(ev[0], ev[1]))
    assert np.array_equal(got, words(prod))


def test_argument_errors_overlap_and_empty_batch(engine):
    lib = engine.lib
    n, log_n = 8, 3
    fill = np.full((2, 4, n), SENTINEL, dtype=np.uint64)            # two arrays' worth: the halves are adjacent, not overlapping
    din, dout, dsh = engine.to_device(fill), engine.to_device(fill), engine.to_device(np.array([5, 0, 0, 0], dtype=np.uint64))
    plain = lambda *a: lib.sylow_hip_fr_ntt_batch(*a, engine.stream)
    tuned = lambda *a: lib.sylow_hip_fr_ntt_batch_tuned(*a, engine.stream)
    assert plain(None, log_n, 1, 0, None, dout.ptr) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    assert plain(din.ptr, log_n, 1, 0, None, None) == E_ARG
    assert plain(din.ptr, 29, 1, 0, None, dout.ptr) == E_ARG and plain(din.ptr, -1, 1, 0, None, dout.ptr) == E_ARG
    assert plain(din.ptr, log_n, 1, 2, None, dout.ptr) == E_ARG and plain(din.ptr, log_n, 1, -1, None, dout.ptr) == E_ARG
    assert tuned(din.ptr, log_n, 1, 0, None, 0, dout.ptr) == E_ARG and tuned(din.ptr, log_n, 1, 0, None, S_MAX + 1, dout.ptr) == E_ARG
    half = 32 * n
    for off in (0, 32, half - 8, -(half - 8)):                       # out inside in's byte range, from either side
        base = din.ptr + half if off < 0 else din.ptr
        assert plain(base, log_n, 1, 0, None, base + off) == E_ARG, off
    assert plain(din.ptr, log_n, 2, 0, None, din.ptr + half) == E_ARG   # two arrays: the second half is inside the range
    assert plain(din.ptr, log_n, 0, 0, None, dout.ptr) == 0 and plain(None, log_n, 0, 1, dsh.ptr, None) == 0      # m = 0: OK, nothing launched
    engine.sync()
    assert np.array_equal(dout.download(), fill) and np.array_equal(din.download(), fill), "nothing written"
    # adjacent halves of one allocation do not overlap: the call runs (the sentinel words mod r, transformed)
    assert plain(din.ptr, log_n, 1, 0, None, din.ptr + half) == 0
    assert tuned(din.ptr, log_n, 1, 0, dsh.ptr, S_MAX, dout.ptr) == 0 and tuned(din.ptr, log_n, 1, 1, dsh.ptr, 1, dout.ptr + half) == 0
    engine.sync()
    v = int.from_bytes(np.full(4, SENTINEL, dtype=np.uint64).tobytes(), "little")
    got = din.download()
    assert np.array_equal(got[0], fill[0]) and np.array_equal(np.ascontiguousarray(got[1].T), words(N.ntt_radix2([v] * n, log_n)))
    got = dout.download()
    assert np.array_equal(np.ascontiguousarray(got[0].T), words(N.ntt_radix2([v] * n, log_n, False, 5)))
    assert np.array_equal(np.ascontiguousarray(got[1].T), words(N.ntt_radix2([v] * n, log_n, True, 5)))
    # commit_evals
    ds, do, doi = engine.to_device(np.zeros((8, n), dtype=np.uint64)), engine.to_device(fill[0]), engine.to_device(np.full(8, 7, np.uint8))
    commit = lambda *a: lib.sylow_hip_kzg_commit_evals_batch(*a, engine.stream)
    assert commit(ds.ptr, din.ptr, 29, 1, do.ptr, doi.ptr) == E_ARG and commit(ds.ptr, din.ptr, -1, 1, do.ptr, doi.ptr) == E_ARG
    assert commit(None, din.ptr, log_n, 1, do.ptr, doi.ptr) == E_ARG and commit(ds.ptr, None, log_n, 1, do.ptr, doi.ptr) == E_ARG
    assert commit(ds.ptr, din.ptr, log_n, 1, None, doi.ptr) == E_ARG and commit(ds.ptr, din.ptr, log_n, 1, do.ptr, None) == E_ARG
    assert commit(ds.ptr, din.ptr, log_n, 0, do.ptr, doi.ptr) == 0
    engine.sync()
    assert np.array_equal(do.download(), fill[0]) and (doi.download() == 7).all()


def test_short_buffer_is_refused_before_the_launch(engine):
    import sylow_amd
    din, dout = engine.empty((1, 4, 16)), engine.empty((1, 4, 8))
    with pytest.raises(sylow_amd._lib.SylowHipError, match="out holds"):
        engine._call("sylow_hip_fr_ntt_batch", din.ptr, 4, 1, 0, None, dout.ptr)


# ---- KZG from evaluations ------------------------------------------------------------------------------------------------------------
KZG_SIZES = sorted({6} | ({T + 1} if (1 << (T + 1)) <= 4096 else set()))


@pytest.fixture(scope="module")
def srs():
    return KM.srs_points(TAU, 1 << max(KZG_SIZES))


@pytest.mark.parametrize("log_n", KZG_SIZES)
def test_kzg_commit_evals(engine, srs, log_n):
    import groth16_model as G
    from sylow_amd import api
    api.set_engine(engine)
    n, m = 1 << log_n, 3
    evals = [list(array(log_n, 10 + j)) for j in range(m - 1)] + [[0, R] * (n // 2)]      # the zero array last
    coeffs = [N.ntt_radix2(e, log_n, inverse=True) for e in evals]
    prover = api.KzgProver(api.G1Affine(srs[:n]))
    c = prover.commit_evals(evals)
    from_coeffs = prover.commit(api.intt(evals))
    assert np.array_equal(c.xy, from_coeffs.xy) and np.array_equal(c.infinity, from_coeffs.infinity), "commit_evals == commit(intt(evals))"
    wxy, winf = KM.expected_commit(coeffs, TAU)
    assert np.array_equal(c.xy, wxy) and np.array_equal(c.infinity, winf), "the oracle's f(tau) G1gen"
    assert list(c.infinity) == [0, 0, 1] and np.array_equal(c.xy[2], IDENTITY), "the zero array commits to the identity"
    assert (prover.commit_evals(KM.poly_words(evals)) == c).all()                          # words in, the same points
    # the interpolated polynomial opens at z = w^i with y = evals_i
    at = [1, n - 1, n // 2]
    zs = [pow(N.omega(log_n), i, R) for i in at]
    y, pi = prover.open(api.intt(evals), zs)
    assert np.array_equal(y, words([evals[j][i] % R for j, i in enumerate(at)]))
    verifier = api.KzgVerifier(api.G2Affine(G.g2_gen_mul([TAU])[0]))
    assert verifier.verify((c, zs, y, pi)).all()
    bad = [(v + 1) % R for v in KM.ints(y)]
    assert not verifier.verify((c, zs, bad, pi)).any()
