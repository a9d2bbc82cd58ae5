"""GPU: many KZG polynomials opened at one point under one folded proof -- sylow_hip_kzg_open_multi_batch, sylow_hip_kzg_open_multi_evals_batch,
sylow_hip_kzg_combine_openings_batch and sylow_hip_kzg_verify_multi_batch (kzg_multi.hip) -- against the integer model of
tests/kzg_multi_model.py.  Everything is exact: y word for word against the integer evaluation, the proofs word for word against the
oracle's q_F(tau) G1gen, against sylow_hip_kzg_open_batch of the model's F_g and against the group sums of the per-polynomial proofs the
existing calls give; the combined commitments against generator multiples of the model's discrete logarithms.  CH is the quotient's chunk
(kzg_prove_plan.hpp): CH + 1 takes its three-launch route.  The SRS (CH + 1 points) is made once per module."""
import random

import numpy as np
import pytest

import groth16_model as G
import kzg_evals_model as E
import kzg_multi_model as M
import kzg_prove_model as KP
from kzg_multi_model import R, TOP

pytestmark = pytest.mark.gpu
CH = KP.plan_constants()["KZG_POLY_CHUNK"]
SLOT = M.plan_constants()["KZGM_BYTES_PER_SLOT"]
MSM_MIN = 1 << 18                                                   # sylow_hip_g1_msm's default crossover
TAU = 0x1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA987654321 % R
IDENTITY = M.limbs([0, 1]).reshape(8)


@pytest.fixture(scope="module")
def srs():
    return KP.srs_points(TAU, CH + 1)


def rand_poly(rng, n):
    f = [rng.randrange(R) for _ in range(n)]
    for i, w in enumerate(M.EDGE_WORDS):
        if 2 * i < n:
            f[(i * 37) % n if i % 2 else n - 1 - (i * 11) % n] = w
    return f


def ragged_instance(rng, n):
    """groups {1, 0, 3, 2, 2}: a group of one, an empty group, a plain one, one whose fold is a constant and one whose fold cancels to zero"""
    sizes = [1, 0, 3, 2, 2]
    gs = M.offsets(sizes)
    polys = [rand_poly(rng, n) for _ in range(gs[-1])]
    z = [rng.randrange(1 << 256) for _ in sizes]
    gamma = [rng.randrange(1 << 256) for _ in sizes]
    gi = pow(gamma[3] % R, R - 2, R)
    polys[gs[3] + 1] = [rng.randrange(R)] + [(-c * gi) % R for c in polys[gs[3]][1:]]      # f_0 + gamma f_1 = a constant
    gamma[4] = R - 1
    polys[gs[4] + 1] = list(polys[gs[4]])                                                  # f_0 - f_0 = 0
    return polys, gs, z, gamma


def group_sum_of_proofs(engine, srs, polys, gs, z, gamma):
    """sum_j gamma_g^i pi_j from the calls that were there before: one sylow_hip_kzg_open_batch over all m polynomials, then per group a
    sylow_hip_g1_scalar_mul_batch and a sylow_hip_g1_sum_batch"""
    n = len(polys[0])
    zs = [z[g] for g, js in M.groups_of(gs) for _ in js]
    _, pi, pi_inf = engine.kzg_open(srs[:n], KP.poly_words(polys), M.limbs(zs))
    pw = M.powers(gamma, gs)
    out, flags = [], []
    for g, js in M.groups_of(gs):
        if not len(js):
            out.append(IDENTITY)
            flags.append(1)
            continue
        xy, inf = engine.g1_scalar_mul(pi[js.start:js.stop], M.limbs([pw[j] for j in js]), pi_inf[js.start:js.stop])
        sxy, sinf = engine.g1_sum(xy, inf)
        out.append(sxy[0])
        flags.append(int(sinf[0]))
    return np.stack(out), np.array(flags, dtype=np.uint8)


@pytest.mark.parametrize("n", [1, CH, CH + 1])
def test_open_multi_against_the_model(engine, srs, n):
    rng = random.Random(0xE0 + n)
    polys, gs, z, gamma = ragged_instance(rng, n)
    wy, F, qF, yF = M.open_multi(polys, gs, z, gamma)
    y, pi, pi_inf = engine.kzg_open_multi(srs[:n], KP.poly_words(polys), gs, M.limbs(z), M.limbs(gamma))
    assert np.array_equal(y, M.limbs(wy)), "y against the integer evaluation"
    wpi, winf = M.expected_points([KP.evaluate(q, TAU) for q in qF])
    assert np.array_equal(pi_inf, winf) and np.array_equal(pi, wpi), "pi against the oracle's q_F(tau) G1gen"
    # the empty group, the constant fold and the fold that cancels give the flagged identity (at len = 1 every group does)
    assert list(pi_inf) == ([1] * 5 if n == 1 else [0, 1, 0, 1, 1]) and F[1] == [0] * n and F[4] == [0] * n and not any(F[3][1:])
    fy, fpi, fpi_inf = engine.kzg_open(srs[:n], KP.poly_words(F), M.limbs(z))
    assert np.array_equal(pi, fpi) and np.array_equal(pi_inf, fpi_inf) and np.array_equal(fy, M.limbs(yF)), "bit-equal to kzg_open_batch of F_g"
    # a group of one is then word for word kzg_open_batch of its polynomial
    oy, opi, opi_inf = engine.kzg_open(srs[:n], KP.poly_words(polys[:1]), M.limbs(z[:1]))
    assert np.array_equal(y[:1], oy) and np.array_equal(pi[:1], opi) and np.array_equal(pi_inf[:1], opi_inf)
    spi, sinf = group_sum_of_proofs(engine, srs, polys, gs, z, gamma)
    assert np.array_equal(pi_inf, sinf) and np.array_equal(pi, spi), "the group sums of the per-polynomial proofs"


def test_open_multi_at_the_bucket_route(engine):
    """One group of two polynomials at the length where the commitment of the quotient takes the bucket method.  The SRS and the expected
    proof are generator multiples made on the GPU (sylow_hip_g1_generator_mul_batch, tested on its own, as the yardstick)."""
    n = MSM_MIN
    rng = random.Random(0xE1)
    logs, t = [], 1
    for _ in range(n):
        logs.append(t)
        t = t * TAU % R
    srs_xy, srs_inf = engine.g1_generator_mul(M.limbs(logs))
    assert not srs_inf.any()
    words = np.frombuffer(rng.randbytes(2 * 32 * n), dtype=np.uint64).reshape(2, n, 4).copy()      # any 256-bit words
    polys = [M.ints(words[0]), M.ints(words[1])]
    z, gamma = [rng.randrange(1 << 256)], [rng.randrange(1 << 256)]
    wy, F, qF, yF = M.open_multi(polys, [0, 2], z, gamma)
    y, pi, pi_inf = engine.kzg_open_multi(srs_xy, words, [0, 2], M.limbs(z), M.limbs(gamma))
    want, want_inf = engine.g1_generator_mul(M.limbs([sum(q * p for q, p in zip(qF[0], logs)) % R]))
    assert np.array_equal(y, M.limbs(wy)) and not pi_inf.any() and not want_inf.any() and np.array_equal(pi, want)


@pytest.mark.parametrize("log_n", [0, 1, 3, 11])
def test_open_multi_evals_equals_the_coefficient_form(engine, srs, log_n):
    n = 1 << log_n
    rng = random.Random(0xE2 + log_n)
    sizes = [2, 0, 3, 1]
    gs = M.offsets(sizes)
    evals = [rand_poly(rng, n) for _ in range(gs[-1])]
    w = E.omega(log_n)
    z = [rng.randrange(1 << 256), 5, pow(w, 3 % n, R) + R, rng.randrange(R)]       # outside the domain; group 2 at w^k, written above r
    gamma = [rng.randrange(1 << 256) for _ in sizes]
    lag, lag_inf = engine.kzg_srs_lagrange(srs[:n])
    assert not lag_inf.any()
    y, pi, pi_inf = engine.kzg_open_multi_evals(lag, KP.poly_words(evals), gs, M.limbs(z), M.limbs(gamma))
    coeffs = engine.fr_ntt(KP.poly_words(evals), inverse=True)
    cy, cpi, cpi_inf = engine.kzg_open_multi(srs[:n], coeffs, gs, M.limbs(z), M.limbs(gamma))
    assert np.array_equal(y, cy) and np.array_equal(pi, cpi) and np.array_equal(pi_inf, cpi_inf)
    assert np.array_equal(y[gs[2]:gs[3]], M.limbs([f[3 % n] % R for f in evals[gs[2]:gs[3]]])), "z = w^k: y is the k-th value"
    assert pi_inf[1] == 1 and (log_n > 0 or pi_inf.all())


# ---- the verifier's half -------------------------------------------------------------------------------------------------------------
def commitments(logs):
    xy, inf = G.g1_gen_mul(logs)
    return KP.canonical_identity(xy, inf)


def check_combine(engine, c_logs, y, gs, gamma, c_xy, c_inf):
    cf, cf_inf, yf = engine.kzg_combine_openings(c_xy, M.limbs(y), gs, M.limbs(gamma), c_inf)
    wcf, wyf = M.combine_logs(c_logs, y, gs, gamma)
    wxy, winf = M.expected_points(wcf)
    assert np.array_equal(yf, M.limbs(wyf)) and np.array_equal(cf_inf, winf) and np.array_equal(cf, wxy)
    return cf, cf_inf, yf


def test_combine_against_the_discrete_logarithms(engine):
    rng = random.Random(0xE3)
    sizes = [0, 3, 1, 0, 5, 2, 2, 0]
    gs = M.offsets(sizes)
    m = gs[-1]
    logs = [rng.randrange(1, R) for _ in range(m)]
    y = [rng.randrange(1 << 256) for _ in range(m)]
    gamma = [rng.randrange(1 << 256) for _ in sizes]
    gamma[6] = 1
    logs[gs[6] + 1] = R - logs[gs[6]]                               # C + (-C): a group sum that lands on the identity
    c_xy, c_inf = commitments(logs)
    assert not c_inf.any()
    cf, cf_inf, _ = check_combine(engine, logs, y, gs, gamma, c_xy, None)       # c_inf = NULL
    assert list(cf_inf) == [1, 0, 0, 1, 0, 0, 1, 1] and np.array_equal(cf[6], IDENTITY) and np.array_equal(cf[0], IDENTITY)
    # flagged identities among the C_j, their coordinate words garbage: a flagged point adds nothing
    flagged = list(logs)
    for j in (gs[1] + 1, gs[2], gs[4] + 4):
        flagged[j] = 0
    f_xy, f_inf = commitments(flagged)
    f_xy[f_inf.astype(bool)] = M.limbs([TOP, 12345]).reshape(8)
    check_combine(engine, flagged, y, gs, gamma, f_xy, f_inf)
    # the same words on every route: chunks of whole groups under a small scratch limit (12 slots: {0, 3, 1, 0}, {5, 2}, {2, 0}), and a limit
    # under which the group of five does not fit on its own and goes through sylow_hip_g1_msm
    try:
        engine.set_scratch_limit(12 * SLOT)
        chunked = check_combine(engine, logs, y, gs, gamma, c_xy, None)
        engine.set_scratch_limit(4 * SLOT)
        through_msm = check_combine(engine, flagged, y, gs, gamma, f_xy, f_inf)
    finally:
        engine.set_scratch_limit(0)
    assert np.array_equal(chunked[0], cf) and np.array_equal(chunked[1], cf_inf) and through_msm[1][2] == 1


def test_combine_in_chunks_of_groups_longer_than_one_fold(engine):
    """Groups of 17 and 18 terms, one more than a lane of the segmented sum folds: the sum runs in two stages and takes its words of the
    chunk's lease.  Under a limit of 40 slots the groups {17, 2} are one chunk of two segments that goes through its own sums, the group of
    18 the next one: every region of a chunk's lease is in use.  The same words as under the default limit, where all three are one chunk."""
    rng = random.Random(0xE5)
    sizes = [17, 2, 18]
    gs = M.offsets(sizes)
    logs = [rng.randrange(1, R) for _ in range(gs[-1])]
    y = [rng.randrange(1 << 256) for _ in logs]
    gamma = [rng.randrange(1 << 256) for _ in sizes]
    c_xy, c_inf = commitments(logs)
    whole = check_combine(engine, logs, y, gs, gamma, c_xy, c_inf)
    try:
        engine.set_scratch_limit(40 * SLOT)
        chunked = check_combine(engine, logs, y, gs, gamma, c_xy, c_inf)
    finally:
        engine.set_scratch_limit(0)
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)


def test_round_trips_through_the_verifier(engine, srs):
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0xE4)
    n, sizes = 40, [4, 0, 1, 3]
    m = sum(sizes)
    prover = api.KzgProver(api.G1Affine(srs[:n]))
    verifier = api.KzgVerifier(api.G2Affine(G.g2_gen_mul([TAU])[0]))
    polys = [rand_poly(rng, n) for _ in range(m)]
    z = [rng.randrange(1 << 256) for _ in sizes]
    gamma = [rng.randrange(1 << 256) for _ in sizes]
    weights = [rng.randrange(1, 1 << 128) for _ in sizes]
    c = prover.commit(polys)
    y, pi = prover.open_multi(polys, sizes, z, gamma)
    assert list(pi.infinity) == [0, 1, 0, 0]
    assert verifier.verify_multi(c, y, sizes, z, gamma, pi).all()
    assert verifier.verify_multi_weighted(c, y, sizes, z, gamma, pi, weights)
    cf, yf = verifier.combine(c, y, sizes, gamma)
    assert verifier.verify((cf, z, yf, pi)).all()                  # the folded rows are rows of the existing verifier as they stand
    # one y_j altered, one C_j swapped, a wrong gamma: exactly that group's flag turns false
    bad_y = [(v + (j == 6)) % R for j, v in enumerate(M.ints(y))]
    assert list(verifier.verify_multi(c, bad_y, sizes, z, gamma, pi)) == [True, True, True, False]
    assert not verifier.verify_multi_weighted(c, bad_y, sizes, z, gamma, pi, weights)
    swapped = c.xy.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    assert list(verifier.verify_multi(api.G1Affine(swapped, c.infinity), y, sizes, z, gamma, pi)) == [False, True, True, True]
    wrong = list(gamma)
    wrong[3] = (wrong[3] + 1) % R
    assert list(verifier.verify_multi(c, y, sizes, z, wrong, pi)) == [True, True, True, False]
    wrong[3], wrong[2] = gamma[3], gamma[2] + 1                    # a group of one does not depend on its gamma: gamma^0 = 1
    assert verifier.verify_multi(c, y, sizes, z, wrong, pi).all()
    # evaluation form under the Lagrange SRS of the same tau, through the same verifier
    n2 = 32
    ev = prover_evals = api.KzgProver(api.G1Affine(srs[:n2])).eval_prover()
    evals = [rand_poly(rng, n2) for _ in range(m)]
    z[0] = pow(E.omega(5), 7, R)                                    # the first group inside the domain
    y2, pi2 = ev.open_multi(evals, sizes, z, gamma)
    assert verifier.verify_multi(prover_evals.commit(evals), y2, sizes, z, gamma, pi2).all()
