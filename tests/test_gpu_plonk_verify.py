"""GPU: the batched PLONK verifier -- sylow_pverify_scalars_batch(_tuned), sylow_pverify_fold_batch, sylow_pverify_verify_batch and
sylow_pverify_batch_verify_weighted (plonk_verify.hip) -- against the integer model of tests/plonk_verify_model.py.  The scalars are formulas
in their inputs, so they run word for word on RANDOM full-range 256-bit words (the mod-r rule) at log_n = 1, 3, 5, W = 2, 3, 32, log_e = 0,
2, n_pub = 0, 1, n, and at m = 1, 3 and 257 (one past a block of 256 lanes), pinned to one block as well, with zeta inside the domain, zeta
= 1 + r and v = u = 0.  The fold equals g1_lincomb over the model's literal terms, points and flags, also under a scratch limit that holds
exactly one proof.  Then five proofs made BY THE LIBRARY'S OWN PROVER (permutation -> quotient -> PlonkOpening.open, commitments by
KzgProver.commit): all five verify, four are then broken in four different places, the flags are the same on the three routes of the KZG
verifier and equal kzg_verify on the fold's rows, and the weighted form agrees with the pairing product over the model's two literal pairs."""
import random

import numpy as np
import pytest

import groth16_model as G
import kzg_model as K
import kzg_prove_model as M
import ntt_model as T
import plonk_quotient_model as Q
import plonk_verify_model as V
from groth16_model import ints, limbs

pytestmark = pytest.mark.gpu
R = V.R
TOP = (1 << 256) - 1
BLOCK = 256                      # the lanes of a block of k_pv_scalars (plonk_verify_plan.hpp: PV_BLOCK)
SCRATCH_FOR_ONE = 3000           # bytes: one proof of the fold at W = 3, E = 4, n_pub = 3 and not two (checked below)


def words(rows):
    """nested lists of ints [..][n] -> [.., n, 4] words"""
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


def wide(rng, *shape):
    """random full-range 256-bit integers"""
    if len(shape) == 1:
        return [rng.getrandbits(256) for _ in range(shape[0])]
    return [wide(rng, *shape[1:]) for _ in range(shape[0])]


def scalar_case(rng, log_n, W, n_pub, m):
    c = {"evals": wide(rng, m, 2 * W + 1), "pub": wide(rng, m, n_pub), "shifts": wide(rng, W)}
    for k in V.CHALLENGES:
        c[k] = wide(rng, m)
    return c


def model_scalars(c, log_n, log_e):
    m = len(c["zeta"])
    out = [V.scalars(c["evals"][i], c["pub"][i], c["shifts"], *(c[k][i] for k in V.CHALLENGES), log_n, log_e) for i in range(m)]
    return words([o[0] for o in out]), limbs([o[1] for o in out]), [o[2] for o in out]


def run_scalars(engine, c, log_n, log_e, **pins):
    pub = words(c["pub"]) if c["pub"] and c["pub"][0] else None
    return engine.plonk_verify_scalars(words(c["evals"]), pub, limbs(c["shifts"]), *(limbs(c[k]) for k in V.CHALLENGES), log_n, log_e, **pins)


@pytest.mark.parametrize("W", [2, 3, 32])
@pytest.mark.parametrize("log_n", [1, 3, 5])
def test_the_scalars_word_for_word_against_the_model(engine, log_n, W):
    m = 3
    for log_e in (0, 2):
        for n_pub in (0, 1, 1 << log_n):
            c = scalar_case(random.Random(0xE100 + 4096 * log_n + 64 * W + 8 * log_e + n_pub), log_n, W, n_pub, m)
            assert max(c["zeta"]) >= R and max(max(r) for r in c["evals"]) >= R, "full-range words: the mod-r rule"
            want_k, want_y, want_s = model_scalars(c, log_n, log_e)
            k, y, status = run_scalars(engine, c, log_n, log_e)
            assert k.shape == (m, 3 * W + (1 << log_e) + 5, 4) and np.array_equal(k, want_k), (log_n, W, log_e, n_pub)
            assert np.array_equal(y, want_y) and list(status) == want_s == [0] * m, (log_n, W, log_e, n_pub)


@pytest.mark.parametrize("m", [1, 3, BLOCK + 1])
def test_the_scalars_across_a_block_pinned_and_at_the_special_challenges(engine, m):
    log_n, W, log_e, n_pub = 3, 3, 2, 8
    c = scalar_case(random.Random(0xE200 + m), log_n, W, n_pub, m)
    c["zeta"][0] = pow(T.omega(log_n), 2, R)                  # inside the domain: status 2, the outputs by the formulas (L_2 = 0 by inv(0) = 0)
    if m >= 3:
        c["zeta"][m - 2] = 1 + R                               # zeta = 1 as a non-canonical word: L1 = 0
        c["v"][m - 1] = c["u"][m - 1] = 0
    want_k, want_y, want_s = model_scalars(c, log_n, log_e)
    assert want_s == [2] + ([0] * (m - 3) + [2, 0] if m >= 3 else []), "zeta = w_n^2 and zeta = 1 lie in the domain"
    k, y, status = run_scalars(engine, c, log_n, log_e)
    assert np.array_equal(k, want_k) and np.array_equal(y, want_y) and list(status) == want_s
    if m >= 3:
        assert not k[m - 1, 2 * W + 2:3 * W + 2].any() and not k[m - 1, -1].any(), "v = 0: the wires' scalars; u = 0: W_omega's"
    k1, y1, s1 = run_scalars(engine, c, log_n, log_e, max_blocks=1)
    assert k1.tobytes() == k.tobytes() and y1.tobytes() == y.tobytes() and list(s1) == want_s, "max_blocks = 1: the same words"


# ---- the fold ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fold_case():
    """W = 3, E = 4, n_pub = 3, m = 3: points with known logarithms, a flagged identity at [q_C] and a flagged W_omega in proof 1, both with
    garbage under the flag; random evaluations; the model's scalars"""
    rng = random.Random(0xE300)
    log_n, W, log_e, n_pub, m = 3, 3, 2, 3, 3
    P = V.proof_points(W, log_e)
    vk_xy, vk_inf = V.points([0 if c == W + 1 else rng.randrange(1, R) for c in range(V.key_points(W))])
    assert list(vk_inf) == [int(c == W + 1) for c in range(V.key_points(W))]
    vk_xy[W + 1] = K.GARBAGE
    pr_xy, pr_inf = V.points([rng.randrange(1, R) for _ in range(m * P)])
    pr_xy, pr_inf = pr_xy.reshape(m, P, 8).copy(), pr_inf.reshape(m, P).copy()
    pr_xy[1, P - 1], pr_inf[1, P - 1] = K.GARBAGE, 1
    c = scalar_case(rng, log_n, W, n_pub, m)
    return {"log_n": log_n, "W": W, "log_e": log_e, "m": m, "vk": (vk_xy, vk_inf), "proofs": (pr_xy, pr_inf), "c": c, "want": model_scalars(c, log_n, log_e)}


def run_fold(engine, f):
    c = f["c"]
    return engine.plonk_verify_fold(f["vk"], f["proofs"][0], words(c["evals"]), words(c["pub"]), limbs(c["shifts"]), *(limbs(c[k]) for k in V.CHALLENGES),
                                    f["log_n"], f["log_e"], proof_inf=f["proofs"][1])


def test_the_fold_is_g1_lincomb_over_the_literal_terms(engine, fold_case):
    f, m, W = fold_case, fold_case["m"], fold_case["W"]
    want_k, want_y, want_s = f["want"]
    (c_xy, c_inf), (pi_xy, pi_inf), y, status = run_fold(engine, f)
    xy, inf = V.literal_terms(*f["vk"], *f["proofs"])
    n_terms = V.terms(W, f["log_e"])
    assert xy.shape == (n_terms * m, 8)
    want_c = engine.g1_lincomb(xy, np.ascontiguousarray(want_k.transpose(1, 0, 2)).reshape(-1, 4), m, n_terms, p_inf=inf)
    assert np.array_equal(c_xy, want_c[0]) and np.array_equal(c_inf, want_c[1]) and not c_inf.any()
    pr_xy, pr_inf = f["proofs"]
    want_pi = engine.g1_lincomb(np.concatenate([pr_xy[:, -2], pr_xy[:, -1]]), limbs([1] * m + [u % R for u in f["c"]["u"]]), m, 2,
                                p_inf=np.concatenate([pr_inf[:, -2], pr_inf[:, -1]]))
    assert np.array_equal(pi_xy, want_pi[0]) and np.array_equal(pi_inf, want_pi[1])
    assert np.array_equal(pi_xy[1], pr_xy[1, -2]), "a flagged W_omega: pi is W_zeta"
    assert np.array_equal(y, want_y) and list(status) == want_s
    try:                                                       # one proof per chunk: the same words
        engine.set_scratch_limit(SCRATCH_FOR_ONE)
        chunked = run_fold(engine, f)
    finally:
        engine.set_scratch_limit(0)
    for got, ref in ((chunked[0], (c_xy, c_inf)), (chunked[1], (pi_xy, pi_inf))):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(chunked[2], y) and np.array_equal(chunked[3], status)


def test_the_scratch_limit_of_the_chunked_run_holds_one_proof_and_not_two():
    """the limit the test above sets, from the lease rule of plonk_verify_plan.hpp at W = 3, E = 4 (T = 18), n_pub = 3: per proof 8 n_pub words
    of denominators and inverses, 4 + 8 words a term, 2 (8 + 4) + 16 words for pi's two terms and the two results, and the flags of the chunk
    -- a byte a term and four a proof -- rounded up to a word"""
    one, two = [(k * (24 + 12 * 18 + 40) + (22 * k + 7) // 8) * 8 for k in (1, 2)]
    assert one <= SCRATCH_FOR_ONE < two, (one, two)


def test_a_row_that_holds_with_zeta_inside_the_domain_is_refused_all_the_same(engine):
    """two rows made to hold in the exponent -- random scalars, then [w_0] of each proof solved from C - y = tau pi -- the first with
    zeta = w_n^3: kzg_verify accepts both rows, the verifier's flag of the first is forced to 0, and the weighted boolean is 0 although the
    Gt value is 1, unless that proof's weight is 0 mod r"""
    rng = random.Random(0xE600)
    log_n, W, log_e, n_pub, m = 3, 3, 2, 3, 2
    K_, P = V.key_points(W), V.proof_points(W, log_e)
    c = scalar_case(rng, log_n, W, n_pub, m)
    c["zeta"][0] = pow(T.omega(log_n), 3, R)
    vk = [rng.randrange(1, R) for _ in range(K_)]
    proofs = []
    for i in range(m):
        k, y, status = V.scalars(c["evals"][i], c["pub"][i], c["shifts"], *(c[x][i] for x in V.CHALLENGES), log_n, log_e)
        assert status == (2 if i == 0 else 0) and k[K_] != 0
        pr = [0] + [rng.randrange(1, R) for _ in range(P - 1)]
        got, pi = V.row(vk, pr, k, c["u"][i])
        pr[0] = (y + V.TAU * pi - got) * pow(k[K_], R - 2, R) % R
        got, pi = V.row(vk, pr, k, c["u"][i])
        assert (got - y - V.TAU * pi) % R == 0
        proofs.append(pr)
    vk_pts, pr_xy = V.points(vk), V.points([x for pr in proofs for x in pr])[0].reshape(m, P, 8)
    tau_g2 = G.g2_gen_mul([V.TAU])[0]
    args = (vk_pts, pr_xy, words(c["evals"]), words(c["pub"]), limbs(c["shifts"])) + tuple(limbs(c[x]) for x in V.CHALLENGES)
    (c_xy, c_inf), (pi_xy, pi_inf), y, status = engine.plonk_verify_fold(*args, log_n, log_e)
    assert list(engine.kzg_verify(tau_g2, c_xy, limbs([0] * m), y, pi_xy, c_inf=c_inf, pi_inf=pi_inf)) == [1, 1] and list(status) == [2, 0]
    ok, status = engine.plonk_verify(tau_g2, *args, log_n, log_e)
    assert list(ok) == [0, 1] and list(status) == [2, 0]
    weights = [rng.getrandbits(256), rng.getrandbits(256)]
    gt, one, status = engine.plonk_batch_verify_weighted(tau_g2, *args, limbs(weights), log_n, log_e)
    assert np.array_equal(gt[0], K.ONE48) and not one and list(status) == [2, 0]
    gt, one, status = engine.plonk_batch_verify_weighted(tau_g2, *args, limbs([2 * R, weights[1]]), log_n, log_e)
    assert np.array_equal(gt[0], K.ONE48) and one and list(status) == [2, 0]


# ---- five proofs by the library's own prover -------------------------------------------------------------------------------------------------
LOG_N, LOG_E, WIRES, PUBLIC, LEN_F, PROOFS = 4, 2, 3, 3, 32, 5


@pytest.fixture(scope="module")
def five(engine):
    """permutation -> quotient -> PlonkOpening.open for five blinded witnesses of one circuit with three public inputs, every commitment by
    KzgProver.commit, the key by PlonkVerifier.key_from; then the four broken copies"""
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0xE400)
    n, E, m = 1 << LOG_N, 1 << LOG_E, PROOFS
    c = V.public_circuit(rng, LOG_N, WIRES, PUBLIC)
    srs = M.srs_points(V.TAU, LEN_F)
    ch = {k: [rng.randrange(R) for _ in range(m)] for k in V.CHALLENGES}
    perm = api.PlonkPermutation.from_mapping(LOG_N, c["shifts"], c["mapping"])
    z_vals, status = perm.grand_product(words([c["wires"]] * m), ch["beta"], ch["gamma"])
    assert list(status) == [0] * m
    base = [ints(row) for row in api.intt(words(c["wires"]))]
    w_c = [[Q.blind(row, LOG_N, [rng.randrange(R), rng.randrange(R)]) for row in base] for _ in range(m)]
    z_c = [Q.blind(ints(z), LOG_N, [rng.randrange(R) for _ in range(3)]) for z in api.intt(z_vals)]
    pi_c = [ints(api.intt(words(c["pi"])))] * m
    t, status = api.PlonkQuotient(LOG_N, c["shifts"], perm.sigma, c["selectors"], LOG_E).quotient(w_c, z_c, ch["beta"], ch["gamma"], ch["alpha"], pi=pi_c)
    assert list(status) == [0] * m
    opening = api.PlonkOpening(LOG_N, c["shifts"], perm.sigma, c["selectors"], LOG_E)
    prover = api.KzgProver(api.G1Affine(srs))
    evals, w_zeta, w_omega, status = opening.open(prover, w_c, z_c, t, ch["beta"], ch["gamma"], ch["alpha"], ch["zeta"], ch["v"], pi=pi_c)
    assert list(status) == [0] * m
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], LEN_F - a.shape[1], 4), dtype=np.uint64)], axis=1)
    c_w, c_z, c_t = prover.commit(pad(words(w_c).reshape(m * WIRES, n + 2, 4))), prover.commit(pad(words(z_c))), prover.commit(pad(t.reshape(m * E, n, 4)))
    xy = np.concatenate([c_w.xy.reshape(m, WIRES, 8), c_z.xy.reshape(m, 1, 8), c_t.xy.reshape(m, E, 8), w_zeta.xy.reshape(m, 1, 8), w_omega.xy.reshape(m, 1, 8)], axis=1)
    inf = np.concatenate([c_w.infinity.reshape(m, WIRES), c_z.infinity.reshape(m, 1), c_t.infinity.reshape(m, E), w_zeta.infinity.reshape(m, 1),
                          w_omega.infinity.reshape(m, 1)], axis=1)
    assert xy.shape == (m, V.proof_points(WIRES, LOG_E), 8) and not inf.any()
    vk = api.PlonkVerifier.key_from(prover, opening.ctable)
    tau_g2 = G.g2_gen_mul([V.TAU])[0]
    verifier = api.PlonkVerifier(LOG_N, c["shifts"], vk, api.G2Affine(tau_g2), LOG_E)
    pub = [list(c["pub"]) for _ in range(m)]
    # four of the five, each broken in another place: an evaluation, a public input, a chunk of t, W_zeta
    bad_evals, bad_pub, bad_xy = evals.copy(), [list(p) for p in pub], xy.copy()
    bad_evals[1, 1] = limbs([(ints(evals[1, 1:2])[0] + 1) % R])[0]
    bad_pub[2][PUBLIC - 1] = (bad_pub[2][PUBLIC - 1] + 1) % R
    bad_xy[3, WIRES + 1 + 1] = xy[3, WIRES + 1]               # t_1 := t_0
    bad_xy[4, -2] = xy[4, -1]                                  # W_zeta := W_omega
    return {"api": api, "c": c, "ch": ch, "vk": vk, "tau_g2": tau_g2, "verifier": verifier, "evals": evals, "pub": pub, "xy": xy, "inf": inf,
            "broken": (bad_xy, bad_evals, bad_pub)}


def challenges(f):
    return [f["ch"][k] for k in V.CHALLENGES]


def test_five_proofs_of_the_library_s_own_prover_verify_and_four_broken_ones_do_not(engine, five):
    f, api = five, five["api"]
    ok, status = f["verifier"].verify(api.G1Affine(f["xy"].reshape(-1, 8), f["inf"].reshape(-1)), f["evals"], f["pub"], *challenges(f))
    assert ok.dtype == bool and list(ok) == [True] * PROOFS and list(status) == [0] * PROOFS
    # the model agrees in the exponent on what the prover wrote: p is PI(zeta), slot 2 W of the prover's evaluations
    for i in range(PROOFS):
        assert V.pi_eval(f["pub"][i], f["ch"]["zeta"][i], LOG_N) == ints(f["evals"][i])[2 * WIRES]
    bad_xy, bad_evals, bad_pub = f["broken"]
    ok, status = f["verifier"].verify(api.G1Affine(bad_xy.reshape(-1, 8), f["inf"].reshape(-1)), bad_evals, bad_pub, *challenges(f))
    assert list(ok) == [True, False, False, False, False] and list(status) == [0] * PROOFS
    with pytest.raises(ValueError):
        api.PlonkVerifier(LOG_N, f["c"]["shifts"], api.G1Affine(f["vk"].xy[:-1], f["vk"].infinity[:-1]), api.G2Affine(f["tau_g2"]), LOG_E)


def engine_args(f, broken):
    xy, evals, pub = f["broken"] if broken else (f["xy"], f["evals"], f["pub"])
    return ((f["vk"].xy, f["vk"].infinity), xy, evals, words(pub), limbs(f["c"]["shifts"])) + tuple(limbs(c) for c in challenges(f)) + (LOG_N, LOG_E)


def test_the_flags_are_the_same_on_the_three_routes_of_the_kzg_verifier(engine, five):
    """m = 5: one wavefront per Miller loop by default; WIDE_TAIL = 0: lane quads; QUAD_MAX = 0 as well: lane pairs"""
    want = {False: [1] * PROOFS, True: [1, 0, 0, 0, 0]}
    both = lambda: {b: list(engine.plonk_verify(five["tau_g2"], *engine_args(five, b))[0]) for b in (False, True)}
    try:
        assert both() == want
        engine.set_option("WIDE_TAIL", 0)
        assert both() == want
        engine.set_option("QUAD_MAX", 0)
        assert both() == want
    finally:
        for o in ("WIDE_TAIL", "QUAD_MAX"):
            engine.set_option(o, -1)


def test_verify_is_kzg_verify_on_the_fold_s_rows_with_z_zero(engine, five):
    for broken in (False, True):
        args = engine_args(five, broken)
        (c_xy, c_inf), (pi_xy, pi_inf), y, status = engine.plonk_verify_fold(*args)
        want = engine.kzg_verify(five["tau_g2"], c_xy, limbs([0] * PROOFS), y, pi_xy, c_inf=c_inf, pi_inf=pi_inf)
        ok, status2 = engine.plonk_verify(five["tau_g2"], *args)
        assert np.array_equal(ok, want) and np.array_equal(status, status2) and list(ok) == ([1, 0, 0, 0, 0] if broken else [1] * PROOFS)
    # zeta inside the domain: the row is still written by the formulas, and ok is forced to 0 whatever kzg_verify says
    inside = list(args)
    inside[8] = limbs([pow(T.omega(LOG_N), 3, R)] + five["ch"]["zeta"][1:])
    ok, status = engine.plonk_verify(five["tau_g2"], *inside)
    assert list(status) == [2, 0, 0, 0, 0] and ok[0] == 0


def test_the_weighted_form(engine, five):
    f, rng = five, random.Random(0xE500)
    weights = [rng.getrandbits(256) for _ in range(PROOFS)]
    args = engine_args(f, False)
    gt, one, status = engine.plonk_batch_verify_weighted(f["tau_g2"], *args[:-2], limbs(weights), LOG_N, LOG_E)
    assert one and list(status) == [0] * PROOFS and np.array_equal(gt[0], K.ONE48)
    # gt_out against the pairing product over the model's two literal pairs, their points by g1_lincomb with n_jobs = 1
    bad_xy, bad_evals, bad_pub = f["broken"]
    bad_args = engine_args(f, True)
    k, y, _ = engine.plonk_verify_scalars(bad_evals, words(bad_pub), *bad_args[4:11], LOG_N, LOG_E)
    ks, ys = [ints(row) for row in k], ints(y)
    assert ks[0] == V.scalars(ints(bad_evals[0]), bad_pub[0], f["c"]["shifts"], *(f["ch"][c][0] for c in V.CHALLENGES), LOG_N, LOG_E)[0]
    shared, own, opn, s = V.weighted_scalars(ks, ys, f["ch"]["u"], weights, WIRES)
    lin = lambda xy, sc, inf=None: engine.g1_lincomb(xy, limbs(sc), 1, len(sc), p_inf=inf)
    m1_terms = np.concatenate([f["vk"].xy, bad_xy.reshape(-1, 8), limbs(G.G1_GEN).reshape(1, 8)])
    m1_flags = np.concatenate([f["vk"].infinity, f["inf"].reshape(-1), [0]]).astype(np.uint8)
    p0 = lin(m1_terms, shared + [x for row in own for x in row] + [(-s) % R], m1_flags)
    p1 = lin(np.concatenate([bad_xy[:, -2], bad_xy[:, -1]]), [(-o[0]) % R for o in opn] + [(-o[1]) % R for o in opn])
    q = np.concatenate([limbs(G.G2_GEN).reshape(1, 16), f["tau_g2"].reshape(1, 16)])
    want_gt, want_one = engine.pairing_product(np.concatenate([p0[0], p1[0]]), q, p_inf=np.concatenate([p0[1], p1[1]]), skip_infinity=True)
    gt, one, status = engine.plonk_batch_verify_weighted(f["tau_g2"], *bad_args[:-2], limbs(weights), LOG_N, LOG_E)
    assert not one and not want_one and np.array_equal(gt, want_gt) and list(status) == [0] * PROOFS
    # one broken proof: 0; its weight r, a zero written as a non-canonical word: 1 again
    mixed = list(args)
    mixed[1] = f["xy"].copy()
    mixed[1][4, -2] = f["xy"][4, -1]
    assert not engine.plonk_batch_verify_weighted(f["tau_g2"], *mixed[:-2], limbs(weights), LOG_N, LOG_E)[1]
    assert engine.plonk_batch_verify_weighted(f["tau_g2"], *mixed[:-2], limbs(weights[:4] + [R]), LOG_N, LOG_E)[1]
    verifier, api = f["verifier"], f["api"]
    pts = lambda xy: api.G1Affine(xy.reshape(-1, 8), f["inf"].reshape(-1))
    assert verifier.verify_weighted(pts(f["xy"]), f["evals"], f["pub"], *challenges(f), weights) is True
    assert verifier.verify_weighted(pts(mixed[1]), f["evals"], f["pub"], *challenges(f), weights) is False
    # zeta inside the domain makes the boolean 0 unless the proof's weight is 0 mod r
    inside = list(args)
    inside[8] = limbs([pow(T.omega(LOG_N), 3, R)] + f["ch"]["zeta"][1:])
    gt, one, status = engine.plonk_batch_verify_weighted(f["tau_g2"], *inside[:-2], limbs([0] + weights[1:]), LOG_N, LOG_E)
    assert one and list(status) == [2, 0, 0, 0, 0]
    # m = 0: the identity
    empty = ((f["vk"].xy, f["vk"].infinity), np.zeros((0, V.proof_points(WIRES, LOG_E), 8), dtype=np.uint64), np.zeros((0, 2 * WIRES + 1, 4), dtype=np.uint64), None,
             limbs(f["c"]["shifts"])) + tuple(np.zeros((0, 4), dtype=np.uint64) for _ in range(7))
    gt, one, status = engine.plonk_batch_verify_weighted(f["tau_g2"], *empty, LOG_N, LOG_E)
    assert one and np.array_equal(gt[0], K.ONE48) and len(status) == 0
