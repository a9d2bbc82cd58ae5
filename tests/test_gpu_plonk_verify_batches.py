"""GPU: the point side of the batched PLONK verifier -- sylow_pverify_fold_batch, sylow_pverify_verify_batch and
sylow_pverify_batch_verify_weighted (plonk_verify.hip) -- past one block, one chunk and one shape, against the integer model of
tests/plonk_verify_model.py.  Every comparison is bit-exact.

The rows come from V.holding_batch: random full-range words for every scalar, random logarithms for every point but [w_0], and [w_0] solved
so that the row verifies in the exponent -- at any shape, a satisfied witness or not.  V.break_rows then breaks chosen rows in five ways.  The
points: the unsolved slots draw from a pool of 64 oracle points with known logarithms, the m solved [w_0] come from ONE g1_generator_mul
(pinned to the oracle in tests/test_gpu_groups.py; eight of them are compared with the oracle here again), and garbage words lie under every
flag.

  * m = 513, two full blocks of 256 lanes and one lane: the flags and the fold, rows 0, 255, 256, 511 and 512 broken, one of each kind, the
    last with zeta inside the domain; C and pi against g1_lincomb over the literal terms and, on the broken rows, against the oracle.
  * m = 7 under scratch limits that hold three proofs (chunks of 3, 3, 1) and two (2, 2, 2, 1): the bytes of the unchunked fold.
  * the weighted form over three blocks: ksum, s and the veto walked through them, gt_out against the ORACLE'S pairing product over the
    model's two literal pairs, and one live lane per block against the call on those three proofs alone.
  * W = 2, 3, 32, log_e = 0, 2, 3, n_pub = 0 (NULL pub), 1, n: a broken row and flagged identities at a key slot, a wire slot and a W_omega.
  * proofs written by the MODEL'S prover (V.proof_for), which shares no code and no convention with the device's, and the public layer on
    one of them."""
import random

import numpy as np
import pytest

import groth16_model as G
import kzg_model as K
import plonk_verify_model as V
from groth16_model import limbs
from test_gpu_plonk_verify import words

R = V.R
BLOCK = 256                      # the lanes of a block (plonk_verify_plan.hpp: PV_BLOCK)
LOG_N, WIRES, LOG_E, PUBLIC = 3, 3, 2, 3
BIG = 2 * BLOCK + 1              # two full blocks and one lane
BROKEN = {0: "evaluation", BLOCK - 1: "public_input", BLOCK: "t0_is_z", 2 * BLOCK - 1: "wzeta_is_womega", 2 * BLOCK: "zeta_in_domain"}
POOL = 64
CHUNKED = 7                      # proofs of the chunked fold


# ---- points ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """64 oracle points with known logarithms: (logarithms, words [64, 8], {logarithm: index})"""
    rng = random.Random(0xF000)
    logs = [rng.randrange(1, R) for _ in range(POOL)]
    xy, inf = V.points(logs)
    assert not inf.any() and len(set(logs)) == POOL
    return logs, xy, {x: i for i, x in enumerate(logs)}


@pytest.fixture(scope="module")
def tau_g2():
    return G.g2_gen_mul([V.TAU])[0]


def pooled(logs, pool):
    """(words [k, 8], flags [k]) of logarithms that are pool entries or 0: the identity is flagged, with garbage underneath"""
    _, xy, index = pool
    inf = np.array([x == 0 for x in logs], dtype=np.uint8)
    out = xy[[index[x] if x else 0 for x in logs]].copy()
    out[inf.astype(bool)] = K.GARBAGE
    return out, inf


def pooled_points(engine, b, pool):
    """the key and the proofs of a batch as words and flags: slots 1 .. P - 1 from the pool, slot 0 of all m proofs by one g1_generator_mul"""
    m, P = b["m"], V.proof_points(b["W"], b["log_e"])
    xy, inf = pooled([0 if s == 0 else x for pr in b["proofs"] for s, x in enumerate(pr)], pool)
    xy, inf = xy.reshape(m, P, 8), inf.reshape(m, P)
    w0_xy, w0_inf = engine.g1_generator_mul(limbs([pr[0] for pr in b["proofs"]]))
    xy[:, 0], inf[:, 0] = w0_xy, w0_inf
    assert not w0_inf.any()
    return {"vk": pooled(b["vk"], pool), "xy": xy, "inf": inf}


def oracle_points(b):
    """the key and the proofs of a small batch by the oracle alone; garbage under every flag"""
    m, P = b["m"], V.proof_points(b["W"], b["log_e"])
    vk_xy, vk_inf = V.points(b["vk"])
    xy, inf = V.points([x for pr in b["proofs"] for x in pr])
    vk_xy, xy = vk_xy.copy(), xy.copy()
    vk_xy[vk_inf.astype(bool)] = K.GARBAGE
    xy[inf.astype(bool)] = K.GARBAGE
    return {"vk": (vk_xy, vk_inf), "xy": xy.reshape(m, P, 8), "inf": inf.reshape(m, P).copy()}


def take(b, pts, rows):
    rows = list(rows)
    return V.take_rows(b, rows), {"vk": pts["vk"], "xy": np.ascontiguousarray(pts["xy"][rows]), "inf": np.ascontiguousarray(pts["inf"][rows])}


# ---- the calls and what the model and the oracle say of them --------------------------------------------------------------------------------
def call_args(b, pts):
    """the arguments every point-side entry point shares, up to u; NULL pub where n_pub = 0"""
    pub = words(b["pub"]) if b["n_pub"] else None
    return (pts["vk"], pts["xy"], words(b["evals"]), pub, limbs(b["shifts"])) + tuple(limbs(b[c]) for c in V.CHALLENGES)


def dims(b):
    return b["log_n"], b["log_e"]


def weighted(engine, tau_g2, b, pts, weights):
    return engine.plonk_batch_verify_weighted(tau_g2, *call_args(b, pts), limbs(weights), *dims(b), proof_inf=pts["inf"])


def oracle_gt(p0, p1, tau_g2):
    """the Gt words of e(p0 G1gen, G2gen) e(p1 G1gen, tau G2) by the oracle's scalar multiplication and pairing: neither the device's
    multi-scalar multiplication nor its pairing takes part.  A pair whose G1 side is the identity is left out, as the device leaves it out"""
    xy, inf = V.points([p0, p1])
    q = (G.g2_proj(limbs(G.G2_GEN).reshape(1, 16))[0], G.g2_proj(tau_g2)[0])
    return G.products([[(G.g1_proj(xy[j:j + 1])[0], q[j]) for j in range(2) if not inf[j]]])[0]


def check_fold(engine, b, pts, sc, oracle_rows):
    """y and status against the model; C and pi bit-identical to g1_lincomb over the literal terms under the model's scalars; and C and pi of
    `oracle_rows` against the oracle's points of the model's row"""
    m, W, n_terms = b["m"], b["W"], V.terms(b["W"], b["log_e"])
    (c_xy, c_inf), (pi_xy, pi_inf), y, status = engine.plonk_verify_fold(*call_args(b, pts), *dims(b), proof_inf=pts["inf"])
    assert np.array_equal(y, limbs([s[1] for s in sc])) and list(status) == [s[2] for s in sc]
    xy, inf = V.literal_terms(*pts["vk"], pts["xy"], pts["inf"])
    k = words([s[0] for s in sc])
    want_c = engine.g1_lincomb(xy, np.ascontiguousarray(k.transpose(1, 0, 2)).reshape(-1, 4), m, n_terms, p_inf=inf)
    assert np.array_equal(c_xy, want_c[0]) and np.array_equal(c_inf, want_c[1]) and not c_inf.any()
    want_pi = engine.g1_lincomb(np.concatenate([pts["xy"][:, -2], pts["xy"][:, -1]]), limbs([1] * m + [u % R for u in b["u"]]), m, 2,
                                p_inf=np.concatenate([pts["inf"][:, -2], pts["inf"][:, -1]]))
    assert np.array_equal(pi_xy, want_pi[0]) and np.array_equal(pi_inf, want_pi[1]) and not pi_inf.any()
    rows = [V.row(b["vk"], b["proofs"][i], sc[i][0], b["u"][i]) for i in oracle_rows]
    want_xy, want_inf = V.points([x for r in rows for x in r])
    assert not want_inf.any()
    assert np.array_equal(c_xy[oracle_rows], want_xy[0::2]) and np.array_equal(pi_xy[oracle_rows], want_xy[1::2]), "C and pi by the oracle"
    return (c_xy, c_inf), (pi_xy, pi_inf), y, status


# ---- 513 proofs: two full blocks and one lane ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(engine, pool):
    """the holding batch of 513 proofs and its copy with five rows broken, one of each kind; the model's scalars and booleans of both"""
    rng = random.Random(0xF100)
    clean = V.holding_batch(rng, LOG_N, WIRES, LOG_E, PUBLIC, BIG, pool=pool[0])
    broken = V.break_rows(clean, BROKEN)
    out = {"weights": [rng.getrandbits(256) for _ in range(BIG)]}
    for name, b in (("clean", clean), ("broken", broken)):
        sc = V.batch_scalars(b)
        out[name] = {"b": b, "pts": pooled_points(engine, b, pool), "sc": sc, "ok": V.batch_verify(b, sc)}
    assert out["clean"]["ok"] == [True] * BIG and out["broken"]["ok"] == [i not in BROKEN for i in range(BIG)]
    assert [s[2] for s in out["broken"]["sc"]] == [0] * (BIG - 1) + [2]
    # the solved [w_0] of eight proofs, the broken rows among them, by the oracle
    sample = sorted(BROKEN) + [1, BLOCK + 1, BIG - 2]
    want_xy, want_inf = V.points([broken["proofs"][i][0] for i in sample])
    assert np.array_equal(out["broken"]["pts"]["xy"][sample, 0], want_xy) and not want_inf.any()
    return out


@pytest.mark.gpu
def test_the_flags_and_the_fold_past_one_block(engine, big, tau_g2):
    """k_pv_veto, k_pv_gather and k_pv_scatter beyond their first block; row 512, the one live lane of the third block, is refused by its status
    alone"""
    for name in ("clean", "broken"):
        f = big[name]
        ok, status = engine.plonk_verify(tau_g2, *call_args(f["b"], f["pts"]), *dims(f["b"]), proof_inf=f["pts"]["inf"])
        assert [bool(x) for x in ok] == f["ok"] and list(status) == [s[2] for s in f["sc"]], name
    f = big["broken"]
    (c_xy, c_inf), (pi_xy, pi_inf), y, status = check_fold(engine, f["b"], f["pts"], f["sc"], [0, BLOCK - 1, BLOCK, 2 * BLOCK])
    # the row with zeta inside the domain holds as a KZG row: the veto alone refuses it
    ok = engine.kzg_verify(tau_g2, c_xy[-2:], limbs([0, 0]), y[-2:], pi_xy[-2:])
    assert list(ok) == [0, 1] and list(status[-2:]) == [0, 2]


@pytest.mark.gpu
def test_the_weighted_form_past_one_block(engine, big, tau_g2):
    """ksum, s and the count of vetoed proofs through three blocks of k_pv_weighted_prep and three partials a column in k_pv_join"""
    w = big["weights"]
    f = big["clean"]
    gt, one, status = weighted(engine, tau_g2, f["b"], f["pts"], w)
    assert one and np.array_equal(gt[0], K.ONE48) and list(status) == [0] * BIG
    f = big["broken"]
    p0, p1, want_one = V.batch_weighted(f["b"], w, f["sc"])
    gt, one, status = weighted(engine, tau_g2, f["b"], f["pts"], w)
    assert not one and not want_one and list(status) == [0] * (BIG - 1) + [2]
    want_gt = oracle_gt(p0, p1, tau_g2)
    assert not np.array_equal(want_gt, K.ONE48) and np.array_equal(gt[0], want_gt)
    # the four rows that fail removed by weights that are 0 mod r; the row with zeta inside the domain still live: Gt is 1, the boolean 0
    w = list(w)
    w[0], w[BLOCK - 1], w[BLOCK], w[2 * BLOCK - 1] = R, 2 * R, 0, 0
    assert w[2 * BLOCK] % R
    gt, one, status = weighted(engine, tau_g2, f["b"], f["pts"], w)
    assert np.array_equal(gt[0], K.ONE48) and not one and not V.batch_weighted(f["b"], w, f["sc"])[2]
    w[2 * BLOCK] = R
    gt, one, status = weighted(engine, tau_g2, f["b"], f["pts"], w)
    assert np.array_equal(gt[0], K.ONE48) and one and V.batch_weighted(f["b"], w, f["sc"])[2]


@pytest.mark.gpu
def test_one_live_lane_per_block_is_the_call_on_those_three_proofs(engine, big, tau_g2):
    """weights zero but at rows 255, 256 and 512: a partial sum in the wrong column or block shows here even where errors would cancel above"""
    live = [BLOCK - 1, BLOCK, 2 * BLOCK]
    w = [big["weights"][i] if i in live else 0 for i in range(BIG)]
    for name in ("broken", "clean"):
        f = big[name]
        gt, one, status = weighted(engine, tau_g2, f["b"], f["pts"], w)
        sub_b, sub_pts = take(f["b"], f["pts"], live)
        sub_gt, sub_one, sub_status = weighted(engine, tau_g2, sub_b, sub_pts, [w[i] for i in live])
        assert np.array_equal(gt, sub_gt) and one == sub_one == (name == "clean") and list(status[live]) == list(sub_status)
        assert np.array_equal(gt[0], K.ONE48) == (name == "clean")
        if name == "broken":
            p0, p1, _ = V.batch_weighted(sub_b, [w[i] for i in live], [f["sc"][i] for i in live])
            assert np.array_equal(gt[0], oracle_gt(p0, p1, tau_g2))


# ---- chunks of more than one proof with a ragged tail -----------------------------------------------------------------------------------------
def scratch_for(mc):
    """a scratch limit, in bytes, that holds mc proofs of the fold at W = 3, E = 4, n_pub = 3 and not mc + 1: halfway between the two leases"""
    return (V.fold_chunk_bytes(WIRES, LOG_E, PUBLIC, mc) + V.fold_chunk_bytes(WIRES, LOG_E, PUBLIC, mc + 1)) // 2


@pytest.mark.parametrize("mc", [2, 3])
def test_the_scratch_limits_of_the_chunked_fold_hold_mc_proofs_and_not_one_more(mc):
    """the lease rule of plonk_verify_plan.hpp (V.fold_chunk_bytes; its figures for one and two proofs are pinned in
    tests/test_plonk_verify_model.py and in tests/cpp/plonk_verify_plan_test.cpp)"""
    lease = lambda k: 8 * (k * (8 * PUBLIC + 12 * 18 + 40) + (22 * k + 7) // 8)
    assert lease(mc) == V.fold_chunk_bytes(WIRES, LOG_E, PUBLIC, mc) and lease(mc) <= scratch_for(mc) < lease(mc + 1), (lease(mc), scratch_for(mc), lease(mc + 1))
    assert 1 < mc < CHUNKED and CHUNKED % mc, "several proofs a chunk, several chunks, a ragged last one"


@pytest.mark.gpu
def test_the_fold_in_chunks_of_three_and_of_two_with_a_ragged_tail(engine, pool):
    """fold_run with 1 < mc < m: s0 > 0 together with c > 1, and a last chunk of one proof laid out inside a lease sized for mc"""
    rng = random.Random(0xF200)
    b = V.break_rows(V.holding_batch(rng, LOG_N, WIRES, LOG_E, PUBLIC, CHUNKED, pool=pool[0]), {4: "zeta_in_domain"})
    pts, sc = pooled_points(engine, b, pool), V.batch_scalars(b)
    pts["xy"][5, -1], pts["inf"][5, -1] = K.GARBAGE, 1           # a flag that has to travel with its proof: pi of proof 5 is its W_zeta
    run = lambda: engine.plonk_verify_fold(*call_args(b, pts), *dims(b), proof_inf=pts["inf"])
    (c_xy, c_inf), (pi_xy, pi_inf), y, status = whole = run()
    assert np.array_equal(y, limbs([s[1] for s in sc])) and list(status) == [0, 0, 0, 0, 2, 0, 0] and np.array_equal(pi_xy[5], pts["xy"][5, -2])
    assert len({c_xy[i].tobytes() for i in range(CHUNKED)}) == CHUNKED, "every proof has a C of its own"
    for mc in (3, 2):
        try:
            engine.set_scratch_limit(scratch_for(mc))
            chunked = run()
        finally:
            engine.set_scratch_limit(0)
        got = [chunked[0][0], chunked[0][1], chunked[1][0], chunked[1][1], chunked[2], chunked[3]]
        ref = [c_xy, c_inf, pi_xy, pi_inf, y, status]
        assert all(g.tobytes() == r.tobytes() for g, r in zip(got, ref)), mc
    assert whole[0][0].tobytes() == run()[0][0].tobytes(), "and the limit is lifted again"


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("log_n,W,log_e,n_pub,kind", [(1, 2, 0, 0, "t0_is_z"), (3, 2, 3, 8, "public_input"), (5, 32, 0, 32, "evaluation"),
                                                      (3, 3, 2, 1, "wzeta_is_womega")])
def test_the_point_side_at_other_shapes_with_flagged_points(engine, pool, tau_g2, log_n, W, log_e, n_pub, kind):
    """m = 5, row 2 broken; a flagged identity with garbage underneath at the key's [q_C], at [w_1] of row 1 and at W_omega of row 3, [w_0] of
    every row solved AFTER the logarithms of those slots were set to 0, so that rows 1 and 3 hold: the flags steer the value, not only the
    bytes.  n_pub = 0 runs with a NULL pub"""
    m, P = 5, V.proof_points(W, log_e)
    rng = random.Random(0xF300 + 64 * W + 8 * log_e + n_pub)
    clean = V.holding_batch(rng, log_n, W, log_e, n_pub, m, pool=pool[0], vk_zero=(W + 1,), proof_zero={1: [1], 3: [P - 1]})
    b = V.break_rows(clean, {2: kind})
    pts, sc = pooled_points(engine, b, pool), V.batch_scalars(b)
    assert pts["vk"][1][W + 1] and pts["inf"][1, 1] and pts["inf"][3, P - 1] and pts["inf"].sum() == 2 and pts["vk"][1].sum() == 1
    assert V.batch_verify(b, sc) == [True, True, False, True, True]
    assert call_args(b, pts)[3] is None or n_pub
    check_fold(engine, b, pts, sc, [1, 2, 3])
    ok, status = engine.plonk_verify(tau_g2, *call_args(b, pts), *dims(b), proof_inf=pts["inf"])
    assert list(ok) == [1, 1, 0, 1, 1] and list(status) == [0] * m
    w = [rng.getrandbits(256) for _ in range(m)]
    p0, p1, want_one = V.batch_weighted(b, w, sc)
    gt, one, status = weighted(engine, tau_g2, b, pts, w)
    assert not one and not want_one and np.array_equal(gt[0], oracle_gt(p0, p1, tau_g2)) and list(status) == [0] * m
    w[2] = 0
    gt, one, status = weighted(engine, tau_g2, b, pts, w)
    assert one and V.batch_weighted(b, w, sc)[2] and np.array_equal(gt[0], K.ONE48)


# ---- proofs the device's prover did not write ------------------------------------------------------------------------------------------------
INDEPENDENT = [(2, 2, 0), (3, 2, 1), (3, 3, 8), (2, 3, 8)]       # (W, log_e, l) at log_n = 3


def independent(W, log_e, l):
    """three proofs of ONE circuit by the model's prover (V.proof_for), as a batch, and its points by the oracle; at log_e = 3 the upper chunks
    of t commit to the identity and travel as flagged points with garbage underneath"""
    rng = random.Random(0xF400 + 64 * W + 8 * log_e + l)
    first = V.proof_for(rng, LOG_N, W, log_e, l)
    b = V.batch_of([first] + [V.proof_for(rng, LOG_N, W, log_e, l, circuit=first["c"]) for _ in range(2)], LOG_N, log_e)
    pts = oracle_points(b)
    assert [bool(f) for f in pts["inf"][0, W + 1:W + 1 + (1 << log_e)]] == [e > W for e in range(1 << log_e)] and not pts["vk"][1].any()
    return b, pts


@pytest.mark.gpu
@pytest.mark.parametrize("W,log_e,l", INDEPENDENT)
def test_proofs_of_the_model_s_prover_verify_on_the_device(engine, tau_g2, W, log_e, l):
    """a convention the device's prover and verifier shared -- the order of the terms, a slot, the sign of a chunk's scalar -- would show here"""
    b, pts = independent(W, log_e, l)
    rng = random.Random(0xF500)
    w = [rng.getrandbits(256) for _ in range(3)]
    ok, status = engine.plonk_verify(tau_g2, *call_args(b, pts), *dims(b), proof_inf=pts["inf"])
    assert list(ok) == [1, 1, 1] and list(status) == [0, 0, 0] and V.batch_verify(b) == [True] * 3
    gt, one, status = weighted(engine, tau_g2, b, pts, w)
    assert one and np.array_equal(gt[0], K.ONE48) and list(status) == [0, 0, 0]
    bad = V.break_rows(b, {1: "evaluation"})
    ok, status = engine.plonk_verify(tau_g2, *call_args(bad, pts), *dims(bad), proof_inf=pts["inf"])
    assert list(ok) == [1, 0, 1] and list(status) == [0, 0, 0]
    gt, one, status = weighted(engine, tau_g2, bad, pts, w)
    p0, p1, want_one = V.batch_weighted(bad, w)
    assert not one and not want_one and np.array_equal(gt[0], oracle_gt(p0, p1, tau_g2))


@pytest.mark.gpu
def test_the_public_layer_at_two_columns_and_eight_chunks(engine, tau_g2):
    from sylow_amd import api
    api.set_engine(engine)
    W, log_e, l = INDEPENDENT[-1]
    b, pts = independent(W, log_e, l)
    verifier = api.PlonkVerifier(LOG_N, b["shifts"], api.G1Affine(*pts["vk"]), api.G2Affine(tau_g2), log_e)
    proofs = api.G1Affine(pts["xy"].reshape(-1, 8), pts["inf"].reshape(-1))
    challenges = lambda x: [x[c] for c in V.CHALLENGES]
    w = [random.Random(0xF600).getrandbits(256) for _ in range(3)]
    ok, status = verifier.verify(proofs, words(b["evals"]), b["pub"], *challenges(b))
    assert ok.dtype == bool and list(ok) == [True] * 3 and list(status) == [0] * 3
    assert verifier.verify_weighted(proofs, words(b["evals"]), b["pub"], *challenges(b), w) is True
    bad = V.break_rows(b, {1: "evaluation"})
    ok, status = verifier.verify(proofs, words(bad["evals"]), bad["pub"], *challenges(bad))
    assert list(ok) == [True, False, True] and list(status) == [0] * 3
    assert verifier.verify_weighted(proofs, words(bad["evals"]), bad["pub"], *challenges(bad), w) is False
    assert verifier.verify_weighted(proofs, words(bad["evals"]), bad["pub"], *challenges(bad), [w[0], R, w[2]]) is True
