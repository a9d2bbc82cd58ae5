"""GPU: PLONK's closing rounds -- sylow_popen_prepare, sylow_popen_evaluate_batch(_tuned), sylow_popen_linearise_batch(_tuned) and
sylow_popen_open_batch (plonk_open.hip) -- word for word against the integer model of tests/plonk_open_model.py.  The outputs of the
evaluation and of the linearisation are formulas in their inputs, so the kernel tests run on RANDOM rows of the stated lengths: log_n = 0, 3,
8 and 11 with len_w = n + 2 and len_z = n + 3 (one coefficient per row of the table at log_n = 0; 2050 and 2051 at log_n = 11, two and three
coefficients past a chunk of 2048; 259 at log_n = 8, three columns past a tile of 256), W = 2 and 17 for the evaluations and (W, E) = (2, 4),
(3, 4), (4, 8), (17, 32) for r and F -- 11 products a column for r and exactly 16 with F, 16 and more, and several flushes -- m = 3, with and
without public inputs, under max_blocks = 1, 5 and the default, and on v + j r with the largest j.  Then satisfied witnesses: the statuses,
the full route against kzg_open of the model's F and of z, chunked under a scratch limit, and the loop closed through the API up to
KzgVerifier.verify."""
import random

import numpy as np
import pytest

import groth16_model as G
import kzg_prove_model as M
import ntt_model as T
import plonk_open_model as O
import plonk_quotient_model as Q
from groth16_model import ints, limbs

pytestmark = pytest.mark.gpu
R = O.R
TOP = (1 << 256) - 1
TAU = 0x5EED0FA11CE5 * 0x10001 + 12345
LOG_NS = (0, 3, 8, 11)
M_INST = 3
SCRATCH_FOR_ONE = 4000           # bytes: one instance of the full route at log_n = 3, E = 4, W = 3, len_f = 16 and not two (checked below)


def words(rows):
    """nested lists of ints [..][n] -> [.., n, 4] words"""
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


def rand(rng, *shape):
    if len(shape) == 1:
        return [rng.randrange(R) for _ in range(shape[0])]
    return [rand(rng, *shape[1:]) for _ in range(shape[0])]


def lift(tree):
    """v + j r with the largest j that fits 256 bits, for every value of a nested list: another word for the same element of Fr"""
    if isinstance(tree, list):
        return [lift(t) for t in tree]
    return tree + (TOP - tree) // R * R


@pytest.mark.parametrize("log_n,W", [(0, 2), (3, 3), (5, 4)])
def test_the_coefficient_table_is_the_model_s_and_the_inverse_transform(engine, log_n, W):
    rng = random.Random(0xC100 + 16 * log_n + W)
    n = 1 << log_n
    selectors, sigma = rand(rng, W + 2, n), rand(rng, W, n)
    got = engine.plonk_open_ctable_down(engine.plonk_open_prepare(words(lift(selectors)), words(lift(sigma))))
    assert got.shape == (2 * W + 2, n, 4) and np.array_equal(got, words(O.ctable(selectors, sigma, log_n)))
    assert np.array_equal(got, engine.fr_ntt(np.concatenate([words(selectors), words(sigma)]), inverse=True))


# ---- the evaluations -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eval_cases():
    """(log_n, W) -> random rows (the table, the wires at len_w = n + 2, z at len_z = n + 3, pi, zeta) and the model's evaluations, made once"""
    out = {}
    for log_n in LOG_NS:
        for W in (2, 17):
            rng = random.Random(0xC200 + 64 * log_n + W)
            n = 1 << log_n
            c = {"ct": rand(rng, 2 * W + 2, n), "wires": rand(rng, M_INST, W, n + 2), "z": rand(rng, M_INST, n + 3), "pi": rand(rng, M_INST, n),
                 "zeta": rand(rng, M_INST)}
            c["want"] = [O.evaluate(c["ct"], c["wires"][s], c["z"][s], c["pi"][s], c["zeta"][s], log_n) for s in range(M_INST)]
            c["want_no_pi"] = [O.evaluate(c["ct"], c["wires"][s], c["z"][s], None, c["zeta"][s], log_n) for s in range(M_INST)]
            out[(log_n, W)] = c
    return out


def run_evaluate(engine, c, pi=True, **pins):
    return engine.plonk_open_evaluate(engine.plonk_open_ctable_up(words(c["ct"])), words(c["wires"]), words(c["z"]), words(c["pi"]) if pi else None,
                                      limbs(c["zeta"]), **pins)


@pytest.mark.parametrize("W", [2, 17])
@pytest.mark.parametrize("log_n", LOG_NS)
def test_the_evaluations_against_the_model(engine, eval_cases, log_n, W):
    c = eval_cases[(log_n, W)]
    got = run_evaluate(engine, c)
    assert got.shape == (M_INST, 2 * W + 1, 4) and np.array_equal(got, words(c["want"])), (log_n, W)
    no_pi = run_evaluate(engine, c, pi=False)
    assert np.array_equal(no_pi, words(c["want_no_pi"])) and not no_pi[:, 2 * W].any() and got[:, 2 * W].any(), "no public inputs: PI(zeta) = 0"
    for pin in (1, 5):
        assert np.array_equal(run_evaluate(engine, c, max_blocks=pin), got), f"max_blocks = {pin}: the words do not depend on the pin"
    lifted = {k: (v if k.startswith("want") else lift(v)) for k, v in c.items()}
    assert min(lifted["zeta"]) >= R and min(min(r) for r in lifted["ct"]) >= R
    assert run_evaluate(engine, lifted).tobytes() == got.tobytes(), "v + j r: the same bytes"


def test_a_row_of_more_than_256_chunks_beside_short_ones(engine):
    """len_w = 257 chunks of 2048 and one coefficient: the second launch gives a lane two chunks (eval_fold_segment = 2), and the items of
    the short rows (sigma and pi of 8 coefficients, z of 5) past their end store zeros"""
    rng = random.Random(0xC280)
    log_n, W, len_w = 3, 2, 257 * 2048 + 1
    c = {"ct": rand(rng, 2 * W + 2, 8), "wires": rand(rng, 1, W, len_w), "z": rand(rng, 1, 5), "pi": rand(rng, 1, 8), "zeta": rand(rng, 1)}
    want = O.evaluate(c["ct"], c["wires"][0], c["z"][0], c["pi"][0], c["zeta"][0], log_n)
    got = run_evaluate(engine, c)
    assert np.array_equal(got, words([want]))
    assert np.array_equal(run_evaluate(engine, c, max_blocks=3), got)


# ---- r and F ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 2), (3, 2), (4, 3), (17, 5)]        # (W, log_e): E = 4, 4, 8, 32


@pytest.fixture(scope="module")
def lin_cases():
    """(log_n, W) -> random rows (the table, wires, z, t, evaluations, challenges) and the model's (r, F, status), made once"""
    out = {}
    for log_n in LOG_NS:
        for W, log_e in SHAPES:
            rng = random.Random(0xC300 + 64 * log_n + W)
            n = 1 << log_n
            c = {"ct": rand(rng, 2 * W + 2, n), "wires": rand(rng, M_INST, W, n + 2), "z": rand(rng, M_INST, n + 3), "t": rand(rng, M_INST, n << log_e),
                 "evals": rand(rng, M_INST, 2 * W + 1), "shifts": rand(rng, W), "log_e": log_e}
            for k in ("beta", "gamma", "alpha", "zeta", "v"):
                c[k] = rand(rng, M_INST)
            c["want"] = [O.linearise(c["ct"], c["wires"][s], c["z"][s], c["t"][s], c["evals"][s], c["shifts"], c["beta"][s], c["gamma"][s], c["alpha"][s],
                                     c["zeta"][s], c["v"][s], log_n, log_e) for s in range(M_INST)]
            out[(log_n, W)] = c
    return out


def run_linearise(engine, c, **kw):
    return engine.plonk_open_linearise(engine.plonk_open_ctable_up(words(c["ct"])), words(c["wires"]), words(c["z"]), words(c["t"]), words(c["evals"]),
                                       limbs(c["shifts"]), limbs(c["beta"]), limbs(c["gamma"]), limbs(c["alpha"]), limbs(c["zeta"]), limbs(c["v"]), c["log_e"], **kw)


@pytest.mark.parametrize("W,log_e", SHAPES)
@pytest.mark.parametrize("log_n", LOG_NS)
def test_r_and_f_against_the_model(engine, lin_cases, log_n, W, log_e):
    c, n = lin_cases[(log_n, W)], 1 << log_n
    want_r, want_f, want_s = (words([w[0] for w in c["want"]]), words([w[1] for w in c["want"]]), [w[2] for w in c["want"]])
    assert want_r.shape == (M_INST, n + 3, 4) and want_f.shape == (M_INST, n + 3, 4) and want_s == [1] * M_INST, "random rows: r(zeta) != 0"
    r, f, status = run_linearise(engine, c)
    assert np.array_equal(r, want_r) and np.array_equal(f, want_f) and list(status) == want_s, (log_n, W)
    # r alone, F alone: the same words and the same status
    r1, none, s1 = run_linearise(engine, c, want_f=False)
    assert none is None and np.array_equal(r1, r) and list(s1) == want_s
    none, f2, s2 = run_linearise(engine, c, want_r=False)
    assert none is None and np.array_equal(f2, f) and list(s2) == want_s
    # len_out above the polynomials' length: zeros there, under every pin
    len_out = n + 3 + 300
    for pins in ({}, {"max_blocks": 1}, {"max_blocks": 5}):
        r3, f3, s3 = run_linearise(engine, c, len_out=len_out, **pins)
        assert r3.shape == (M_INST, len_out, 4) and not r3[:, n + 3:].any() and not f3[:, n + 3:].any()
        assert np.array_equal(r3[:, :n + 3], r) and np.array_equal(f3[:, :n + 3], f) and list(s3) == want_s, pins
    lifted = {k: (v if k in ("want", "log_e") else lift(v)) for k, v in c.items()}
    assert min(lifted["v"]) >= R and min(min(row) for row in lifted["t"]) >= R
    r4, f4, s4 = run_linearise(engine, lifted)
    assert r4.tobytes() == r.tobytes() and f4.tobytes() == f.tobytes() and list(s4) == want_s, "v + j r: the same bytes"


def test_the_product_counts_the_shapes_were_chosen_for():
    """(3, 4): 11 products a column for r and exactly 16 with F; (4, 8): 16 for r, more with F; W = 17: several flushes"""
    counts = {(W, 1 << log_e): (W + 4 + (1 << log_e), 3 * W + 3 + (1 << log_e)) for W, log_e in SHAPES}
    assert counts[(3, 4)] == (11, 16) and counts[(4, 8)] == (16, 23) and counts[(2, 4)] == (10, 13) and counts[(17, 32)][0] > 48


# ---- satisfied witnesses ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def witnesses():
    """with_pi -> a circuit of 8 rows and 3 wires, a blinded witness that satisfies it, its quotient, and the table on the model's side"""
    return {with_pi: O.satisfied(random.Random(0xC400 + with_pi), 3, 3, 2, True, with_pi) for with_pi in (False, True)}


def test_the_statuses_on_a_satisfied_witness(engine, witnesses):
    s, rng = witnesses[True], random.Random(0xC500)
    log_n, log_e, W, sh = 3, 2, 3, witnesses[True]["c"]["shifts"]
    broken = list(s["t"])
    broken[9] = (broken[9] + 1) % R
    zetas, ts = [rng.randrange(2, R), rng.randrange(2, R), T.omega(log_n), 1 + R], [s["t"], broken, s["t"], s["t"]]      # zeta = 1: L1 = 0 by inv(0) = 0
    v = rand(rng, 4)
    ctable = engine.plonk_open_prepare(words(s["c"]["selectors"]), words(s["c"]["sigma"]))
    evals = engine.plonk_open_evaluate(ctable, words([s["wires"]] * 4), words([s["z"]] * 4), words([s["pi"]] * 4), limbs(zetas))
    want_ev = [O.evaluate(s["ct"], s["wires"], s["z"], s["pi"], zeta, log_n) for zeta in zetas]
    assert np.array_equal(evals, words(want_ev))
    want = [O.linearise(s["ct"], s["wires"], s["z"], t, ev, sh, s["beta"], s["gamma"], s["alpha"], zeta, x, log_n, log_e) for t, ev, zeta, x in zip(ts, want_ev, zetas, v)]
    assert [w[2] & 1 for w in want[:2]] == [0, 1] and want[0][2] == 0 and want[2][2] & want[3][2] & O.STATUS_ZETA_IN_DOMAIN
    r, f, status = engine.plonk_open_linearise(ctable, words([s["wires"]] * 4), words([s["z"]] * 4), words(ts), evals, limbs(sh), limbs([s["beta"]] * 4),
                                               limbs([s["gamma"]] * 4), limbs([s["alpha"]] * 4), limbs(zetas), limbs(v), log_e)
    assert list(status) == [w[2] for w in want] and np.array_equal(r, words([w[0] for w in want])) and np.array_equal(f, words([w[1] for w in want]))


@pytest.fixture(scope="module")
def srs():
    return M.srs_points(TAU, 32)


@pytest.mark.parametrize("with_pi", [False, True])
def test_the_full_route_is_kzg_open_of_the_model_s_polynomials(engine, witnesses, srs, with_pi):
    s, rng = witnesses[with_pi], random.Random(0xC600 + with_pi)
    log_n, log_e, W, m, len_f, sh = 3, 2, 3, 2, 16, witnesses[with_pi]["c"]["shifts"]
    assert len(s["wires"][0]) == 10 and len(s["z"]) == 11 and (s["pi"] is not None) == with_pi
    # instance 1: another t, so that its r(zeta) != 0 -- the proofs are still those of the formulas
    t1 = list(s["t"])
    t1[3] = (t1[3] + 5) % R
    ts, zetas, v = [s["t"], t1], rand(rng, m), rand(rng, m)
    want = [O.open_polys(s["ct"], s["wires"], s["z"], s["pi"], t, sh, s["beta"], s["gamma"], s["alpha"], zeta, x, log_n, log_e, len_f)
            for t, zeta, x in zip(ts, zetas, v)]
    assert [w[3] for w in want] == [0, 1]
    ctable = engine.plonk_open_prepare(words(s["c"]["selectors"]), words(s["c"]["sigma"]))
    args = (srs[:len_f], ctable, words([s["wires"]] * m), words([s["z"]] * m), words([s["pi"]] * m) if with_pi else None, words(ts), limbs(sh),
            limbs([s["beta"]] * m), limbs([s["gamma"]] * m), limbs([s["alpha"]] * m), limbs(zetas), limbs(v), log_e)
    evals, w_zeta, w_omega, status = engine.plonk_open(*args)
    assert np.array_equal(evals, words([w[0] for w in want])) and list(status) == [0, 1]
    y_f, pi_f, inf_f = engine.kzg_open(srs[:len_f], words([w[1] for w in want]), limbs(zetas))
    y_z, pi_z, inf_z = engine.kzg_open(srs[:len_f], words([w[2] for w in want]), limbs([zeta * T.omega(log_n) % R for zeta in zetas]))
    assert np.array_equal(w_zeta[0], pi_f) and np.array_equal(w_zeta[1], inf_f) and np.array_equal(w_omega[0], pi_z) and np.array_equal(w_omega[1], inf_z)
    assert ints(y_f)[0] == O.folded_value(want[0][0], v[0], W) and ints(y_z) == [w[0][2 * W - 1] for w in want]
    try:                                                       # one instance per chunk: the same words
        engine.set_scratch_limit(SCRATCH_FOR_ONE)
        chunked = engine.plonk_open(*args)
    finally:
        engine.set_scratch_limit(0)
    assert np.array_equal(chunked[0], evals) and np.array_equal(chunked[3], status)
    for got, ref in ((chunked[1], w_zeta), (chunked[2], w_omega)):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_the_scratch_limit_of_the_chunked_run_holds_one_instance_and_not_two():
    """the limit the test above sets, from the lease rule of plonk_open_plan.hpp at W = 3, E = 4, len_f = 16 and rows of one chunk: per
    instance 8 words of points, 4 (2 W + 1) of partials, 4 (3 W + 5 + E) of weights, 2 x 4 len_f of F and the padded z, 8 of the two values,
    16 of the two proofs, the quotient buffer of kzg_open_batch of 4 len_f, and the flags of the chunk rounded up to a word"""
    one, two = [(k * (8 + 28 + 72 + 128 + 8 + 16 + 64) + (2 * k + 7) // 8) * 8 for k in (1, 2)]
    assert one <= SCRATCH_FOR_ONE < two, (one, two)


def test_the_loop_closes_through_the_api(engine, srs):
    """PlonkPermutation.grand_product -> PlonkQuotient.quotient -> PlonkOpening.open, then KzgVerifier.verify accepts
    (commit(F), zeta, F(zeta), W_zeta) and (commit(z), zeta w_n, z(zeta w_n), W_omega), and rejects both after one evaluation word changes"""
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0xC700)
    log_n, log_e, W, len_f = 4, 2, 3, 32
    c = Q.circuit(rng, log_n, W, with_pi=True)
    perm = api.PlonkPermutation.from_mapping(log_n, c["shifts"], c["mapping"])
    beta, gamma, alpha, zeta, v = (rng.randrange(R) for _ in range(5))
    z_vals, status = perm.grand_product(words(c["wires"]), [beta], [gamma])
    assert list(status) == [0]
    w_c = [Q.blind(ints(row), log_n, [rng.randrange(R), rng.randrange(R)]) for row in api.intt(words(c["wires"]))]
    z_c = Q.blind(ints(api.intt(z_vals)[0]), log_n, [rng.randrange(R) for _ in range(3)])
    pi_c = ints(api.intt(words(c["pi"])))
    t, status = api.PlonkQuotient(log_n, c["shifts"], perm.sigma, c["selectors"], log_e).quotient([w_c], [z_c], [beta], [gamma], [alpha], pi=[pi_c])
    assert list(status) == [0]
    opening = api.PlonkOpening(log_n, c["shifts"], perm.sigma, c["selectors"], log_e)
    prover, verifier = api.KzgProver(api.G1Affine(srs[:len_f])), api.KzgVerifier(api.G2Affine(G.g2_gen_mul([TAU])[0]))
    evals, w_zeta, w_omega, status = opening.open(prover, [w_c], [z_c], t, [beta], [gamma], [alpha], [zeta], [v], pi=[pi_c])
    assert list(status) == [0] and evals.shape == (1, 2 * W + 1, 4)
    ev = ints(evals[0])
    assert ev == O.evaluate(O.ctable(c["selectors"], c["sigma"], log_n), w_c, z_c, pi_c, zeta, log_n)
    assert np.array_equal(opening.evaluate(w_c, z_c, [zeta], pi=pi_c), evals), "one instance without the batch dimension"
    r, f, status = opening.linearise([w_c], [z_c], t, evals, [beta], [gamma], [alpha], [zeta], v=[v])
    assert list(status) == [0] and f.shape == (1, (1 << log_n) + 3, 4)
    r_only = opening.linearise(None, [z_c], t, evals, [beta], [gamma], [alpha], [zeta])
    assert np.array_equal(r_only[0], r) and r_only[1] is None and list(r_only[2]) == [0]
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], len_f - a.shape[1], 4), dtype=np.uint64)], axis=1)
    c_f, c_z = prover.commit(pad(f)), prover.commit(pad(words([z_c])))
    y_f, zeta_w = O.folded_value(ev, v, W), zeta * T.omega(log_n) % R
    assert verifier.verify((c_f, [zeta], [y_f], w_zeta)).all() and verifier.verify((c_z, [zeta_w], [ev[2 * W - 1]], w_omega)).all()
    assert not verifier.verify((c_f, [zeta], [(y_f + 1) % R], w_zeta)).any() and not verifier.verify((c_z, [zeta_w], [(ev[2 * W - 1] + 1) % R], w_omega)).any()
    with pytest.raises(ValueError):
        api.PlonkOpening(log_n, c["shifts"], perm.sigma, c["selectors"][:-1], log_e)
