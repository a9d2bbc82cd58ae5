"""GPU: PLONK's quotient polynomial -- sylow_plonk_quotient_prepare, sylow_plonk_quotient_evals_batch(_tuned) and
sylow_plonk_quotient_batch(_tuned) (plonk_quotient.hip) -- word for word against the integer model of tests/plonk_quotient_model.py: the table
against the model and against the composition of transforms the header names; the fused kernel on random values at N = 4, 32 and 2048
(several tiles, the wrap of i + E across them, more than 16 products in the gate sum, one block walking every item) and on v + j r; the full
route at len_w = n and n + 2 with and without public inputs, under a scratch limit that forces one instance per chunk, with the statuses
of broken witnesses; and the loop closed through the API: grand product -> coefficients -> quotient -> N(zeta) = t(zeta) (zeta^n - 1)."""
import random

import numpy as np
import pytest

import ntt_model as T
import plonk_quotient_model as Q
from groth16_model import ints, limbs

pytestmark = pytest.mark.gpu
R = Q.R
TOP = (1 << 256) - 1
SCRATCH_FOR_ONE = 20000          # bytes: one instance of the full route at log_n = 3, E = 4, W = 3 and not two (checked below from the lease rule)


def words(rows):
    """nested lists of ints [..][n] -> [.., n, 4] words"""
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


def rand(rng, *shape):
    if len(shape) == 1:
        return [rng.randrange(R) for _ in range(shape[0])]
    return [rand(rng, *shape[1:]) for _ in range(shape[0])]


def lift(tree, rng):
    """v + j r for every value of a nested list, j >= 1: another word for the same element of Fr"""
    if isinstance(tree, list):
        return [lift(t, rng) for t in tree]
    return tree + rng.randrange(1, (TOP - tree) // R + 1) * R


@pytest.mark.parametrize("log_n,W,log_e", [(0, 2, 2), (3, 3, 2), (3, 2, 3), (5, 4, 0)])
def test_the_table_is_the_model_s_and_the_composition_of_transforms(engine, log_n, W, log_e):
    rng = random.Random(0xA100 + 16 * log_n + W)
    n, lb = 1 << log_n, log_n + log_e
    selectors, sigma = rand(rng, W + 2, n), rand(rng, W, n)
    table = engine.plonk_quotient_prepare(words(lift(selectors, rng)), words(lift(sigma, rng)), log_e)
    rows, zinv = engine.plonk_quotient_table_down(table, W, log_n, log_e)
    want_rows, want_zinv = Q.table(selectors, sigma, log_n, log_e)
    assert np.array_equal(rows, words(want_rows)) and np.array_equal(zinv, limbs(want_zinv))
    # word for word what the transforms return: inverse on <w_n>, zero padding, forward with shift 5 on N points
    values = np.concatenate([words(selectors), words(sigma), words([[1] + [0] * (n - 1)])])
    coeffs = engine.fr_ntt(values, inverse=True)
    padded = np.concatenate([coeffs, np.zeros((2 * W + 3, (1 << lb) - n, 4), dtype=np.uint64)], axis=1)
    assert np.array_equal(rows, engine.fr_ntt(padded, shift=limbs([Q.SHIFT])[0]))


@pytest.fixture(scope="module")
def evals_cases():
    """(log_n, log_e, W, m) -> the inputs of the fused kernel, random values on K, and the model's t_ext, made once"""
    out = {}
    for log_n, log_e, W, m in ((0, 2, 2, 1), (3, 2, 3, 2), (9, 2, 2, 3), (9, 2, 17, 3)):
        rng = random.Random(0xA200 + 64 * log_n + W)
        big = 1 << (log_n + log_e)
        c = {"rows": rand(rng, 2 * W + 3, big), "zinv": rand(rng, 1 << log_e), "wires": rand(rng, m, W, big), "z": rand(rng, m, big), "pi": rand(rng, m, big),
             "shifts": rand(rng, W), "beta": rand(rng, m), "gamma": rand(rng, m), "alpha": rand(rng, m)}
        c["want"] = [Q.quotient_evals(c["rows"], c["zinv"], c["wires"][s], c["z"][s], c["pi"][s], c["shifts"], c["beta"][s], c["gamma"][s], c["alpha"][s],
                                      log_n, log_e) for s in range(m)]
        out[(log_n, log_e, W, m)] = c
    return out


def run_evals(engine, c, log_n, log_e, pi=True, **pins):
    table = engine.plonk_quotient_table_up(words(c["rows"]), limbs(c["zinv"]))
    return engine.plonk_quotient_evals(table, words(c["wires"]), words(c["z"]), words(c["pi"]) if pi else None, limbs(c["shifts"]), limbs(c["beta"]),
                                       limbs(c["gamma"]), limbs(c["alpha"]), log_n, log_e, **pins)


@pytest.mark.parametrize("key", [(0, 2, 2, 1), (3, 2, 3, 2), (9, 2, 2, 3), (9, 2, 17, 3)])
def test_the_fused_kernel_against_the_model(engine, evals_cases, key):
    log_n, log_e, W, m = key
    c = evals_cases[key]
    got = run_evals(engine, c, log_n, log_e)
    assert got.shape == (m, 1 << (log_n + log_e), 4) and np.array_equal(got, words(c["want"])), key
    if log_n == 9:
        assert np.array_equal(run_evals(engine, c, log_n, log_e, max_blocks=1), got), "one block walks every item: the words do not depend on the pin"
        assert np.array_equal(run_evals(engine, c, log_n, log_e, max_blocks=5), got)
    # no public inputs: PI = 0 is the same as a column of zeros
    no_pi = run_evals(engine, c, log_n, log_e, pi=False)
    zeros = dict(c, pi=[[0] * (1 << (log_n + log_e)) for _ in range(m)])
    assert np.array_equal(no_pi, run_evals(engine, zeros, log_n, log_e)) and not np.array_equal(no_pi, got)


@pytest.mark.parametrize("key", [(3, 2, 3, 2), (9, 2, 17, 3)])
def test_the_fused_kernel_takes_any_words_mod_r(engine, evals_cases, key):
    log_n, log_e, W, m = key
    c = evals_cases[key]
    rng = random.Random(0xA300)
    lifted = {k: (v if k == "want" else lift(v, rng)) for k, v in c.items()}
    assert min(lifted["beta"]) >= R and min(min(r) for r in lifted["rows"]) >= R
    assert np.array_equal(run_evals(engine, lifted, log_n, log_e), words(c["want"]))


@pytest.fixture(scope="module")
def circuits():
    """a circuit of 8 rows and 3 wires without public inputs and one with, and the model's table of each, made once"""
    out = {}
    for with_pi in (False, True):
        c = Q.circuit(random.Random(0xA400 + with_pi), 3, 3, with_pi)
        c["rows"], c["zinv"] = Q.table(c["selectors"], c["sigma"], 3, 2)
        out[with_pi] = c
    return out


@pytest.mark.parametrize("with_pi", [False, True])
@pytest.mark.parametrize("blinded", [False, True])
def test_the_full_route_against_the_model(engine, circuits, blinded, with_pi):
    c, rng = circuits[with_pi], random.Random(0xA410 + 2 * blinded + with_pi)
    log_n, log_e, W, m = 3, 2, 3, 3
    n, big = 1 << log_n, 1 << (log_n + log_e)
    table = engine.plonk_quotient_prepare(words(c["selectors"]), words(c["sigma"]), log_e)
    ch = [(rng.randrange(R), rng.randrange(R), rng.randrange(R)) for _ in range(m)]
    polys = [Q.witness_polys(c, b, g, rng if blinded else None) for b, g, _ in ch]
    if blinded:                                                   # len_w = n + 2, len_z = n + 3: D - n = 3 n + 5 < 4 n
        assert (len(polys[0][0][0]), len(polys[0][1])) == (n + 2, n + 3)
    # instance 1 is broken: one wire value changed under the same z
    broken = [list(w) for w in c["wires"]]
    broken[1][4] = (broken[1][4] + 1) % R
    bw = Q.witness_polys(c, ch[1][0], ch[1][1], wires=broken)[0]
    polys[1] = ([w + [0] * (len(polys[1][0][0]) - n) for w in bw], polys[1][1], polys[1][2])
    want = [Q.quotient(c["rows"], c["zinv"], wc, zc, pc, c["shifts"], b, g, a, log_n, log_e) for (wc, zc, pc), (b, g, a) in zip(polys, ch)]
    assert [s for _, s in want] == [0, 1, 0], "the satisfied instances divide; the broken one leaves a tail"
    args = (words([p[0] for p in polys]), words([p[1] for p in polys]), words([p[2] for p in polys]) if with_pi else None, limbs(c["shifts"]),
            limbs([x[0] for x in ch]), limbs([x[1] for x in ch]), limbs([x[2] for x in ch]), log_n, log_e)
    t, status = engine.plonk_quotient(table, *args)
    assert t.shape == (m, big, 4) and np.array_equal(t, words([w for w, _ in want])) and list(status) == [s for _, s in want]
    # the same words under a scratch limit that holds one instance, and under the pin
    try:
        engine.set_scratch_limit(SCRATCH_FOR_ONE)
        chunked = engine.plonk_quotient(table, *args)
    finally:
        engine.set_scratch_limit(0)
    pinned = engine.plonk_quotient(table, *args, max_blocks=1)
    for got in (chunked, pinned):
        assert np.array_equal(got[0], t) and np.array_equal(got[1], status)


def test_the_scratch_limit_of_the_chunked_run_holds_one_instance_and_not_two():
    """the limit the test above sets, from the lease rule of the header's plan: per chunk 4 + 4 N / 2 words of shift and roots, 4 (W + 4) of
    constants and two buffers of cols 4 N words per instance, and the transform's 4 + 4 N / 2 words and one buffer more"""
    for cols in (4, 5):
        one, two = [(4 + 64 + 28 * k + 2 * 128 * cols * k + 4 + 64 + 128 * cols * k) * 8 for k in (1, 2)]
        assert one <= SCRATCH_FOR_ONE < two, (cols, one, two)


def test_the_statuses_where_the_flag_is_exact(engine):
    """D < N (W = 2, unblinded, E = 4): a changed wire, a changed public input and a scaled z each raise bit 0; the witness itself does not"""
    rng = random.Random(0xA500)
    log_n, log_e, W = 3, 2, 2
    n = 1 << log_n
    assert Q.degree_bound(log_n, W, n, n) < 1 << (log_n + log_e)
    c = Q.circuit(rng, log_n, W, with_pi=True)
    rows, zinv = Q.table(c["selectors"], c["sigma"], log_n, log_e)
    table = engine.plonk_quotient_prepare(words(c["selectors"]), words(c["sigma"]), log_e)
    beta, gamma, alpha = rng.randrange(R), rng.randrange(R), rng.randrange(R)
    wc, zc, pc = Q.witness_polys(c, beta, gamma)
    wires = [list(w) for w in c["wires"]]
    wires[1][n - 1] = (wires[1][n - 1] + 1) % R
    cases = [(wc, zc, pc), (Q.witness_polys(c, beta, gamma, wires=wires)[0], zc, pc), (wc, zc, Q.coefficients([(c["pi"][0] + 1) % R] + c["pi"][1:], log_n)),
             (wc, Q.p_scale(zc, 3), pc)]
    want = [Q.quotient(rows, zinv, w, z, p, c["shifts"], beta, gamma, alpha, log_n, log_e) for w, z, p in cases]
    assert [s for _, s in want] == [0, 1, 1, 1]
    m = len(cases)
    t, status = engine.plonk_quotient(table, words([x[0] for x in cases]), words([x[1] for x in cases]), words([x[2] for x in cases]), limbs(c["shifts"]),
                                      limbs([beta] * m), limbs([gamma] * m), limbs([alpha] * m), log_n, log_e)
    assert list(status) == [0, 1, 1, 1] and np.array_equal(t, words([w for w, _ in want]))


def test_the_loop_closes_through_the_api(engine):
    """PlonkPermutation.grand_product -> intt -> PlonkQuotient.quotient -> status 0, then N(zeta) = t(zeta) (zeta^n - 1) at a random zeta with
    every evaluation in Python ints"""
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0xA600)
    log_n, log_e, W = 4, 2, 3
    n = 1 << log_n
    c = Q.circuit(rng, log_n, W, with_pi=True)
    perm = api.PlonkPermutation.from_mapping(log_n, c["shifts"], c["mapping"])
    assert np.array_equal(perm.sigma, words(c["sigma"]))
    beta, gamma, alpha = rng.randrange(R), rng.randrange(R), rng.randrange(R)
    z_vals, status = perm.grand_product(words(c["wires"]), [beta], [gamma])
    assert list(status) == [0]
    z_c = ints(api.intt(z_vals)[0])
    w_c = [ints(row) for row in api.intt(words(c["wires"]))]
    pi_c = ints(api.intt(words(c["pi"])))
    # the prover's blinding, on the host: two values per wire, three for z
    w_c = [Q.blind(w, log_n, [rng.randrange(R), rng.randrange(R)]) for w in w_c]
    z_c = Q.blind(z_c, log_n, [rng.randrange(R) for _ in range(3)])
    quotient = api.PlonkQuotient(log_n, c["shifts"], perm.sigma, c["selectors"], log_e)
    t, status = quotient.quotient([w_c], [z_c], [beta], [gamma], [alpha], pi=[pi_c])
    assert t.shape == (1, n << log_e, 4) and list(status) == [0]
    t_c = ints(t[0])
    assert not any(t_c[Q.degree_bound(log_n, W, n + 2, n + 3) - n + 1:])
    zeta = rng.randrange(R)
    ev = lambda coeffs: Q.p_eval(coeffs, zeta)
    q = [ev(Q.coefficients(v, log_n)) for v in c["selectors"]]
    sg = [ev(Q.coefficients(v, log_n)) for v in c["sigma"]]
    wz, zz, zwz = [ev(w) for w in w_c], ev(z_c), Q.p_eval(z_c, zeta * T.omega(log_n) % R)
    gate = (q[W] * wz[0] * wz[1] + sum(q[j] * wz[j] for j in range(W)) + q[W + 1] + ev(pi_c)) % R
    a, b = zz, zwz
    for j in range(W):
        a = a * (wz[j] + beta * c["shifts"][j] * zeta + gamma) % R
        b = b * (wz[j] + beta * sg[j] + gamma) % R
    vanishing = (pow(zeta, n, R) - 1) % R
    l1 = vanishing * T.inv(n * (zeta - 1)) % R
    numerator = (gate + alpha * (a - b) + alpha * alpha * l1 * (zz - 1)) % R
    assert numerator == ev(t_c) * vanishing % R
    # with words instead of ints, and one instance without the batch dimension
    t2, status2 = quotient.quotient(words(w_c), words([z_c]), limbs([beta]), limbs([gamma]), limbs([alpha]), pi=words([pi_c]))
    assert np.array_equal(t2, t) and list(status2) == [0]
    with pytest.raises(ValueError):
        api.PlonkQuotient(log_n, c["shifts"], perm.sigma, c["selectors"][:-1], log_e)
