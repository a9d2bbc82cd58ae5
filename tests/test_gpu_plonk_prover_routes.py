"""GPU: the two full routes of the PLONK prover -- sylow_popen_open_batch (plonk_open.hip) and sylow_plonk_quotient_batch(_tuned)
(plonk_quotient.hip) -- past one tile, one chunk and one shape, word for word against the integer models of tests/plonk_open_model.py and
tests/plonk_quotient_model.py; the proofs against kzg_open of the model's padded F and z, whose values are in turn the model's.  Which
shape was chosen for which edge:

the opening route
  (a) log_n = 3, E = 4, W = 3, len_f = 16, m = 5, random rows, EVERY instance its own wires, z, pi, t and five challenges, with and without
      public inputs: unchunked, in chunks of 2, 2, 1 (a ragged last chunk: its arrays have stride 1 inside a lease laid out for 2) and of one
      instance; the s0 offsets of every per-instance pointer of po::chunk; and on v + j r
  (b) log_n = 8, W = 2, len_w = n + 2, len_z = n + 3, len_f = 300 (two tiles), m = 3, unchunked and in chunks of 2, 1: the zero fill of the
      padded z from len_z = 259 on, across the tile boundary at 256 and inside the second tile, and F with the wires ending at 258
  (c) (W, E) = (17, 32) and (2, 4) at log_n = 3, m = 2, a satisfied blinded witness and the same with one coefficient of t changed: status
      [0, 1] from F(zeta) minus the folded evaluations (the yf branch of k_po_status) at both ends of W
  (d) len_w = len_z = 1 at W = 2, len_f = 8 and 11: z constant, W_omega the identity with flag 1 and W_zeta not; len_z = 3 with the z of
      instance 1 alone constant: flags [0, 1, 0], so the two flag arrays are neither swapped nor shared; and len_z = 5 < n = 256 through
      plonk_open_linearise (the z row ends before the table rows do), len_out = n and n + 300
  (e) log_n = 0, W = 2, E = 4, len_w = 3, len_z = 4, len_f = 4, m = 300: the lane-per-instance kernels make a second trip (one block under
      max_blocks = 1 through evaluate and linearise), the route unchunked and in chunks of 128, 128, 44; every seventh z is constant, so
      that flags of 1 lie past lane 255

the quotient route
  (f) log_n = 9, E = 4 (N = 2048, 8 tiles), W = 3, len_w = 514, len_z = 515 (the pad boundary inside the third tile), m = 3 with instance 1
      broken, with and without public inputs: the default, max_blocks = 1, chunks of 2, 1 (the second buffer placed for the smaller last
      chunk), the status tail from coefficient 1542 (not a multiple of 256) over two tiles; and on v + j r
  (g) (W, log_e, log_n) = (17, 5, 4) (N = 512, two tiles) and (2, 3, 5), m = 2, one satisfied and one broken instance
  (h) log_n = 0, W = 2, E = 4, len_w = len_z = 1, m = 300 with public inputs, every third instance satisfied and the others random, into a
      status buffer the test filled with 0xFF: the clear and the constants (1800 lanes) walk past one block, at the default and under
      max_blocks = 1

Every scratch limit below is a row of OPEN_LIMITS / QUOTIENT_LIMITS; tests/cpp/plonk_open_plan_test.cpp and plonk_quotient_plan_test.cpp
hold the same rows and check them against the plan's own instances_per_chunk (tests/test_plonk_prover_route_limits.py compares the two)."""
import random

import numpy as np
import pytest

import kzg_prove_model as KP
import ntt_model as T
import plonk_open_model as O
import plonk_quotient_model as Q
from groth16_model import ints, limbs

pytestmark = pytest.mark.gpu
R = O.R
TOP = (1 << 256) - 1
TAU = 0x5EED0FA11CE5 * 0x10001 + 12345
SRS_LEN = 300
# name -> (log_n, log_e, W, len_w, len_z, len_f, m, the limit in bytes, the instances of a full chunk under it)
OPEN_LIMITS = {
    "a_two": (3, 2, 3, 10, 11, 16, 5, 6000, 2),
    "a_one": (3, 2, 3, 10, 11, 16, 5, 4000, 1),
    "b_two": (8, 2, 2, 258, 259, 300, 3, 70000, 2),
    "e_128": (0, 2, 2, 3, 4, 4, 300, 164500, 128),
}
# name -> (log_n, log_e, W, columns, m, the limit in bytes, the instances of a full chunk under it)
QUOTIENT_LIMITS = {
    "f_two": (9, 2, 3, 4, 3, 2200000, 2),
    "f_two_pi": (9, 2, 3, 5, 3, 2200000, 2),
}


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


@pytest.fixture(scope="module")
def srs(engine):
    """tau^k G1gen, k < 300, made on the device; a case takes the first len_f points"""
    xy, inf = engine.g1_generator_mul(limbs(KP.srs_logs(TAU, SRS_LEN)))
    assert not inf.any()
    return xy


# ---- the opening route ---------------------------------------------------------------------------------------------------------------------
OPEN_KEYS = ("wires", "z", "pi", "t", "beta", "gamma", "alpha", "zeta", "v")      # one entry per instance


def open_case(rng, log_n, log_e, W, len_w, len_z, m):
    """random rows: a shared table and shifts, and for every instance its own wires, z, pi, t and five challenges"""
    n = 1 << log_n
    c = {"log_n": log_n, "log_e": log_e, "W": W, "m": m, "ct": rand(rng, 2 * W + 2, n), "shifts": rand(rng, W), "wires": rand(rng, m, W, len_w),
         "z": rand(rng, m, len_z), "pi": rand(rng, m, n), "t": rand(rng, m, n << log_e)}
    for k in ("beta", "gamma", "alpha", "zeta", "v"):
        c[k] = rand(rng, m)
    return c


def open_model(c, len_f, pi=True):
    """per instance (evals, F padded to len_f, z padded to len_f, status)"""
    return [O.open_polys(c["ct"], c["wires"][s], c["z"][s], c["pi"][s] if pi else None, c["t"][s], c["shifts"], c["beta"][s], c["gamma"][s], c["alpha"][s],
                         c["zeta"][s], c["v"][s], c["log_n"], c["log_e"], len_f) for s in range(c["m"])]


def run_open(engine, srs, c, len_f, pi=True, limit=0, ctable=None):
    if ctable is None:
        ctable = engine.plonk_open_ctable_up(words(c["ct"]))
    args = (srs[:len_f], ctable, words(c["wires"]), words(c["z"]), words(c["pi"]) if pi else None, words(c["t"]), limbs(c["shifts"]), limbs(c["beta"]),
            limbs(c["gamma"]), limbs(c["alpha"]), limbs(c["zeta"]), limbs(c["v"]), c["log_e"])
    try:
        engine.set_scratch_limit(limit)
        return engine.plonk_open(*args)
    finally:
        engine.set_scratch_limit(0)


def reference_openings(engine, srs, c, want, len_f):
    """kzg_open of the model's F at zeta and of the model's padded z at zeta w_n, after their values are checked against the model's"""
    zetas = [x % R for x in c["zeta"]]
    zeta_w = [x * T.omega(c["log_n"]) % R for x in zetas]
    y_f, pi_f, inf_f = engine.kzg_open(srs[:len_f], words([w[1] for w in want]), limbs(zetas))
    y_z, pi_z, inf_z = engine.kzg_open(srs[:len_f], words([w[2] for w in want]), limbs(zeta_w))
    assert ints(y_f) == [Q.p_eval(w[1], x) for w, x in zip(want, zetas)] and ints(y_z) == [w[0][2 * c["W"] - 1] for w in want]
    for s, w in enumerate(want):
        if not w[3] & O.STATUS_R_NOT_ZERO:
            assert ints(y_f)[s] == O.folded_value(w[0], c["v"][s] % R, c["W"]), "r(zeta) = 0: F(zeta) is the folded evaluations"
    return (pi_f, inf_f), (pi_z, inf_z)


def assert_open(got, want, ref, tag):
    evals, w_zeta, w_omega, status = got
    m = len(want)
    assert evals.shape == (m, len(want[0][0]), 4) and np.array_equal(evals, words([w[0] for w in want])), tag
    assert list(status) == [w[3] for w in want], tag
    for name, (xy, inf), (ref_xy, ref_inf) in (("W_zeta", w_zeta, ref[0]), ("W_omega", w_omega, ref[1])):
        assert xy.shape == (m, 8) and inf.shape == (m,)
        for w in range(8):                                      # column by column: a failure names the word
            assert np.array_equal(xy[:, w], ref_xy[:, w]), (tag, name, "word", w, np.nonzero(xy[:, w] != ref_xy[:, w])[0][:8])
        assert np.array_equal(inf, ref_inf), (tag, name, "flags")


@pytest.fixture(scope="module")
def case_a():
    c = open_case(random.Random(0xD100), 3, 2, 3, 10, 11, 5)
    return c, {pi: open_model(c, 16, pi) for pi in (False, True)}


@pytest.mark.parametrize("with_pi", [False, True])
def test_a_every_instance_its_own_rows_in_ragged_chunks(engine, srs, case_a, with_pi):
    c, models = case_a
    want, len_f = models[with_pi], 16
    assert [w[3] for w in want] == [1] * 5, "random rows: r(zeta) != 0"
    ref = reference_openings(engine, srs, c, want, len_f)
    whole = run_open(engine, srs, c, len_f, with_pi)
    assert_open(whole, want, ref, "unchunked")
    assert whole[0][:, 6].any() == with_pi, "PI(zeta) = 0 without public inputs"
    for name in ("a_two", "a_one"):                             # chunks of 2, 2, 1 and of one instance
        assert OPEN_LIMITS[name][:7] == (3, 2, 3, 10, 11, len_f, 5)
        assert_open(run_open(engine, srs, c, len_f, with_pi, limit=OPEN_LIMITS[name][7]), want, ref, name)
    if with_pi:
        lifted = dict(c, **{k: lift(c[k]) for k in OPEN_KEYS + ("ct", "shifts")})
        assert min(lifted["v"]) >= R and min(min(r) for r in lifted["t"]) >= R
        again = run_open(engine, srs, lifted, len_f, True, limit=OPEN_LIMITS["a_two"][7])
        assert again[0].tobytes() == whole[0].tobytes() and again[3].tobytes() == whole[3].tobytes(), "v + j r: the same bytes"
        for got, first in ((again[1], whole[1]), (again[2], whole[2])):
            assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), "v + j r: the same bytes"


def test_b_a_padded_z_of_two_tiles(engine, srs):
    log_n, W, len_f = 8, 2, 300
    n = 1 << log_n
    c = open_case(random.Random(0xD200), log_n, 2, W, n + 2, n + 3, 3)
    want = open_model(c, len_f)
    assert all(w[2][:n + 3] == c["z"][s] and not any(w[2][n + 3:]) and len(w[2]) == len_f for s, w in enumerate(want)), "z padded with zeros to 300"
    ref = reference_openings(engine, srs, c, want, len_f)
    assert_open(run_open(engine, srs, c, len_f), want, ref, "unchunked")
    assert OPEN_LIMITS["b_two"][:7] == (log_n, 2, W, n + 2, n + 3, len_f, 3)
    assert_open(run_open(engine, srs, c, len_f, limit=OPEN_LIMITS["b_two"][7]), want, ref, "b_two")      # chunks of 2, 1


@pytest.mark.parametrize("W,log_e,with_pi", [(17, 5, True), (2, 2, False)])
def test_c_the_status_from_f_of_zeta_at_both_ends_of_w(engine, srs, W, log_e, with_pi):
    rng = random.Random(0xD300 + W)
    log_n, m, len_f = 3, 2, 16
    s = O.satisfied(rng, log_n, W, log_e, True, with_pi)
    assert len(s["wires"]) == W and len(s["wires"][0]) == 10 and len(s["z"]) == 11 and (s["pi"] is not None) == with_pi
    t1 = list(s["t"])
    t1[5] = (t1[5] + 1) % R
    c = {"log_n": log_n, "log_e": log_e, "W": W, "m": m, "ct": s["ct"], "shifts": s["c"]["shifts"], "wires": [s["wires"]] * m, "z": [s["z"]] * m,
         "pi": [s["pi"]] * m, "t": [s["t"], t1], "beta": [s["beta"]] * m, "gamma": [s["gamma"]] * m, "alpha": [s["alpha"]] * m, "zeta": rand(rng, m),
         "v": rand(rng, m)}
    want = open_model(c, len_f, with_pi)
    assert [w[3] for w in want] == [0, 1]
    ref = reference_openings(engine, srs, c, want, len_f)      # checks F(zeta) of instance 0 against O.folded_value
    ctable = engine.plonk_open_prepare(words(s["c"]["selectors"]), words(s["c"]["sigma"]))
    got = run_open(engine, srs, c, len_f, with_pi, ctable=ctable)
    assert_open(got, want, ref, (W, log_e))
    assert list(got[3]) == [0, 1]


@pytest.mark.parametrize("len_z,len_f,m", [(1, 8, 2), (1, 11, 2), (3, 8, 3)])
def test_d_a_constant_z_opens_to_the_identity(engine, srs, len_z, len_f, m):
    """len_w = 1 and z constant: W_omega is the identity with flag 1, W_zeta is not.  len_z = 3: only instance 1 has z = [c, 0, 0]"""
    rng = random.Random(0xD400 + 16 * len_z + len_f)
    c = open_case(rng, 3, 2, 2, 1, len_z, m)
    if len_z > 1:
        c["z"][1] = [c["z"][1][0]] + [0] * (len_z - 1)
    constant = [not any(z[1:]) for z in c["z"]]
    assert constant == ([True] * m if len_z == 1 else [False, True, False])
    want = open_model(c, len_f)
    ref = reference_openings(engine, srs, c, want, len_f)
    got = run_open(engine, srs, c, len_f)
    assert_open(got, want, ref, (len_z, len_f))
    assert list(got[2][1]) == [int(x) for x in constant] and list(got[1][1]) == [0] * m, "the flags of W_omega and of W_zeta"
    assert list(ref[1][1]) == [int(x) for x in constant], "kzg_open: the identity exactly when the polynomial is constant"


def test_d_linearise_with_z_shorter_than_the_table_rows(engine):
    rng = random.Random(0xD480)
    log_n, log_e, W, m, len_z = 8, 2, 2, 3, 5
    n = 1 << log_n
    c = open_case(rng, log_n, log_e, W, 1, len_z, m)
    evals = rand(rng, m, 2 * W + 1)
    want = [O.linearise(c["ct"], c["wires"][s], c["z"][s], c["t"][s], evals[s], c["shifts"], c["beta"][s], c["gamma"][s], c["alpha"][s], c["zeta"][s],
                        c["v"][s], log_n, log_e) for s in range(m)]
    assert all(len(w[0]) == n and len(w[1]) == n for w in want), "r_len = n > len_z"
    for len_out in (n, n + 300):
        r, f, status = engine.plonk_open_linearise(engine.plonk_open_ctable_up(words(c["ct"])), words(c["wires"]), words(c["z"]), words(c["t"]), words(evals),
                                                   limbs(c["shifts"]), limbs(c["beta"]), limbs(c["gamma"]), limbs(c["alpha"]), limbs(c["zeta"]), limbs(c["v"]),
                                                   log_e, len_out=len_out)
        assert r.shape == (m, len_out, 4) and f.shape == (m, len_out, 4) and not r[:, n:].any() and not f[:, n:].any(), len_out
        assert np.array_equal(r[:, :n], words([w[0] for w in want])) and np.array_equal(f[:, :n], words([w[1] for w in want])), len_out
        assert list(status) == [w[2] for w in want], len_out


@pytest.fixture(scope="module")
def case_e():
    """300 instances of one row each; every seventh z is constant, so that flags of 1 lie on both sides of lane 255"""
    c = open_case(random.Random(0xD500), 0, 2, 2, 3, 4, 300)
    for s in range(0, 300, 7):
        c["z"][s] = [c["z"][s][0], 0, 0, 0]
    return c, open_model(c, 4)


def test_e_more_instances_than_a_block_has_lanes_kernel_entries(engine, case_e):
    c, want = case_e
    m, W = c["m"], c["W"]
    ctable = engine.plonk_open_ctable_up(words(c["ct"]))
    want_ev = words([w[0] for w in want])
    lin = [O.linearise(c["ct"], c["wires"][s], c["z"][s], c["t"][s], want[s][0], c["shifts"], c["beta"][s], c["gamma"][s], c["alpha"][s], c["zeta"][s],
                       c["v"][s], c["log_n"], c["log_e"]) for s in range(m)]
    for pins in ({}, {"max_blocks": 1}):                        # one block walks 300 lanes in two trips
        evals = engine.plonk_open_evaluate(ctable, words(c["wires"]), words(c["z"]), words(c["pi"]), limbs(c["zeta"]), **pins)
        assert evals.shape == (m, 2 * W + 1, 4) and np.array_equal(evals, want_ev), pins
        r, f, status = engine.plonk_open_linearise(ctable, words(c["wires"]), words(c["z"]), words(c["t"]), want_ev, limbs(c["shifts"]), limbs(c["beta"]),
                                                   limbs(c["gamma"]), limbs(c["alpha"]), limbs(c["zeta"]), limbs(c["v"]), c["log_e"], **pins)
        assert np.array_equal(r, words([x[0] for x in lin])) and np.array_equal(f, words([x[1] for x in lin])) and list(status) == [x[2] for x in lin], pins


def test_e_more_instances_than_a_block_has_lanes_full_route(engine, srs, case_e):
    c, want = case_e
    len_f = 4
    ref = reference_openings(engine, srs, c, want, len_f)
    flags = [int(s % 7 == 0) for s in range(c["m"])]
    assert list(ref[1][1]) == flags and not ref[0][1].any() and sum(flags[256:]) >= 6
    assert_open(run_open(engine, srs, c, len_f), want, ref, "unchunked")
    assert OPEN_LIMITS["e_128"][:7] == (0, 2, 2, 3, 4, len_f, 300)
    assert_open(run_open(engine, srs, c, len_f, limit=OPEN_LIMITS["e_128"][7]), want, ref, "e_128")      # chunks of 128, 128, 44


# ---- the quotient route --------------------------------------------------------------------------------------------------------------------
def quotient_case(rng, log_n, log_e, W, with_pi, m, broken):
    """one circuit, m blinded witnesses (len_w = n + 2, len_z = n + 3) under their own challenges, the instances in `broken` with one wire
    value changed under the same z, and the model's (t, status) of each"""
    n = 1 << log_n
    c = Q.circuit(rng, log_n, W, with_pi)
    rows, zinv = Q.table(c["selectors"], c["sigma"], log_n, log_e)
    ch = [(rng.randrange(R), rng.randrange(R), rng.randrange(R)) for _ in range(m)]
    polys = [Q.witness_polys(c, b, g, rng) for b, g, _ in ch]
    for s in broken:
        wires = [list(w) for w in c["wires"]]
        wires[1][n // 2] = (wires[1][n // 2] + 1) % R
        bw = Q.witness_polys(c, ch[s][0], ch[s][1], wires=wires)[0]
        polys[s] = ([w + [0, 0] for w in bw], polys[s][1], polys[s][2])
    assert all((len(p[0][0]), len(p[1])) == (n + 2, n + 3) for p in polys)
    want = [Q.quotient(rows, zinv, wc, zc, pc, c["shifts"], b, g, a, log_n, log_e) for (wc, zc, pc), (b, g, a) in zip(polys, ch)]
    return {"c": c, "log_n": log_n, "log_e": log_e, "ch": ch, "polys": polys, "want": want}


def run_quotient(engine, q, limit=0, lifted=False, **pins):
    up = lift if lifted else (lambda x: x)
    c, polys, ch = q["c"], q["polys"], q["ch"]
    table = engine.plonk_quotient_prepare(words(up(c["selectors"])), words(up(c["sigma"])), q["log_e"])
    args = (words(up([p[0] for p in polys])), words(up([p[1] for p in polys])), words(up([p[2] for p in polys])) if c["pi"] is not None else None,
            limbs(up(c["shifts"])), limbs(up([x[0] for x in ch])), limbs(up([x[1] for x in ch])), limbs(up([x[2] for x in ch])), q["log_n"], q["log_e"])
    try:
        engine.set_scratch_limit(limit)
        return engine.plonk_quotient(table, *args, **pins)
    finally:
        engine.set_scratch_limit(0)


def assert_quotient(got, q, tag):
    t, status = got
    m, big = len(q["want"]), 1 << (q["log_n"] + q["log_e"])
    assert t.shape == (m, big, 4) and list(status) == [s for _, s in q["want"]], tag
    for s in range(m):
        assert np.array_equal(t[s], limbs(q["want"][s][0])), (tag, "instance", s)


@pytest.fixture(scope="module")
def case_f():
    return {with_pi: quotient_case(random.Random(0xD600 + with_pi), 9, 2, 3, with_pi, 3, broken=(1,)) for with_pi in (False, True)}


@pytest.mark.parametrize("with_pi", [False, True])
def test_f_the_quotient_over_eight_tiles(engine, case_f, with_pi):
    q = case_f[with_pi]
    log_n, log_e, W, n, big = 9, 2, 3, 512, 2048
    assert [s for _, s in q["want"]] == [0, 1, 0], "the satisfied instances divide; the broken one leaves a tail"
    first = Q.degree_bound(log_n, W, n + 2, n + 3) - n + 1
    assert first == 1542 and first % 256 and (big - first) > 256, "the status tail starts inside a tile and spans more than one"
    assert 2 * 256 < n + 2 < n + 3 < 3 * 256, "the pad boundary lies inside the third tile"
    whole = run_quotient(engine, q)
    assert_quotient(whole, q, "default")
    assert_quotient(run_quotient(engine, q, max_blocks=1), q, "max_blocks = 1")
    name = "f_two_pi" if with_pi else "f_two"
    assert QUOTIENT_LIMITS[name][:5] == (log_n, log_e, W, W + 1 + with_pi, 3)
    assert_quotient(run_quotient(engine, q, limit=QUOTIENT_LIMITS[name][5]), q, name)                   # chunks of 2, 1
    if with_pi:
        again = run_quotient(engine, q, limit=QUOTIENT_LIMITS[name][5], lifted=True)
        assert again[0].tobytes() == whole[0].tobytes() and again[1].tobytes() == whole[1].tobytes(), "v + j r: the same bytes"


@pytest.mark.parametrize("W,log_e,log_n,with_pi", [(17, 5, 4, True), (2, 3, 5, False)])
def test_g_the_quotient_at_both_ends_of_w(engine, W, log_e, log_n, with_pi):
    q = quotient_case(random.Random(0xD700 + W), log_n, log_e, W, with_pi, 2, broken=(1,))
    assert Q.args_ok(log_n, log_e, W, (1 << log_n) + 2, (1 << log_n) + 3) and [s for _, s in q["want"]] == [0, 1]
    assert_quotient(run_quotient(engine, q), q, (W, log_e, log_n))
    assert_quotient(run_quotient(engine, q, max_blocks=1), q, (W, log_e, log_n, "max_blocks = 1"))


def quotient_into(engine, table, wires, z, pi, shifts, beta, gamma, alpha, log_n, log_e, status, max_blocks=-1):
    """engine.plonk_quotient into the caller's status buffer (a DeviceArray of m bytes): a byte the call leaves unwritten keeps its contents"""
    w, z, pi = (np.ascontiguousarray(x, dtype=np.uint64) for x in (wires, z, pi))
    m, W, len_w, len_z = w.shape[0], w.shape[1], w.shape[2], z.shape[1]
    dw, dz, dpi = (engine.to_device(np.ascontiguousarray(np.swapaxes(x, -1, -2))) for x in (w, z, pi))
    dsh, db, dg, da = (engine.to_device_soa(x, 4) for x in (shifts, beta, gamma, alpha))
    dt = engine.empty((m, 4, 1 << (log_n + log_e)))
    ins = [table.ptr, dw.ptr, len_w, dz.ptr, len_z, dpi.ptr, dsh.ptr, db.ptr, dg.ptr, da.ptr, log_n, log_e, W, m]
    if max_blocks < 0:
        engine._call("sylow_plonk_quotient_batch", *ins, dt.ptr, status.ptr)
    else:
        engine._call("sylow_plonk_quotient_batch_tuned", *ins, int(max_blocks), dt.ptr, status.ptr)
    return np.ascontiguousarray(dt.download().transpose(0, 2, 1)), status.download()


def case_h(rng):
    """a circuit of one row and two wires, and 300 instances of one coefficient a polynomial: every third one satisfies the circuit (wires
    constant on the cycles of the copy permutation, z = 1, the public input that closes the gate), the others are random"""
    m = 300
    c = Q.circuit(rng, 0, 2, with_pi=True)
    rows, zinv = Q.table(c["selectors"], c["sigma"], 0, 2)
    (q0,), (q1,), (qm,), (qc,) = c["selectors"]
    wires, z, pi = [], [], []
    for s in range(m):
        if s % 3:
            w0, w1, zs, p = rand(rng, 4)
        else:
            w0 = rng.randrange(R)
            w1 = w0 if c["mapping"] != [0, 1] else rng.randrange(R)
            zs, p = 1, -(qm * w0 * w1 + q0 * w0 + q1 * w1 + qc) % R
        wires.append([[w0], [w1]])
        z.append([zs])
        pi.append([p])
    ch = [rand(rng, 3) for _ in range(m)]
    want = [Q.quotient(rows, zinv, wires[s], z[s], pi[s], c["shifts"], *ch[s], 0, 2) for s in range(m)]
    return c, wires, z, pi, ch, want


def test_h_more_instances_than_a_block_has_lanes(engine):
    c, wires, z, pi, ch, want = case_h(random.Random(0xD801))
    m = len(want)
    assert c["mapping"] == [1, 0], "the copy permutation swaps the two wires: sigma is not the identity's"
    statuses = [s for _, s in want]
    assert statuses == [int(s % 3 != 0) for s in range(m)], "the model: the satisfied instances divide, the random ones do not"
    assert 0 in statuses[256:] and 1 in statuses[256:] and m * (2 + 4) > 256
    table = engine.plonk_quotient_prepare(words(c["selectors"]), words(c["sigma"]), 2)
    for pins in ({}, {"max_blocks": 1}):
        status = engine.to_device(np.full((m,), 0xFF, dtype=np.uint8))
        t, got = quotient_into(engine, table, words(wires), words(z), words(pi), limbs(c["shifts"]), limbs([x[0] for x in ch]), limbs([x[1] for x in ch]),
                               limbs([x[2] for x in ch]), 0, 2, status, **pins)
        assert list(got) == statuses, (pins, np.nonzero(got != np.array(statuses, dtype=np.uint8))[0][:8])
        assert np.array_equal(t, words([w for w, _ in want])), pins
