"""CPU: the model of the batched PLONK verifier (tests/plonk_verify_model.py) on its own.  For a satisfied, blinded witness at log_n = 3,
W = 2 and 3 and l = 0, 1 and n public inputs, the proof comes from the prover's model (plonk_open_model.open_polys and the two quotients);
then verify holds and C - y G1 = (tau - 0) pi holds in the exponent.  After adding 1 to any single evaluation, public input or transcript
challenge, or replacing a proof point by its double, it fails.  With u = 0, tampering W_omega goes unnoticed and tampering W_zeta does not:
that is what u is for.  p equals p_eval of the interpolated PI.

The chunks: a blinded witness of W wires has a quotient of 2 n + 5 (W = 2) or 3 n + 6 (W = 3) coefficients, so E = 1 (log_e = 0) holds no
satisfied instance; the valid proofs run at log_e = 2, the smallest that holds both, and at log_e = 3, where the upper chunks commit to the
identity.  log_e = 0 is covered where no witness is needed: the term count and order below, and the scalars on random words on the device.

u itself is not among the tampered challenges: it is the verifier's own randomness, and a valid proof verifies under every u.

Last, the helpers the batch tests on the device stand on (tests/test_gpu_plonk_verify_batches.py): the rows of V.holding_batch verify at W = 2,
3, 32 with and without chunks and public inputs, every kind of V.break_rows fails but the one that moves zeta into the domain, which keeps
holding under status 2, and the weighted form follows.  This is what makes the reference sound before a device sees it."""
import random

import pytest

import plonk_open_model as O
import plonk_quotient_model as Q
import plonk_verify_model as V

R = V.R
LOG_N = 3
CASES = [(W, log_e, l) for W in (2, 3) for log_e in (2, 3) for l in (0, 1, 1 << LOG_N)]


@pytest.fixture(scope="module")
def proofs():
    return {(W, log_e, l): V.proof_for(random.Random(0xD100 + 64 * W + 8 * log_e + l), LOG_N, W, log_e, l) for W, log_e, l in CASES}


def check(p, log_e, **changed):
    a = {k: p[k] for k in ("vk", "proof", "evals", "pub", "shifts", "ch")}
    a.update(changed)
    return V.verify(a["vk"], a["proof"], a["evals"], a["pub"], a["shifts"], a["ch"], LOG_N, log_e)


def bumped(values, i):
    out = list(values)
    out[i] = (out[i] + 1) % R
    return out


@pytest.mark.parametrize("W,log_e,l", CASES)
def test_a_valid_proof_verifies_and_the_row_holds_in_the_exponent(proofs, W, log_e, l):
    p = proofs[(W, log_e, l)]
    assert check(p, log_e)
    k, y, status = V.scalars(p["evals"], p["pub"], p["shifts"], *(p["ch"][c] for c in V.CHALLENGES), LOG_N, log_e)
    c, pi = V.row(p["vk"], p["proof"], k, p["ch"]["u"])
    assert status == 0 and len(k) == V.terms(W, log_e) == 3 * W + (1 << log_e) + 5 and (c - y) % R == V.TAU * pi % R
    assert len(p["pub"]) == l and not any(p["c"]["pi"][l:]), "PI is zero from row l on"
    # another u, drawn by the verifier alone: still valid
    assert check(p, log_e, ch=dict(p["ch"], u=p["ch"]["u"] + 1))


@pytest.mark.parametrize("W,log_e,l", CASES)
def test_p_is_the_interpolated_public_input_polynomial_at_zeta(proofs, W, log_e, l):
    p = proofs[(W, log_e, l)]
    zeta = p["ch"]["zeta"]
    assert V.pi_eval(p["pub"], zeta, LOG_N) == Q.p_eval(Q.coefficients(p["c"]["pi"], LOG_N), zeta) == p["evals"][2 * W]
    assert check(p, log_e, evals=bumped(p["evals"], 2 * W)), "slot 2 W of the evaluations is not read"
    if l:
        assert V.lagrange(0, zeta, LOG_N) == O.scalars(p["evals"], p["shifts"], 0, 0, zeta, LOG_N)[1], "L_0 is the prover's L1"


@pytest.mark.parametrize("W,log_e,l", CASES)
def test_any_single_change_fails(proofs, W, log_e, l):
    p = proofs[(W, log_e, l)]
    for i in range(2 * W):
        assert not check(p, log_e, evals=bumped(p["evals"], i)), f"evaluation {i}"
    for j in range(l):
        assert not check(p, log_e, pub=bumped(p["pub"], j)), f"public input {j}"
    for c in ("beta", "gamma", "alpha", "zeta", "v"):
        assert not check(p, log_e, ch=dict(p["ch"], **{c: p["ch"][c] + 1})), c
    for i, x in enumerate(p["proof"]):
        if x == 0:                                            # a chunk of t above its degree: the identity is its own double
            assert W + 1 <= i < W + 1 + (1 << log_e)
            continue
        doubled = list(p["proof"])
        doubled[i] = 2 * x % R
        assert not check(p, log_e, proof=doubled), f"proof point {i}"
    # t has 2 n + 5 coefficients at W = 2 and 3 n + 6 at W = 3: every chunk from the fourth (W = 2) or fifth (W = 3) on commits to the identity
    assert [x == 0 for x in p["proof"][W + 1:W + 1 + (1 << log_e)]] == [e > W for e in range(1 << log_e)]


@pytest.mark.parametrize("W", [2, 3])
def test_u_is_what_binds_the_second_opening(proofs, W):
    p = proofs[(W, 2, 1)]
    ch0 = dict(p["ch"], u=0)
    w_omega, w_zeta = list(p["proof"]), list(p["proof"])
    w_omega[-1], w_zeta[-2] = 2 * w_omega[-1] % R, 2 * w_zeta[-2] % R
    assert check(p, 2, ch=ch0) and check(p, 2, ch=ch0, proof=w_omega), "u = 0: W_omega is not checked at all"
    assert not check(p, 2, ch=ch0, proof=w_zeta) and not check(p, 2, proof=w_omega)
    assert check(p, 2, ch=dict(ch0, u=R), proof=w_omega), "u = r is 0"


def test_the_status_and_the_formulas_inside_the_domain():
    rng = random.Random(0xD200)
    W, log_e = 3, 0
    ev, pub, sh = [rng.randrange(R) for _ in range(2 * W + 1)], [rng.randrange(R) for _ in range(8)], [1, 5, 7]
    ch = [rng.randrange(R) for _ in range(6)]
    ch[3] = pow(V.T.omega(LOG_N), 2, R)
    k, y, status = V.scalars(ev, pub, sh, *ch, LOG_N, log_e)
    assert status == V.STATUS_ZETA_IN_DOMAIN and len(k) == 3 * W + 1 + 5 and k[3 * W + 3] == 0, "ZH = 0: the chunk's scalar is 0"
    assert V.pi_eval(pub, ch[3], LOG_N) == 0 and k[-2] == ch[3] and k[W + 1] == 1
    lifted = V.scalars([e + R for e in ev], [x + R for x in pub], [s + R for s in sh], *[c + R for c in ch], LOG_N, log_e)
    assert lifted == (k, y, status), "v + r: the same element of Fr"
    assert not V.verify([1] * (2 * W + 2), [1] * (W + 1 + 3), ev, pub, sh, dict(zip(V.CHALLENGES, ch)), LOG_N, log_e)


def test_the_weighted_form_in_the_exponent(proofs):
    W, log_e = 3, 2
    p, rng = proofs[(W, log_e, 1)], random.Random(0xD300)       # proofs of different circuits share no key: one proof under two u
    other = dict(p, ch=dict(p["ch"], u=rng.randrange(R)))        # the same proof under another u
    batch = [p, other]
    sc = [V.scalars(q["evals"], q["pub"], q["shifts"], *(q["ch"][c] for c in V.CHALLENGES), LOG_N, log_e) for q in batch]
    ks, ys, us = [s[0] for s in sc], [s[1] for s in sc], [q["ch"]["u"] for q in batch]
    w = [rng.randrange(R), rng.randrange(R)]
    assert V.weighted_ok(p["vk"], [q["proof"] for q in batch], ks, ys, us, w, W)
    bad = [list(q["proof"]) for q in batch]
    bad[1][0] = 2 * bad[1][0] % R
    assert not V.weighted_ok(p["vk"], bad, ks, ys, us, w, W)
    assert V.weighted_ok(p["vk"], bad, ks, ys, us, [w[0], R], W), "a weight of r is 0: the broken proof is removed"


# ---- the helpers the batch tests on the device stand on: rows that hold at any shape, and the ways to break them ----------------------------
SHAPES = [(1, 2, 0, 0), (3, 3, 2, 3), (5, 32, 0, 32)]          # (log_n, W, log_e, n_pub); log_e = 0 holds no satisfied witness, and needs none
ROWS = 8


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "-".join(map(str, s)))
def holding(request):
    log_n, W, log_e, n_pub = request.param
    return V.holding_batch(random.Random(0xD400 + 64 * W + 8 * log_e + n_pub), log_n, W, log_e, n_pub, ROWS)


def row_holds(b, i):
    """(C - y = tau pi in the exponent, status) of row i"""
    (k, y, status), = V.batch_scalars(b, [i])
    c, pi = V.row(b["vk"], b["proofs"][i], k, b["u"][i])
    return (c - y - V.TAU * pi) % R == 0, status


def test_every_row_of_a_holding_batch_verifies(holding):
    b = holding
    ch = lambda i: {c: b[c][i] for c in V.CHALLENGES}
    assert all(V.verify(b["vk"], b["proofs"][i], b["evals"][i], b["pub"][i], b["shifts"], ch(i), b["log_n"], b["log_e"]) for i in range(ROWS))
    assert V.batch_verify(b) == [True] * ROWS
    assert max(b["zeta"]) >= R and max(max(r) for r in b["evals"]) >= R and all(v % R for v in b["v"]), "full-range words, v != 0"
    assert len(b["vk"]) == V.key_points(b["W"]) and all(len(p) == V.proof_points(b["W"], b["log_e"]) and all(p) for p in b["proofs"]) and all(b["vk"])


def test_every_kind_of_broken_row_fails_and_the_zeta_kind_keeps_holding(holding):
    b = holding
    where = {i: kind for i, kind in enumerate(V.KINDS) if kind != "public_input" or b["n_pub"]}
    bad = V.break_rows(b, where)
    assert V.batch_verify(b) == [True] * ROWS, "the batch it was made from is untouched"
    assert V.batch_verify(bad) == [i not in where for i in range(ROWS)]
    for i, kind in where.items():
        holds, status = row_holds(bad, i)
        assert (holds, status) == ((True, V.STATUS_ZETA_IN_DOMAIN) if kind == "zeta_in_domain" else (False, 0)), kind
    assert pow(bad["zeta"][4], 1 << b["log_n"], R) == 1 and bad["proofs"][4][1:] == b["proofs"][4][1:] and bad["proofs"][4][0] != b["proofs"][4][0]
    sub = V.take_rows(bad, [4, 7, 0])
    assert V.batch_verify(sub) == [False, True, False] and sub["vk"] == b["vk"] and sub["m"] == 3


def test_the_weighted_form_on_a_holding_batch(holding):
    b, rng = holding, random.Random(0xD500)
    w = [rng.getrandbits(256) for _ in range(ROWS)]
    args = lambda x, sc, weights: (x["vk"], x["proofs"], [s[0] for s in sc], [s[1] for s in sc], x["u"], weights, x["W"])
    sc = V.batch_scalars(b)
    assert V.weighted_ok(*args(b, sc, w)) and V.batch_weighted(b, w, sc)[2]
    for kind in V.KINDS[2:4] + V.KINDS[:1]:
        bad = V.break_rows(b, {5: kind})
        sc_bad = V.batch_scalars(bad)
        assert not V.weighted_ok(*args(bad, sc_bad, w)) and not V.batch_weighted(bad, w, sc_bad)[2], kind
        assert V.weighted_ok(*args(bad, sc_bad, w[:5] + [R] + w[6:])), "a weight of r removes the row"
        assert V.batch_weighted(bad, w[:5] + [2 * R] + w[6:], sc_bad)[2]
    # zeta inside the domain: the equation holds, the boolean is refused while the row is live
    bad = V.break_rows(b, {5: "zeta_in_domain"})
    sc_bad = V.batch_scalars(bad)
    p0, p1, ok = V.batch_weighted(bad, w, sc_bad)
    assert V.weighted_ok(*args(bad, sc_bad, w)) and (p0 + V.TAU * p1) % R == 0 and not ok
    assert V.batch_weighted(bad, w[:5] + [R] + w[6:], sc_bad)[2]


def test_zero_logarithms_and_a_pool_are_honoured_and_the_rows_still_hold():
    rng = random.Random(0xD600)
    pool = [rng.randrange(1, R) for _ in range(16)]
    W, log_e = 3, 2
    P = V.proof_points(W, log_e)
    b = V.holding_batch(rng, 3, W, log_e, 1, 5, pool=pool, vk_zero=(W + 1,), proof_zero={1: [1], 3: [P - 1]})
    assert [x == 0 for x in b["vk"]] == [c == W + 1 for c in range(V.key_points(W))] and all(x in pool for x in b["vk"] if x)
    for i, pr in enumerate(b["proofs"]):
        assert [s for s in range(P) if pr[s] == 0] == {1: [1], 3: [P - 1]}.get(i, []) and all(x in pool for x in pr[1:] if x) and pr[0] not in pool
    assert V.batch_verify(b) == [True] * 5


def test_three_proofs_of_one_circuit_share_a_key():
    rng = random.Random(0xD700)
    first = V.proof_for(rng, LOG_N, 2, 2, 1)
    trio = [first] + [V.proof_for(rng, LOG_N, 2, 2, 1, circuit=first["c"]) for _ in range(2)]
    assert all(p["vk"] == first["vk"] and p["pub"] == first["pub"] for p in trio) and len({tuple(p["proof"]) for p in trio}) == 3
    b = V.batch_of(trio, LOG_N, 2)
    assert V.batch_verify(b) == [True] * 3 and all(check(p, 2) for p in trio)
    assert V.batch_verify(V.break_rows(b, {1: "evaluation"})) == [True, False, True]


def test_the_lease_of_a_chunk_is_the_plan_s():
    """the figures tests/cpp/plonk_verify_plan_test.cpp pins for plonk_verify_plan::fold_chunk_bytes"""
    assert V.fold_chunk_bytes(3, 2, 3, 1) == 2264 and V.fold_chunk_bytes(3, 2, 3, 2) == 4528 and V.fold_chunk_bytes(3, 2, 0, 1) == 8 * (216 + 40 + 3)
