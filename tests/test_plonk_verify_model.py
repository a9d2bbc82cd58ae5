"""CPU: the model of the batched PLONK verifier (tests/plonk_verify_model.py) on its own.  For a satisfied, blinded witness at log_n = 3,
W = 2 and 3 and l = 0, 1 and n public inputs, the proof comes from the prover's model (plonk_open_model.open_polys and the two quotients);
then verify holds and C - y G1 = (tau - 0) pi holds in the exponent.  After adding 1 to any single evaluation, public input or transcript
challenge, or replacing a proof point by its double, it fails.  With u = 0, tampering W_omega goes unnoticed and tampering W_zeta does not:
that is what u is for.  p equals p_eval of the interpolated PI.

The chunks: a blinded witness of W wires has a quotient of 2 n + 5 (W = 2) or 3 n + 6 (W = 3) coefficients, so E = 1 (log_e = 0) holds no
satisfied instance; the valid proofs run at log_e = 2, the smallest that holds both, and at log_e = 3, where the upper chunks commit to the
identity.  log_e = 0 is covered where no witness is needed: the term count and order below, and the scalars on random words on the device.

u itself is not among the tampered challenges: it is the verifier's own randomness, and a valid proof verifies under every u."""
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
