"""A CPU model of the batched PLONK verifier (include/sylow_pverify.h).  Not collected by pytest, plain integers only, and it shares nothing
with sylow_amd.  Built on tests/plonk_open_model.py (the evaluations, the scalars ZH, L1, A, B, the polynomials F and z a prover opens),
tests/plonk_quotient_model.py (circuits, witnesses, schoolbook polynomials) and, for the tests that need words, the point helpers of
tests/kzg_model.py and tests/groth16_model.py over the group-law oracle.  A commitment is f(tau) G1gen with the tau the KZG tests use, so the
model works IN THE EXPONENT: a point is its discrete logarithm mod r, and a row (C, pi, y) verifies exactly when C - y = (tau - 0) pi.

    p  = sum_{j<l} pub_j L_j(zeta),  L_j(zeta) = w_n^j ZH inv(n (zeta - w_n^j)), inv(0) = 0
    B' = alpha B zw
    terms, T = 3 W + E + 5:   [q_j]: a_j   [q_M]: a_0 a_1   [q_C]: 1   [sigma_j], j < W - 1: v^(W+1+j)   [sigma_(W-1)]: -beta B'
                              [w_j]: v^(1+j)   [z]: alpha A + alpha^2 L1 + u   [t_e]: -ZH zeta^(e n)   W_zeta: zeta   W_omega: u zeta w_n
    y  = sum_j v^(1+j) a_j + sum_{j<W-1} v^(W+1+j) s_j + u zw - [ p - B' (a_(W-1) + gamma) - alpha^2 L1 ]
    C  = sum_c k_c P_c,   pi = W_zeta + u W_omega,   status bit 1: zeta^n = 1 (then ok is forced to 0)

Inputs are any 256-bit integers, taken mod r."""
import ntt_model as T
import plonk_open_model as O
import plonk_quotient_model as Q

R = O.R
TAU = 0x5EED0FA11CE5 * 0x10001 + 12345           # the tau of tests/test_gpu_kzg_prove.py and tests/test_gpu_plonk_open.py
STATUS_ZETA_IN_DOMAIN = O.STATUS_ZETA_IN_DOMAIN
CHALLENGES = ("beta", "gamma", "alpha", "zeta", "v", "u")


def key_points(W):
    return 2 * W + 2


def proof_points(W, log_e):
    return W + (1 << log_e) + 3


def terms(W, log_e):
    return key_points(W) + proof_points(W, log_e)


def public_circuit(rng, log_n, W, l):
    """Q.circuit(with_pi=True) with the PI values of rows >= l moved into q_C: PI is zero there, and `pub` holds its l values on rows < l"""
    c = Q.circuit(rng, log_n, W, with_pi=True)
    n = 1 << log_n
    assert 0 <= l <= n
    qc, pi = list(c["selectors"][W + 1]), list(c["pi"])
    for i in range(l, n):
        qc[i], pi[i] = (qc[i] + pi[i]) % R, 0
    c["selectors"] = list(c["selectors"][:W + 1]) + [qc]
    c["pi"], c["pub"], c["l"] = pi, pi[:l], l
    return c


def lagrange(j, zeta, log_n):
    """L_j(zeta) by the header's formula (inv(0) = 0: 0, not 1, at zeta = w_n^j)"""
    n, wj = 1 << log_n, pow(T.omega(log_n), j, R)
    return wj * (pow(zeta % R, n, R) - 1) % R * O.inv(n * (zeta - wj)) % R


def pi_eval(pub, zeta, log_n):
    return sum((x % R) * lagrange(j, zeta, log_n) for j, x in enumerate(pub)) % R


def scalars(evals, pub, shifts, beta, gamma, alpha, zeta, v, u, log_n, log_e):
    """(k [T], y, status) of one proof; slot 2 W of evals is not read"""
    W, n, E = len(shifts), 1 << log_n, 1 << log_e
    assert len(evals) == 2 * W + 1 and len(pub) <= n
    beta, gamma, alpha, zeta, v, u = (x % R for x in (beta, gamma, alpha, zeta, v, u))
    ev = [e % R for e in evals]
    a, sg, zw = ev[:W], ev[W:2 * W - 1], ev[2 * W - 1]
    zh, l1, A, B = O.scalars(ev, shifts, beta, gamma, zeta, log_n)
    zn, p, bp = pow(zeta, n, R), pi_eval(pub, zeta, log_n), alpha * B % R * zw % R
    k = (a + [a[0] * a[1] % R, 1] + [pow(v, W + 1 + j, R) for j in range(W - 1)] + [(-beta * bp) % R] + [pow(v, 1 + j, R) for j in range(W)] +
         [(alpha * A + alpha * alpha % R * l1 + u) % R] + [(-zh * pow(zn, e, R)) % R for e in range(E)] + [zeta, u * zeta % R * T.omega(log_n) % R])
    assert len(k) == terms(W, log_e)
    y = (O.folded_value(ev[:2 * W - 1], v, W) + u * zw - (p - bp * (a[W - 1] + gamma) - alpha * alpha % R * l1)) % R
    return k, y, (STATUS_ZETA_IN_DOMAIN if zh == 0 else 0)


def row(vk, proof, k, u):
    """(C, pi) in the exponent from the 2 W + 2 key logarithms, the W + E + 3 proof logarithms and the T scalars"""
    pts = list(vk) + list(proof)
    assert len(pts) == len(k)
    return sum(s * (x % R) for s, x in zip(k, pts)) % R, (proof[-2] + (u % R) * proof[-1]) % R


def verify(vk, proof, evals, pub, shifts, ch, log_n, log_e, tau=TAU):
    """the boolean of one proof; ch: a mapping of the six challenges"""
    k, y, status = scalars(evals, pub, shifts, *(ch[c] for c in CHALLENGES), log_n, log_e)
    c, pi = row(vk, proof, k, ch["u"])
    return status == 0 and (c - y - tau * pi) % R == 0


def weighted_scalars(ks, ys, us, weights, W):
    """the scalars of the weighted form: (shared [2 W + 2] column sums, own [m][W + E + 3], open [m][2], s)"""
    w, K = [x % R for x in weights], key_points(W)
    shared = [sum(r * k[c] for r, k in zip(w, ks)) % R for c in range(K)]
    own = [[r * x % R for x in k[K:]] for r, k in zip(w, ks)]
    return shared, own, [[r, r * (u % R) % R] for r, u in zip(w, us)], sum(r * y for r, y in zip(w, ys)) % R


def weighted_pairs(vk, proofs, ks, ys, us, weights, W, tau=TAU):
    """the G1 sides of the two literal pairs in the exponent: (M1 - s, -M2); the product of the pairings is 1 exactly when M1 - s = tau M2"""
    shared, own, opn, s = weighted_scalars(ks, ys, us, weights, W)
    m1 = (sum(a * b for a, b in zip(shared, vk)) + sum(a * b for row_k, pr in zip(own, proofs) for a, b in zip(row_k, pr))) % R
    m2 = sum(o[0] * pr[-2] + o[1] * pr[-1] for o, pr in zip(opn, proofs)) % R
    return (m1 - s) % R, (-m2) % R


def weighted_ok(vk, proofs, ks, ys, us, weights, W, tau=TAU):
    p0, p1 = weighted_pairs(vk, proofs, ks, ys, us, weights, W, tau)
    return (p0 + tau * p1) % R == 0


def proof_for(rng, log_n, W, log_e, l, tau=TAU):
    """a circuit with l public inputs, a blinded witness that satisfies it and its proof by the prover's model (O.open_polys, then the two
    quotients by X - zeta and X - zeta w_n), every commitment f(tau) as its logarithm: a dict with vk, proof, evals, pub, shifts, ch"""
    c = public_circuit(rng, log_n, W, l)
    n, big = 1 << log_n, 1 << (log_n + log_e)
    ch = {k: rng.randrange(2, R) for k in CHALLENGES}
    wc, zc, pc = Q.witness_polys(c, ch["beta"], ch["gamma"], rng)
    quo, rem = Q.divide_by_vanishing(Q.numerator(c["selectors"], c["sigma"], wc, zc, pc, c["shifts"], ch["beta"], ch["gamma"], ch["alpha"], log_n), log_n)
    assert not any(rem) and not any(quo[big:]), "the witness satisfies the circuit and t has at most N coefficients"
    t, ct = O.padded(quo[:big], big), O.ctable(c["selectors"], c["sigma"], log_n)
    ev, f, z, status = O.open_polys(ct, wc, zc, pc, t, c["shifts"], ch["beta"], ch["gamma"], ch["alpha"], ch["zeta"], ch["v"], log_n, log_e,
                                    max(n, len(zc), len(wc[0])))
    assert status == 0
    q_f, y_f = O.divide_by_linear(f, ch["zeta"])
    q_z, y_z = O.divide_by_linear(z, ch["zeta"] * T.omega(log_n) % R)
    assert y_f == O.folded_value(ev, ch["v"], W) and y_z == ev[2 * W - 1]
    at = lambda poly: Q.p_eval(poly, tau)
    return {"c": c, "ct": ct, "wires": wc, "z": zc, "pi": pc, "t": t, "vk": [at(r) for r in ct], "evals": ev, "pub": list(c["pub"]), "shifts": c["shifts"], "ch": ch,
            "proof": [at(w) for w in wc] + [at(zc)] + [at(t[e * n:(e + 1) * n]) for e in range(1 << log_e)] + [at(q_f), at(q_z)]}


# ---- words for the tests that drive the engine: points from logarithms through the oracle's generator multiples ---------------------------
def points(logs):
    """([k, 8] affine words, [k] flags) of the points with these logarithms; 0 gives the flagged identity"""
    import groth16_model as G
    return G.g1_gen_mul([x % R for x in logs])


def literal_terms(vk_xy, vk_inf, proofs_xy, proofs_inf):
    """the term-major bases of m proofs for g1_lincomb (n_jobs = m, n_terms = T): key point c replicated m times, then slot c of every proof.
    proofs_xy [m, W + E + 3, 8], proofs_inf [m, W + E + 3] -> ([T m, 8], [T m])"""
    import numpy as np
    m = proofs_xy.shape[0]
    xy = np.concatenate([np.repeat(vk_xy, m, axis=0), proofs_xy.transpose(1, 0, 2).reshape(-1, 8)])
    inf = np.concatenate([np.repeat(vk_inf, m), proofs_inf.T.reshape(-1)])
    return np.ascontiguousarray(xy), np.ascontiguousarray(inf)
