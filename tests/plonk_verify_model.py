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

Inputs are any 256-bit integers, taken mod r.  proof_for is an independent prover in the exponent; holding_batch makes rows that verify at any
shape with no circuit behind them, and break_rows breaks them."""
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


def proof_for(rng, log_n, W, log_e, l, tau=TAU, circuit=None):
    """a circuit with l public inputs, a blinded witness that satisfies it and its proof by the prover's model (O.open_polys, then the two
    quotients by X - zeta and X - zeta w_n), every commitment f(tau) as its logarithm: a dict with vk, proof, evals, pub, shifts, ch.
    circuit: the "c" of an earlier call with the same log_n, W and l -- the proof is then of that circuit, under the same key, with blinders and
    challenges of its own"""
    c = public_circuit(rng, log_n, W, l) if circuit is None else circuit
    assert (c["log_n"], c["W"], c["l"]) == (log_n, W, l)
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


# ---- batches of rows that hold at any shape, with no circuit behind them --------------------------------------------------------------------
KINDS = ("evaluation", "public_input", "t0_is_z", "wzeta_is_womega", "zeta_in_domain")       # the ways break_rows breaks a row


def batch_scalars(b, rows=None):
    """[(k, y, status)] of the rows of a batch (all of them by default)"""
    rows = range(b["m"]) if rows is None else rows
    return [scalars(b["evals"][i], b["pub"][i], b["shifts"], *(b[c][i] for c in CHALLENGES), b["log_n"], b["log_e"]) for i in rows]


def batch_verify(b, sc=None):
    """[the boolean of every row]; sc: batch_scalars(b), where the caller has them"""
    out = []
    for i, (k, y, status) in enumerate(batch_scalars(b) if sc is None else sc):
        c, pi = row(b["vk"], b["proofs"][i], k, b["u"][i])
        out.append(status == 0 and (c - y - TAU * pi) % R == 0)
    return out


def batch_weighted(b, weights, sc=None):
    """(p0, p1, the boolean) of the weighted form: the logarithms of the G1 sides of the two literal pairs, and weighted_ok with the veto of a
    live row (weight != 0 mod r) whose zeta lies in the domain"""
    sc = batch_scalars(b) if sc is None else sc
    ks, ys = [s[0] for s in sc], [s[1] for s in sc]
    p0, p1 = weighted_pairs(b["vk"], b["proofs"], ks, ys, b["u"], weights, b["W"])
    vetoed = any(s[2] and w % R for s, w in zip(sc, weights))
    assert ((p0 + TAU * p1) % R == 0) == weighted_ok(b["vk"], b["proofs"], ks, ys, b["u"], weights, b["W"])
    return p0, p1, (p0 + TAU * p1) % R == 0 and not vetoed


def solve_w0(b, i):
    """slot 0 ([w_0], scalar v != 0) of proof i from C - y = tau pi: the row then holds in the exponent whatever its status says"""
    (k, y, _), = batch_scalars(b, [i])
    K, pr = key_points(b["W"]), b["proofs"][i]
    assert k[K] == b["v"][i] % R != 0
    pr[0] = 0
    c, pi = row(b["vk"], pr, k, b["u"][i])
    pr[0] = (y + TAU * pi - c) * pow(k[K], R - 2, R) % R
    c, pi = row(b["vk"], pr, k, b["u"][i])
    assert (c - y - TAU * pi) % R == 0


def holding_batch(rng, log_n, W, log_e, n_pub, m, pool=None, vk_zero=(), proof_zero=None):
    """m rows under one key that verify in the exponent, at ANY shape -- also where no satisfied witness exists (log_e = 0): evaluations, public
    inputs, shifts and the six challenges are random full-range 256-bit words (v nonzero mod r), the key's logarithms and those of slots
    1 .. P - 1 of every proof are random and nonzero (drawn from `pool`, a list of logarithms, where one is given), and slot 0 of every proof
    is solved last.  vk_zero: key slots whose logarithm is 0 (the identity); proof_zero: {row: slots >= 1} likewise.  A dict: the dimensions,
    vk [2 W + 2], proofs [m][W + E + 3], evals [m][2 W + 1], pub [m][n_pub], shifts [W] and a list [m] under the name of every challenge"""
    wide = lambda: rng.getrandbits(256)
    draw = (lambda: rng.choice(pool)) if pool else (lambda: rng.randrange(1, R))
    K, P = key_points(W), proof_points(W, log_e)
    b = {"log_n": log_n, "W": W, "log_e": log_e, "n_pub": n_pub, "m": m, "shifts": [wide() for _ in range(W)],
         "evals": [[wide() for _ in range(2 * W + 1)] for _ in range(m)], "pub": [[wide() for _ in range(n_pub)] for _ in range(m)]}
    for c in CHALLENGES:
        b[c] = [wide() for _ in range(m)]
    for i in range(m):
        while b["v"][i] % R == 0:
            b["v"][i] = wide()
    b["vk"] = [0 if c in vk_zero else draw() for c in range(K)]
    b["proofs"] = [[0] + [draw() for _ in range(P - 1)] for _ in range(m)]
    for i, slots in (proof_zero or {}).items():
        for s in slots:
            assert 1 <= s < P
            b["proofs"][i][s] = 0
    for i in range(m):
        solve_w0(b, i)
    assert all(batch_verify(b))
    return b


def break_rows(b, where):
    """a copy of a batch with the rows of `where` ({row: one of KINDS}) broken: evaluation 0 + 1; public input 0 + 1 (n_pub > 0); slot [t_0]
    replaced by slot [z]; W_zeta replaced by W_omega; or zeta := w_n^j with [w_0] solved again, so that the row KEEPS holding in the exponent
    and only its status (bit 1) refuses it"""
    out = dict(b)
    for key in ("evals", "pub", "proofs"):
        out[key] = [list(r) for r in b[key]]
    out["zeta"] = list(b["zeta"])
    W, n = b["W"], 1 << b["log_n"]
    for i, kind in where.items():
        assert kind in KINDS
        if kind == "evaluation":
            out["evals"][i][0] = out["evals"][i][0] % R + 1            # + 1 in Fr, and still a 256-bit word
        elif kind == "public_input":
            assert b["n_pub"] > 0
            out["pub"][i][0] = out["pub"][i][0] % R + 1
        elif kind == "t0_is_z":
            out["proofs"][i][W + 1] = out["proofs"][i][W]
        elif kind == "wzeta_is_womega":
            out["proofs"][i][-2] = out["proofs"][i][-1]
        else:
            out["zeta"][i] = pow(T.omega(b["log_n"]), 3 % n, R)
            solve_w0(out, i)
    return out


def take_rows(b, rows):
    """the rows `rows` of a batch as a batch of their own, under the same key"""
    out = dict(b, m=len(rows))
    for key in ("evals", "pub", "proofs") + CHALLENGES:
        out[key] = [b[key][i] for i in rows]
    return out


def batch_of(proofs, log_n, log_e):
    """the batch, as holding_batch lays it out, of proofs that proof_for made for ONE circuit"""
    p = proofs[0]
    assert all(q["vk"] == p["vk"] and q["shifts"] == p["shifts"] for q in proofs), "one key"
    b = {"log_n": log_n, "W": len(p["shifts"]), "log_e": log_e, "n_pub": len(p["pub"]), "m": len(proofs), "shifts": list(p["shifts"]), "vk": list(p["vk"]),
         "proofs": [list(q["proof"]) for q in proofs], "evals": [list(q["evals"]) for q in proofs], "pub": [list(q["pub"]) for q in proofs]}
    for c in CHALLENGES:
        b[c] = [q["ch"][c] for q in proofs]
    return b


def fold_chunk_bytes(W, log_e, n_pub, mc):
    """the lease of a chunk of mc whole proofs of the fold, by the rule of plonk_verify_plan.hpp: per proof 8 n_pub words of denominators and
    inverses, 4 + 8 words a term, 2 (8 + 4) + 16 words for pi's two terms and the two results, and the flags of the chunk -- a byte a term and
    four a proof -- rounded up to a word"""
    t = terms(W, log_e)
    return 8 * (mc * (8 * n_pub + 12 * t + 40) + ((t + 4) * mc + 7) // 8)


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
