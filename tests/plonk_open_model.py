"""A CPU model of PLONK's closing rounds (include/sylow_popen.h).  Not collected by pytest, plain integers only, and it shares nothing with
sylow_amd.  Built on tests/plonk_quotient_model.py (circuits, witnesses, schoolbook polynomials), tests/ntt_model.py (the roots and the
transform) and tests/fr_scan_model.py (the grand product, through the quotient model).  With n = 2^log_n, E = 2^log_e, N = E n, w_n the
root of the transform, W wire polynomials and z as coefficients, the quotient t as N coefficients in E chunks t_e of n, the circuit's
selectors and sigma as coefficients (the `ctable`), the shifts k_j and the challenges beta, gamma, alpha, zeta, v:

    evaluations   a_j = w_j(zeta), j < W;  s_j = sigma_j(zeta), j < W - 1;  zw = z(zeta w_n);  p = PI(zeta) (0 without public inputs)
    ZH = zeta^n - 1,  L1 = ZH inv(n (zeta - 1)) with inv(0) = 0,  A = prod_j (a_j + beta k_j zeta + gamma),  B = prod_{j<W-1} (a_j + beta s_j + gamma)
    r = a_0 a_1 q_M + sum_j a_j q_j + q_C + p + alpha [A z - B zw (a_(W-1) + beta sigma_(W-1) + gamma)] + alpha^2 L1 (z - 1) - ZH sum_e zeta^(e n) t_e
    F = r + sum_j v^(1+j) w_j + sum_{j<W-1} v^(W+1+j) sigma_j
    status: bit 0 = r(zeta) != 0, bit 1 = zeta^n = 1

Inputs are any 256-bit integers, taken mod r."""
import ntt_model as T
import plonk_quotient_model as Q

R = Q.R
STATUS_R_NOT_ZERO, STATUS_ZETA_IN_DOMAIN = 1, 2


def inv(x):
    return pow(x % R, R - 2, R)               # inv(0) = 0


def ctable(selectors, sigma, log_n):
    """[2 W + 2][n]: the coefficients of q_0 .. q_(W-1), q_M, q_C, then of sigma_0 .. sigma_(W-1), from their values on <w_n>"""
    W = len(sigma)
    assert len(selectors) == W + 2
    return [Q.coefficients(v, log_n) for v in list(selectors) + list(sigma)]


def evaluate(ct, wires, z, pi, zeta, log_n):
    """the 2 W + 1 evaluations of one instance, in the header's order; pi may be None"""
    W = len(wires)
    zeta %= R
    return ([Q.p_eval(w, zeta) for w in wires] + [Q.p_eval(ct[W + 2 + j], zeta) for j in range(W - 1)] +
            [Q.p_eval(z, zeta * T.omega(log_n) % R), Q.p_eval(pi, zeta) if pi is not None else 0])


def scalars(evals, shifts, beta, gamma, zeta, log_n):
    """(ZH, L1, A, B)"""
    W, n = len(shifts), 1 << log_n
    beta, gamma, zeta = beta % R, gamma % R, zeta % R
    a, sg = [e % R for e in evals[:W]], [e % R for e in evals[W:2 * W - 1]]
    zh = (pow(zeta, n, R) - 1) % R
    l1 = zh * inv(n * (zeta - 1)) % R
    A = B = 1
    for j in range(W):
        A = A * (a[j] + beta * (shifts[j] % R) * zeta + gamma) % R
    for j in range(W - 1):
        B = B * (a[j] + beta * sg[j] + gamma) % R
    return zh, l1, A, B


def linearise(ct, wires, z, t, evals, shifts, beta, gamma, alpha, zeta, v, log_n, log_e):
    """(r, F or None, status) of one instance; r has max(n, len_z) coefficients and F max(n, len_z, len_w).  v None: no F (and wires is
    not read)"""
    W, n, E = len(shifts), 1 << log_n, 1 << log_e
    assert len(ct) == 2 * W + 2 and len(t) == n * E and len(evals) == 2 * W + 1
    beta, gamma, alpha, zeta = beta % R, gamma % R, alpha % R, zeta % R
    ev = [e % R for e in evals]
    a, zw, p = ev[:W], ev[2 * W - 1], ev[2 * W]
    zh, l1, A, B = scalars(ev, shifts, beta, gamma, zeta, log_n)
    r = Q.p_scale(ct[W], a[0] * a[1] % R)
    for j in range(W):
        r = Q.p_add(r, Q.p_scale(ct[j], a[j]))
    r = Q.p_add(r, Q.p_add(ct[W + 1], [p]))
    perm = Q.p_add(Q.p_scale(z, A), Q.p_scale(Q.p_add(Q.p_scale(ct[2 * W + 1], beta), [(a[W - 1] + gamma) % R]), (R - B * zw % R) % R))
    r = Q.p_add(r, Q.p_scale(perm, alpha))
    r = Q.p_add(r, Q.p_scale(Q.p_add(z, [R - 1]), alpha * alpha % R * l1 % R))
    zn = pow(zeta, n, R)
    for e in range(E):
        r = Q.p_add(r, Q.p_scale(t[e * n:(e + 1) * n], (R - zh * pow(zn, e, R) % R) % R))
    status = (STATUS_R_NOT_ZERO if Q.p_eval(r, zeta) else 0) | (STATUS_ZETA_IN_DOMAIN if zh == 0 else 0)
    if v is None:
        return r, None, status
    v %= R
    f = list(r)
    for j in range(W):
        f = Q.p_add(f, Q.p_scale(wires[j], pow(v, 1 + j, R)))
    for j in range(W - 1):
        f = Q.p_add(f, Q.p_scale(ct[W + 2 + j], pow(v, W + 1 + j, R)))
    return r, f, status


def folded_value(evals, v, W):
    """sum_j v^(1+j) a_j + sum_{j<W-1} v^(W+1+j) s_j: what F(zeta) is when r(zeta) = 0"""
    return (sum(pow(v, 1 + j, R) * evals[j] for j in range(W)) + sum(pow(v, W + 1 + j, R) * evals[W + j] for j in range(W - 1))) % R


def divide_by_linear(f, x):
    """(quotient, remainder) of f by X - x"""
    q, carry = [0] * max(len(f) - 1, 0), 0
    for k in range(len(f) - 1, -1, -1):
        carry = (f[k] + carry * x) % R
        if k:
            q[k - 1] = carry
    return q, carry


def padded(coeffs, length):
    assert len(coeffs) <= length
    return [c % R for c in coeffs] + [0] * (length - len(coeffs))


def open_polys(ct, wires, z, pi, t, shifts, beta, gamma, alpha, zeta, v, log_n, log_e, len_f):
    """the full route of one instance up to the two polynomials the KZG opening takes: (evals, F padded to len_f, z padded to len_f, status)"""
    ev = evaluate(ct, wires, z, pi, zeta, log_n)
    _, f, status = linearise(ct, wires, z, t, ev, shifts, beta, gamma, alpha, zeta, v, log_n, log_e)
    return ev, padded(f, len_f), padded(z, len_f), status


def numerator_at(q_at, sg_at, a, z_at, zw, p, shifts, beta, gamma, alpha, x, log_n):
    """gate + alpha perm + alpha^2 boundary at the point x from the VALUES there: q_at [W + 2], sg_at [W], a [W] -- the independent route"""
    W, n = len(shifts), 1 << log_n
    gate = (q_at[W] * a[0] * a[1] + sum(q_at[j] * a[j] for j in range(W)) + q_at[W + 1] + p) % R
    u, w = z_at, zw
    for j in range(W):
        u = u * (a[j] + beta * shifts[j] * x + gamma) % R
        w = w * (a[j] + beta * sg_at[j] + gamma) % R
    zh = (pow(x, n, R) - 1) % R
    return (gate + alpha * (u - w) + alpha * alpha * zh * inv(n * (x - 1)) % R * (z_at - 1)) % R


def satisfied(rng, log_n, W, log_e, blinded, with_pi):
    """a circuit, a blinded or plain witness that satisfies it, its challenges and its quotient t [N] by the schoolbook route"""
    c = Q.circuit(rng, log_n, W, with_pi)
    beta, gamma, alpha = rng.randrange(R), rng.randrange(R), rng.randrange(R)
    wc, zc, pc = Q.witness_polys(c, beta, gamma, rng if blinded else None)
    num = Q.numerator(c["selectors"], c["sigma"], wc, zc, pc, c["shifts"], beta, gamma, alpha, log_n)
    quo, rem = Q.divide_by_vanishing(num, log_n)
    big = 1 << (log_n + log_e)
    assert not any(rem) and not any(quo[big:]), "the witness satisfies the circuit and t has at most N coefficients"
    t = padded(quo[:big], big)
    return {"c": c, "ct": ctable(c["selectors"], c["sigma"], log_n), "wires": wc, "z": zc, "pi": pc, "t": t, "beta": beta, "gamma": gamma, "alpha": alpha,
            "log_n": log_n, "log_e": log_e, "W": W}
