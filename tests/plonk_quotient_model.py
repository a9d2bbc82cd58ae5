"""A CPU model of PLONK's quotient polynomial (include/sylow_plonk.h).  Not collected by pytest, plain integers only, and it shares nothing
with sylow_amd.  With n = 2^log_n, E = 2^log_e, N = E n, w_N and w_n = w_N^E the roots of tests/ntt_model.py, the coset K = 5 <w_N>,
x_i = 5 w_N^i, W wire columns, the shifts k_j and the permutation columns sigma_j of tests/fr_scan_model.py:

    gate     = q_M w_0 w_1 + sum_j q_j w_j + q_C + PI
    perm     = z(X) prod_j (w_j + beta k_j X + gamma) - z(w_n X) prod_j (w_j + beta sigma_j + gamma)
    boundary = L_1(X) (z(X) - 1)
    t(X)     = [gate + alpha perm + alpha^2 boundary] / (X^n - 1)

Two routes.  SCHOOLBOOK: every polynomial by its coefficients, products by the definition, long division by X^n - 1: (quotient, remainder).
POINTWISE: the route of the device -- the table of the circuit on K, the zero-padded inputs onto K by the transform, the fused element-wise
step, the transform back, and the status from the tail of the result.  Inputs are any 256-bit integers, taken mod r."""
import fr_scan_model as S
import ntt_model as T

R = T.R
SHIFT = 5
WIRES_MAX = 32


def log_big(log_n, log_e):
    assert log_n >= 0 and log_e >= 0 and log_n + log_e <= 28
    return log_n + log_e


def coefficients(values, log_n):
    """the polynomial of degree < n through `values` on <w_n>"""
    return T.ntt_radix2(values, log_n, inverse=True)


def on_coset(coeffs, log_big_n):
    """the values on K of the polynomial with these coefficients (at most N of them), natural order"""
    big = 1 << log_big_n
    assert 1 <= len(coeffs) <= big
    return T.ntt_radix2(list(coeffs) + [0] * (big - len(coeffs)), log_big_n, shift=SHIFT)


def from_coset(values, log_big_n):
    return T.ntt_radix2(values, log_big_n, inverse=True, shift=SHIFT)


def zinv(log_n, log_e):
    """(5^n w_E^k - 1)^-1 for k < E, w_E = w_N^n: X^n - 1 at x_i is entry i mod E"""
    w_e = pow(T.omega(log_big(log_n, log_e)), 1 << log_n, R)
    return [T.inv(pow(SHIFT, 1 << log_n, R) * pow(w_e, k, R) - 1) for k in range(1 << log_e)]


def table(selectors, sigma, log_n, log_e):
    """(rows [2 W + 3][N], zinv [E]): the selectors q_0 .. q_(W-1), q_M, q_C, then sigma_0 .. sigma_(W-1), then L_1, each on K"""
    n, W = 1 << log_n, len(sigma)
    assert len(selectors) == W + 2 and all(len(v) == n for v in list(selectors) + list(sigma))
    rows = [on_coset(coefficients(v, log_n), log_big(log_n, log_e)) for v in list(selectors) + list(sigma) + [[1] + [0] * (n - 1)]]
    return rows, zinv(log_n, log_e)


def degree_bound(log_n, W, len_w, len_z):
    n = 1 << log_n
    return max((len_z - 1) + W * max(len_w - 1, 1), 2 * (len_w - 1) + n - 1, n + len_z - 2)


def args_ok(log_n, log_e, W, len_w, len_z):
    """what the full route accepts: the quotient's degree D - n stays below N"""
    big = 1 << log_big(log_n, log_e)
    return 2 <= W <= WIRES_MAX and 1 <= len_w <= big and 1 <= len_z <= big and degree_bound(log_n, W, len_w, len_z) - (1 << log_n) < big


def quotient_evals(rows, zi, wires_ext, z_ext, pi_ext, shifts, beta, gamma, alpha, log_n, log_e):
    """the fused step of one instance: t_ext [N] from values on K; pi_ext may be None"""
    W, big, E = len(shifts), 1 << log_big(log_n, log_e), 1 << log_e
    w_big = T.omega(log_big(log_n, log_e))
    beta, gamma, alpha = beta % R, gamma % R, alpha % R
    out, x = [], SHIFT
    for i in range(big):
        w = [wires_ext[j][i] % R for j in range(W)]
        gate = (rows[W][i] * w[0] * w[1] + sum(rows[j][i] * w[j] for j in range(W)) + rows[W + 1][i] + (pi_ext[i] if pi_ext is not None else 0)) % R
        a, b = z_ext[i] % R, z_ext[(i + E) % big] % R
        for j in range(W):
            a = a * (w[j] + beta * (shifts[j] % R) * x + gamma) % R
            b = b * (w[j] + beta * rows[W + 2 + j][i] + gamma) % R
        bnd = rows[2 * W + 2][i] * (z_ext[i] - 1) % R
        out.append((gate + alpha * (a - b) + alpha * alpha * bnd) * zi[i % E] % R)
        x = x * w_big % R
    return out


def quotient(rows, zi, wires, z, pi, shifts, beta, gamma, alpha, log_n, log_e):
    """the full route of one instance from coefficients: (t [N], status).  wires [W][len_w], z [len_z], pi [n] or None"""
    W, lb = len(shifts), log_big(log_n, log_e)
    assert args_ok(log_n, log_e, W, len(wires[0]), len(z)) and all(len(w) == len(wires[0]) for w in wires)
    t_ext = quotient_evals(rows, zi, [on_coset(w, lb) for w in wires], on_coset(z, lb), None if pi is None else on_coset(pi, lb), shifts, beta, gamma,
                           alpha, log_n, log_e)
    t = from_coset(t_ext, lb)
    tail = degree_bound(log_n, W, len(wires[0]), len(z)) - (1 << log_n) + 1
    return t, int(any(t[tail:]))


# ---- the schoolbook route --------------------------------------------------------------------------------------------------------------
def p_add(a, b):
    out = [0] * max(len(a), len(b))
    for i, v in enumerate(a):
        out[i] = v % R
    for i, v in enumerate(b):
        out[i] = (out[i] + v) % R
    return out


def p_scale(a, c):
    return [v * c % R for v in a]


def p_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, u in enumerate(a):
        if u % R:
            for k, v in enumerate(b):
                out[i + k] = (out[i + k] + u * v) % R
    return out


def p_eval(a, x):
    y = 0
    for v in reversed(a):
        y = (y * x + v) % R
    return y


def numerator(selectors, sigma, wires, z, pi, shifts, beta, gamma, alpha, log_n):
    """the coefficients of gate + alpha perm + alpha^2 boundary; selectors and sigma as VALUES on <w_n>, wires, z and pi as coefficients"""
    n, W, w_n = 1 << log_n, len(shifts), T.omega(log_n)
    q = [coefficients(v, log_n) for v in selectors]
    sg = [coefficients(v, log_n) for v in sigma]
    l1 = coefficients([1] + [0] * (n - 1), log_n)
    gate = p_add(p_mul(q[W], p_mul(wires[0], wires[1])), q[W + 1])
    for j in range(W):
        gate = p_add(gate, p_mul(q[j], wires[j]))
    if pi is not None:
        gate = p_add(gate, pi)
    a, b = list(z), [v * pow(w_n, k, R) % R for k, v in enumerate(z)]
    for j in range(W):
        a = p_mul(a, p_add(wires[j], [gamma % R, beta * shifts[j] % R]))
        b = p_mul(b, p_add(p_add(wires[j], p_scale(sg[j], beta)), [gamma % R]))
    perm = p_add(a, p_scale(b, R - 1))
    bnd = p_mul(l1, p_add(z, [R - 1]))
    return p_add(gate, p_add(p_scale(perm, alpha % R), p_scale(bnd, alpha * alpha % R)))


def divide_by_vanishing(num, log_n):
    """(quotient, remainder [n]) of num by X^n - 1"""
    n = 1 << log_n
    rem = [v % R for v in num] + [0] * max(0, n - len(num))
    quo = [0] * max(len(rem) - n, 0)
    for k in range(len(rem) - 1, n - 1, -1):
        quo[k - n] = rem[k]
        rem[k - n] = (rem[k - n] + rem[k]) % R
        rem[k] = 0
    return quo, rem[:n]


# ---- instances -------------------------------------------------------------------------------------------------------------------------
def circuit(rng, log_n, W, with_pi=False):
    """a random circuit and a witness that satisfies it: a random copy permutation, wires constant on its cycles, random linear selectors and
    q_M, and q_C (or, with_pi, the public input column) chosen row by row so that the gate holds.  A dict of values on <w_n>."""
    n = 1 << log_n
    shifts = [1, 5, 7, 10, 11, 13, 14, 15, 17, 19, 20, 21, 22, 23, 26, 28, 29, 30, 31, 33, 34, 35, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46][:W]
    mapping = list(range(W * n))
    rng.shuffle(mapping)
    wires = S.satisfying_wires(mapping, W, log_n, rng)
    lin = [[rng.randrange(R) for _ in range(n)] for _ in range(W)]
    qm = [rng.randrange(R) for _ in range(n)]
    free = [rng.randrange(R) if with_pi else 0 for _ in range(n)]
    rest = [(-(qm[i] * wires[0][i] * wires[1][i] + sum(lin[j][i] * wires[j][i] for j in range(W)) + free[i])) % R for i in range(n)]
    qc, pi = (free, rest) if with_pi else (rest, None)
    return {"log_n": log_n, "W": W, "shifts": shifts, "mapping": mapping, "sigma": S.sigma_from_mapping(shifts, log_n, mapping), "wires": wires,
            "selectors": lin + [qm, qc], "pi": pi}


def blind(coeffs, log_n, blinders):
    """a + (b_1 X^(k-1) + .. + b_k) (X^n - 1) for the k blinders, highest power first"""
    n = 1 << log_n
    out = list(coeffs) + [0] * len(blinders)
    for d, b in enumerate(reversed(blinders)):
        out[d] = (out[d] - b) % R
        out[d + n] = (out[d + n] + b) % R
    return out


def witness_polys(c, beta, gamma, rng=None, wires=None):
    """(wire coefficients [W][len_w], z coefficients [len_z], pi coefficients or None) of the circuit's witness (or of `wires`), z from the
    grand product of tests/fr_scan_model.py; rng: blind the wires with two and z with three random values"""
    wv = c["wires"] if wires is None else wires
    zv, total, status = S.permutation(c["wires"], c["sigma"], c["shifts"], beta, gamma, c["log_n"])
    assert (total, status) == (1, 0)
    wc = [coefficients(w, c["log_n"]) for w in wv]
    zc = coefficients(zv, c["log_n"])
    if rng is not None:
        wc = [blind(w, c["log_n"], [rng.randrange(R), rng.randrange(R)]) for w in wc]
        zc = blind(zc, c["log_n"], [rng.randrange(R) for _ in range(3)])
    return wc, zc, None if c["pi"] is None else coefficients(c["pi"], c["log_n"])
