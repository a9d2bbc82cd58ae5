"""A CPU model of the KZG proofs of one polynomial on EVERY COSET of its domain (kzg_cosets.hip): n = c l points, c = 2^log_c cosets of
l = 2^log_l points, coset i = { w^(i + c j) : j < l } the roots of X^l - v^i, v = w^l.  Not collected by pytest, and it shares nothing with
sylow_amd.  It works on discrete logarithms, as tests/kzg_open_all_model.py does: the SRS point s_t = tau^t G1gen is the integer tau^t, the
identity is 0, and a proof is the integer q_i(tau), turned into a point by the oracle's fixed-base product.

The EXPECTED proofs know no transform: q_i = f div (X^l - v^i) by plain long division, evaluated at tau -- nothing is inverted, so a tau inside
the domain is as good as any.  The expected interpolant is Lagrange's formula in integers.

convolution() is the route of kzg_cosets.hip array by array and stage by stage on the logarithms -- the l residue arrays (2c)^-1 f_(a + l j)
padded to 2c, their Fr transforms, the product-sums of each plane fused with stage 0 of the inverse transform of 2c points, the fold of the
planes, the stages p >= 1, stage 0 of the forward transform of c points with h_(c-1) taken as the identity, its stages -- and counts the
products a scalar multiplication would make."""
import os

import kzg_open_all_model as OA
import ntt_model as N
from ntt_model import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = os.path.join(ROOT, "sylow_amd", "csrc", "kzg_cosets_plan.hpp")
CUBE_ROOT = OA.CUBE_ROOT


def multiplications(log_c, log_l):
    """2n products, then what the transforms of 2c and of c points make: (c (log_c - 1) + 1) + ((c / 2)(log_c - 2) + 1), in halves"""
    c, n = 1 << log_c, 1 << (log_c + log_l)
    total2 = 4 * n + (2 * c * (log_c - 1) + 2) + (c * (log_c - 2) + 2)
    assert total2 % 2 == 0
    return total2 // 2


def roots(log_c, log_l):
    """(w, v = w^l, u = w^c)"""
    w = N.omega(log_c + log_l)
    return w, pow(w, 1 << log_l, R), pow(w, 1 << log_c, R)


def coset(i, log_c, log_l):
    w = N.omega(log_c + log_l)
    return [pow(w, i + (j << log_c), R) for j in range(1 << log_l)]


def values(f, log_c, log_l):
    return N.ntt_radix2([v % R for v in f], log_c + log_l)


def cells(y, log_c, log_l):
    """cells[i][j] = y[i + c j]"""
    return [[y[i + (j << log_c)] for j in range(1 << log_l)] for i in range(1 << log_c)]


def divide(f, i, log_c, log_l):
    """(q, rem) with f = q (X^l - v^i) + rem by long division, top coefficient first"""
    n, l = 1 << (log_c + log_l), 1 << log_l
    vi = pow(roots(log_c, log_l)[1], i, R)
    rem, q = [x % R for x in f], [0] * n
    assert len(rem) == n
    for k in range(n - 1, l - 1, -1):
        q[k - l] = rem[k]
        rem[k - l] = (rem[k - l] + vi * rem[k]) % R
        rem[k] = 0
    return q, rem[:l]


def evaluate(p, x):
    acc = 0
    for v in reversed(p):
        acc = (acc * x + v) % R
    return acc


def proof_logs(f, tau, log_c, log_l):
    """q_i(tau) for every coset, by long division; the remainders are checked against the values on the coset"""
    out, y = [], values(f, log_c, log_l)
    for i in range(1 << log_c):
        q, rem = divide(f, i, log_c, log_l)
        assert [evaluate(rem, x) for x in coset(i, log_c, log_l)] == cells(y, log_c, log_l)[i]
        out.append(evaluate(q, tau))
    return out


def h_logs(f, tau, log_c, log_l):
    """the definition: h_t = sum_(k < n - (t+1) l) f_(k + (t+1) l) tau^k"""
    n, l = 1 << (log_c + log_l), 1 << log_l
    return [sum((f[k + (t + 1) * l] % R) * pow(tau, k, R) for k in range(n - (t + 1) * l)) % R for t in range(1 << log_c)]


def x_logs(tau, a, log_c, log_l):
    """x^(a)_(2c-1-u) = tau^(a + l u) for u = 0 .. c - 2, 0 (the identity) everywhere else"""
    c, l = 1 << log_c, 1 << log_l
    x = [0] * (2 * c)
    for u in range(c - 1):
        x[2 * c - 1 - u] = pow(tau, a + l * u, R)
    return x


def table_logs(tau, log_c, log_l):
    return [N.ntt_radix2(x_logs(tau, a, log_c, log_l), log_c + 1) for a in range(1 << log_l)]


def convolution(f, table, log_c, log_l, planes_log=0):
    """(proof logarithms, h, products made) by the route of kzg_cosets.hip over a table of logarithms, with 2^planes_log planes"""
    c, l, L = 1 << log_c, 1 << log_l, log_c + 1
    assert len(f) == c * l and len(table) == l and all(len(t) == 2 * c for t in table) and 0 <= planes_log <= log_l
    s = N.n_inverse(L)
    F = [N.ntt_radix2([s * (f[a + l * j] % R) % R for j in range(c)] + [0] * c, L) for a in range(l)]
    made = [0]
    planes, per = 1 << planes_log, l >> planes_log
    owned = sorted(a for p in range(planes) for a in range(p * per, (p + 1) * per))
    assert owned == list(range(l))                                   # the slices partition the residues
    buf = []
    for p in range(planes):                                          # the fused stage, one plane at a time
        plane = [None] * (2 * c)
        for j in range(c):
            u = v = 0
            for a in range(p * per, (p + 1) * per):
                u = (u + F[a][j] * table[a][j]) % R
            for a in range(p * per, (p + 1) * per):
                v = (v + F[a][j + c] * table[a][j + c]) % R
            made[0] += 2 * per
            plane[2 * j], plane[2 * j + 1] = (u + v) % R, (u - v) % R
        buf.append(plane)
    wide = [sum(plane[q] for plane in buf) % R for q in range(2 * c)]        # the fold
    wide = OA._stages(wide, L, 1, True, made)
    h = wide[:c]
    if log_c == 0:
        return [0], [0], made[0]                                     # the one proof is h_0 = h_(c-1): the identity
    half, nxt = c // 2, [None] * c
    for j in range(half):                                            # stage 0 of the forward transform, h_(c-1) as the identity
        u, v = h[j], (0 if j + half == c - 1 else h[j + half])
        nxt[2 * j], nxt[2 * j + 1] = (u + v) % R, (u - v) % R
    out = OA._stages(nxt, log_c, 1, False, made)
    return out, h[:c - 1] + [0], made[0]


def interp_lagrange(vals, i, log_c, log_l):
    """the coefficients of the polynomial of degree below l through (x_j, vals_j), x = coset i mod c: Lagrange's formula in integers"""
    l = 1 << log_l
    xs = coset(i % (1 << log_c), log_c, log_l)
    out = [0] * l
    for j in range(l):
        num, den = [1], 1
        for t in range(l):
            if t != j:
                num = [(a - xs[t] * b) % R for a, b in zip([0] + num, num + [0])]
                den = den * (xs[j] - xs[t]) % R
        k = (vals[j] % R) * N.inv(den) % R
        for e, a in enumerate(num):
            out[e] = (out[e] + k * a) % R
    return out


def interp_twist(vals, i, log_c, log_l):
    """r_k = l^-1 w^(-ik) sum_j val_j u^(-jk): the inverse transform of l points, then the twist"""
    w = N.omega(log_c + log_l)
    r = N.ntt_radix2([v % R for v in vals], log_l, inverse=True)
    g = N.inv(pow(w, i % (1 << log_c), R))
    return [r[k] * pow(g, k, R) % R for k in range(1 << log_l)]


def reduced_row(c_log, i, vals, tau, log_c, log_l):
    """(C - R(tau), z = v^i) in exponents"""
    return (c_log - evaluate(interp_twist(vals, i, log_c, log_l), tau)) % R, pow(roots(log_c, log_l)[1], i % (1 << log_c), R)


def single_point_holds(cred, z, pi_log, tau, log_l):
    """e(cred + z pi, G2gen) e(-pi, tau^l G2gen) == 1 in exponents"""
    return (cred + z * pi_log - pi_log * pow(tau, 1 << log_l, R)) % R == 0


def points(logs):
    return OA.points(logs)
