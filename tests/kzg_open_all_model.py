"""A CPU model of the KZG proofs of one polynomial at ALL n = 2^log_n points of its domain (kzg_open_all.hip).  Not collected by pytest, and it
shares nothing with sylow_amd.  It works on discrete logarithms, as tests/g1_ntt_model.py does: the SRS point s_t = tau^t G1gen is the
integer tau^t, the identity is 0, and a proof is the integer q_i(tau), turned into a point by the oracle's fixed-base product.

The EXPECTED proofs know no transform: q_i = (f - f(w^i)) / (X - w^i) by synthetic division, evaluated at tau -- nothing is inverted, so a tau
inside the domain is as good as any.  The expected table is the transform of tests/ntt_model.py over the logarithms of x.

convolution() is the route of kzg_open_all.hip stage by stage on the logarithms -- (2n)^-1 f padded to 2n, its Fr transform F, the pointwise
products fused with stage 0 of the inverse transform of 2n points, its stages p >= 1 with the skipped unit twiddles, stage 0 of the forward
transform of n points reading the first n columns with h_(n-1) taken as the identity, its stages p >= 1 -- and counts the products a scalar
multiplication would make."""
import os

import g1_ntt_model as G
import ntt_model as N
from ntt_model import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = os.path.join(ROOT, "sylow_amd", "csrc", "kzg_open_all_plan.hpp")
CUBE_ROOT = pow(5, (R - 1) // 3, R)              # tau^3 = 1, tau != 1
assert CUBE_ROOT != 1 and pow(CUBE_ROOT, 3, R) == 1


def multiplications(log_n):
    """the issue's formula: 2n + (n (log_n - 1) + 1) + ((n / 2)(log_n - 2) + 1), in halves so that log_n = 0 is exact"""
    n = 1 << log_n
    total2 = 4 * n + (2 * n * (log_n - 1) + 2) + (n * (log_n - 2) + 2)
    assert total2 % 2 == 0
    return total2 // 2


def x_logs(tau, log_n):
    """x of the table: x_(2n-1-t) = tau^t for t = 0 .. n - 2, 0 (the identity) everywhere else; s_(n-1) is not used"""
    n = 1 << log_n
    x, p = [0] * (2 * n), 1
    for t in range(n - 1):
        x[2 * n - 1 - t] = p
        p = p * tau % R
    return x


def table_logs(tau, log_n):
    return N.ntt_radix2(x_logs(tau, log_n), log_n + 1)


def values(f, log_n):
    """f(w^i): the forward Fr transform"""
    return N.ntt_radix2([v % R for v in f], log_n)


def proof_logs(f, tau, log_n):
    """q_i(tau) for every i by synthetic division: h_(n-1) = f_(n-1), h_k = f_k + z h_(k+1); q_k = h_(k+1), f(z) = h_0"""
    n, w = 1 << log_n, N.omega(log_n)
    f = [v % R for v in f]
    assert len(f) == n
    out, ys, z = [], [], 1
    for _ in range(n):
        h, q = 0, [0] * n
        for k in range(n - 1, -1, -1):
            q[k] = h                             # h_(k+1)
            h = (f[k] + z * h) % R
        ys.append(h)
        acc = 0
        for k in range(n - 1, -1, -1):
            acc = (acc * tau + q[k]) % R
        out.append(acc)
        z = z * w % R
    assert ys == values(f, log_n)
    return out


def h_logs(f, tau, log_n):
    """the definition: h_b = sum_(t = 0 .. n-2-b) f_(b+1+t) tau^t"""
    n = 1 << log_n
    return [sum((f[b + 1 + t] % R) * pow(tau, t, R) for t in range(n - 1 - b)) % R for b in range(n)]


def _stages(src, log_n, first, inverse, made):
    """stages first .. log_n - 1 of g1_ntt.hip on the logarithms (tests/g1_ntt_model.py: stockham), without a closing scale"""
    n, half, w = 1 << log_n, (1 << log_n) >> 1, N.omega(log_n)
    if inverse:
        w = N.inv(w)
    for p in range(first, log_n):
        ns, dst = 1 << p, [None] * n
        for j in range(half):
            k = j & (ns - 1)
            u, v = src[j], src[j + half]
            if k:
                v = v * pow(w, k * (n // (2 * ns)), R) % R
                made[0] += 1
            o = (j // ns) * 2 * ns + k
            assert dst[o] is None and dst[o + ns] is None
            dst[o], dst[o + ns] = (u + v) % R, (u - v) % R
        assert None not in dst
        src = dst
    return src


def convolution(f, table, log_n):
    """(proof logarithms, h, products made) by the route of kzg_open_all.hip over a table of logarithms"""
    n, L = 1 << log_n, log_n + 1
    assert len(f) == n and len(table) == 2 * n
    c = N.n_inverse(L)
    F = N.ntt_radix2([c * (v % R) % R for v in f] + [0] * n, L)
    made = [0]
    wide = [None] * (2 * n)
    for j in range(n):                           # the fused stage: U = F_j T_j, V = F_(j+n) T_(j+n)
        u, v = F[j] * table[j] % R, F[j + n] * table[j + n] % R
        made[0] += 2
        wide[2 * j], wide[2 * j + 1] = (u + v) % R, (u - v) % R
    wide = _stages(wide, L, 1, True, made)
    h = wide[:n]
    if log_n == 0:
        return [0], [0], made[0]                 # the one proof is h_0 = h_(n-1): the identity
    half, nxt = n // 2, [None] * n
    for j in range(half):                        # stage 0 of the forward transform, h_(n-1) as the identity whatever the array holds
        u, v = h[j], (0 if j + half == n - 1 else h[j + half])
        nxt[2 * j], nxt[2 * j + 1] = (u + v) % R, (u - v) % R
    out = _stages(nxt, log_n, 1, False, made)
    return out, h[:n - 1] + [0], made[0]


def points(logs):
    return G.points(logs)
