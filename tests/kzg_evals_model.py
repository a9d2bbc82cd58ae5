"""A CPU model of KZG openings from evaluation form on BN254's Fr.  Not collected by pytest, integer arithmetic with Python's pow only, and it
shares nothing with sylow_amd.  With w = w_n (the root of tests/ntt_model.py), n = 2^log_n, f_i = f(w^i) and d_i = z - w^i:

    z outside the domain:   y = (z^n - 1) n^-1 sum_i f_i w^i / d_i,     q_i = (y - f_i) / d_i
    z = w^k:                y = f_k,     q_i = (y - f_i) / d_i (i != k),     q_k = -w^-k sum_(i != k) q_i w^i

and the Lagrange basis of the domain at tau:   L_i(tau) = (tau^n - 1) w^i / (n (tau - w^i)).
Values, z and the elements to invert are any 256-bit integers, taken mod r; inv(0) = 0."""
import os
import re

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
TOP = (1 << 256) - 1
W = pow(5, (R - 1) >> 28, R)
EDGE_WORDS = [0, 1, R - 1, R, R + 1, 2 * R, P, TOP]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_constants():
    """the named constants of sylow_amd/csrc/kzg_evals_plan.hpp, read from the source"""
    src = open(os.path.join(ROOT, "sylow_amd", "csrc", "kzg_evals_plan.hpp")).read()
    out = {name: int(re.search(r"constexpr (?:int|size_t) " + name + r" = (\d+);", src).group(1))
           for name in ("EVALS_BLOCK", "EVALS_LANE_ELEMS", "EVALS_CHUNK", "EVALS_LOG_N_MAX")}
    assert out["EVALS_CHUNK"] == out["EVALS_BLOCK"] * out["EVALS_LANE_ELEMS"]
    return out


def omega(log_n):
    assert 0 <= log_n <= 28
    return pow(W, 1 << (28 - log_n), R)


def inv(x):
    return pow(x % R, R - 2, R)                  # inv(0) = 0


def batch_inv(a):
    """Montgomery's trick with the zero rule: a zero enters the product chain as 1 and comes out as 0; ONE pow for the whole list"""
    a = [v % R for v in a]
    pre, run = [], 1
    for v in a:
        run = run * (v if v else 1) % R
        pre.append(run)
    run = pow(run, R - 2, R)
    out = [0] * len(a)
    for i in range(len(a) - 1, -1, -1):
        if a[i]:
            out[i] = run * (pre[i - 1] if i else 1) % R
            run = run * a[i] % R
    return out


def hit_index(log_n, z):
    """k with z = w^k mod r, or None"""
    z %= R
    if pow(z, 1 << log_n, R) != 1:
        return None
    w, x = omega(log_n), 1
    for k in range(1 << log_n):
        if x == z:
            return k
        x = x * w % R
    raise AssertionError("an n-th root of unity outside <w_n>")


def quotient(evals, log_n, z, k=None):
    """(q values on the domain, y).  k: the index of z in the domain when the caller knows it (saves the search); both formulas run over the
    inverses of batch_inv, as the definitions above"""
    n, w = 1 << log_n, omega(log_n)
    assert len(evals) == n
    f, z = [v % R for v in evals], z % R
    xs, x = [], 1
    for _ in range(n):
        xs.append(x)
        x = x * w % R
    if k is None:
        k = hit_index(log_n, z)
    assert k is None or xs[k] == z
    dinv = batch_inv([z - x for x in xs])        # 0 at the hit
    if k is None:
        y = (pow(z, n, R) - 1) * (R - ((R - 1) >> log_n)) % R * (sum(fi * x % R * di for fi, x, di in zip(f, xs, dinv)) % R) % R
    else:
        y = f[k]
    q = [(y - fi) * di % R for fi, di in zip(f, dinv)]
    if k is not None:
        assert q[k] == 0
        q[k] = -pow(xs[k], R - 2, R) * sum(qi * x for qi, x in zip(q, xs)) % R
    return q, y


def lagrange_at(log_n, tau):
    """[L_i(tau)] for the domain of n = 2^log_n points; tau outside the domain"""
    n, w = 1 << log_n, omega(log_n)
    tau %= R
    c = (pow(tau, n, R) - 1) * pow(n, R - 2, R) % R
    assert c, "tau inside the domain"
    out, x = [], 1
    for _ in range(n):
        out.append(c * x % R * pow(tau - x, R - 2, R) % R)
        x = x * w % R
    return out
