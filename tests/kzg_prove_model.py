"""A CPU model of the prover's half of KZG on BN254 under one SRS.  Not collected by pytest, and it shares nothing with sylow_amd: the
quotient is integer arithmetic mod r, and the expected points are generator multiples by a maker who knows tau -- C = f(tau) G1gen and
pi = q(tau) G1gen -- through the C oracle (the point helpers of groth16_model).

    h_len = 0,  h_k = f_k + z h_{k+1};      y = h_0,  q_k = h_{k+1} (k < len - 1),  q_{len-1} = 0      <=>      f(X) - y = (X - z) q(X)

Coefficients and z are any 256-bit integers, taken mod r."""
import os
import re

import numpy as np

import groth16_model as G
from groth16_model import P, R, ints, limbs  # noqa: F401  (re-exported for the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = (1 << 256) - 1


def plan_constants():
    """the named constants of sylow_amd/csrc/kzg_prove_plan.hpp, read from the source"""
    src = open(os.path.join(ROOT, "sylow_amd", "csrc", "kzg_prove_plan.hpp")).read()
    out = {}
    for name in ("KZG_POLY_BLOCK", "KZG_POLY_LANE_COEFFS", "KZG_POLY_CHUNK"):
        out[name] = int(re.search(r"constexpr (?:int|size_t) " + name + r" = (\d+);", src).group(1))
    terms = re.search(r"constexpr size_t KZG_SHORT_BYTES_PER_TERM = ([\d +]+);", src).group(1)
    out["KZG_SHORT_BYTES_PER_TERM"] = sum(int(t) for t in terms.split("+"))
    assert out["KZG_POLY_CHUNK"] == out["KZG_POLY_BLOCK"] * out["KZG_POLY_LANE_COEFFS"]
    return out


def quotient(f, z):
    """(q, y) by the recurrence, len(q) == len(f)"""
    z %= R
    q, h = [0] * len(f), 0
    for k in range(len(f) - 1, -1, -1):
        q[k] = h                                   # h_{k+1}; h_len = 0 puts the zero at q[len - 1]
        h = (f[k] + z * h) % R
    return q, h


def evaluate(f, x):
    acc = 0
    for c in reversed(f):
        acc = (acc * x + c) % R
    return acc


def _suffix_scan(v, mult_of_step, live):
    """Hillis-Steele over the lanes of a block: step s adds mult_of_step(s) * S[t + 2^s]; lanes from `live` on hold zero and are not read"""
    s, off, B = 0, 1, len(v)
    v = list(v)
    while off < B:
        m = mult_of_step(s)
        v = [(v[t] + m * v[t + off]) % R if t + off < live else v[t] for t in range(B)]
        s, off = s + 1, off * 2
    return v


def chunked_quotient(f, z, L, B):
    """the same (q, y) by the decomposition of kzg_prove.hip: a lane owns L consecutive coefficients, a block of B lanes a chunk of L B;
    lane values by Horner, a block suffix scan with multipliers z^(L 2^s), one total per chunk, the carry scan over the totals in tiles of B
    chunks with multipliers z^(L B 2^s) (the running carry enters a tile through its top lane), then per chunk the carry through the top
    lane, the scan again, and each lane's serial walk from the value above it"""
    z %= R
    n, CH = len(f), L * B
    f = [c % R for c in f]
    chunks = (n + CH - 1) // CH

    def lane_values(c):
        out = []
        for t in range(B):
            a, v = c * CH + t * L, 0
            for i in range(L - 1, -1, -1):
                if a + i < n:
                    v = (v * z + f[a + i]) % R
            out.append(v)
        return out

    live_of = lambda c: B if n - c * CH >= CH else (n - c * CH + L - 1) // L
    lane_mult = lambda s: pow(z, L << s, R)
    # pass 1 + the carry level (skipped for one chunk: one launch)
    carry = [0] * chunks                           # carry[c] = H_{c+1}, the value above chunk c
    if chunks > 1:
        totals = [_suffix_scan(lane_values(c), lane_mult, live_of(c))[0] for c in range(chunks)]
        run = 0
        for tile in range((chunks + B - 1) // B - 1, -1, -1):
            v = [totals[tile * B + t] if tile * B + t < chunks else 0 for t in range(B)]
            if tile * B + B < chunks:
                v[B - 1] = (v[B - 1] + run * pow(z, CH, R)) % R
            s = _suffix_scan(v, lambda st: pow(z, CH << st, R), min(B, chunks - tile * B))
            for t in range(B):
                c = tile * B + t
                if 1 <= c < chunks:
                    carry[c - 1] = s[t]
            run = s[0]
    # pass 2
    q, y = [None] * n, None
    for c in range(chunks):
        v, live = lane_values(c), live_of(c)
        if c + 1 < chunks:
            v[B - 1] = (v[B - 1] + carry[c] * lane_mult(0)) % R
        s = _suffix_scan(v, lane_mult, live)
        if c == 0:
            y = s[0]
        for t in range(B):
            a = c * CH + t * L
            if a >= n:
                continue
            h = s[t + 1] if t + 1 < live else (carry[c] if c + 1 < chunks else 0)
            for i in range(L - 1, -1, -1):
                k = a + i
                if k >= n:
                    continue
                if k == n - 1:
                    q[k] = 0
                h = (h * z + f[k]) % R
                if k:
                    q[k - 1] = h
    return q, y


def srs_logs(tau, n):
    out, t = [], 1
    for _ in range(n):
        out.append(t)
        t = t * tau % R
    return out


def srs_points(tau, n):
    """tau^k G1gen, k < n: affine words [n, 8] from the oracle"""
    xy, inf = G.g1_gen_mul(srs_logs(tau, n))
    assert not inf.any()
    return xy


def poly_words(polys):
    """m lists of len ints (any 256-bit value) -> [m, len, 4] words"""
    m = len(polys)
    return limbs([v for f in polys for v in f]).reshape(m, -1, 4)


def expected_commit(polys, tau):
    """f_j(tau) G1gen by the oracle: (affine words [m, 8], flags [m]); a zero value comes back flagged"""
    xy, inf = G.g1_gen_mul([evaluate([c % R for c in f], tau) for f in polys])
    return canonical_identity(xy, inf)


def expected_open(polys, zs, tau):
    """(y ints, pi words [m, 8], pi flags [m]) with pi_j = q_j(tau) G1gen -- q from the recurrence, never from a division"""
    qs = [quotient(f, z) for f, z in zip(polys, zs)]
    xy, inf = G.g1_gen_mul([evaluate(q, tau) for q, _ in qs])
    return [y for _, y in qs], *canonical_identity(xy, inf)


def canonical_identity(xy, inf):
    """the library's identity: (0, 1) + the flag"""
    xy, inf = np.array(xy, dtype=np.uint64), np.asarray(inf).astype(np.uint8)
    xy[inf.astype(bool)] = limbs([0, 1]).reshape(8)
    return xy, inf
