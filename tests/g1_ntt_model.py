"""A CPU model of the radix-2 transform over G1 points.  Not collected by pytest, and it shares nothing with sylow_amd.  It works on discrete
logarithms: for P_k = s_k G1gen the transform's output is NTT(s)_i G1gen, so the model is the integer transform of tests/ntt_model.py over
the s_k (no coset shift), then the oracle's fixed-base product, identities made canonical: (0, 1) + the flag.

stockham() is the transform stage by stage as g1_ntt.hip addresses it -- butterfly j < n/2 of stage p, Ns = 2^p, reads j and j + n/2, writes
(j div Ns) 2 Ns + (j mod Ns) and that + Ns, with the twiddle w^((j mod Ns) n / (2 Ns)) (negated exponent for the inverse), and NO product
where j mod Ns = 0 -- on the logarithms; it counts the products it makes."""
import os
import re

import numpy as np

import ntt_model as N
from ntt_model import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = os.path.join(ROOT, "sylow_amd", "csrc", "g1_ntt_plan.hpp")


def plan_constants():
    """the named integer constants of sylow_amd/csrc/g1_ntt_plan.hpp, read from the source"""
    src = open(PLAN).read()
    return {name: int(value) for name, value in re.findall(r"constexpr (?:int|size_t) (G1_NTT_[A-Z_]+) = (\d+);", src)}


def logs_ntt(s, log_n, inverse=False, direct=False):
    return (N.ntt_direct if direct else N.ntt_radix2)(list(s), log_n, inverse=inverse)


def multiplications(log_n):
    """the plan's formula: sum over the stages p >= 1 of (n / 2)(1 - 2^-p)"""
    half = (1 << log_n) >> 1
    return sum(half - (half >> p) for p in range(1, log_n))


def stockham(s, log_n, inverse=False):
    """(the transform of the logarithms by the kernel's stages, the number of twiddle products made); the inverse ends with n^-1"""
    n, half, w = 1 << log_n, (1 << log_n) >> 1, N.omega(log_n)
    assert len(s) == n
    if inverse:
        w = N.inv(w)
    src, made = [v % R for v in s], 0
    for p in range(log_n):
        ns, dst = 1 << p, [None] * n
        for j in range(half):
            k = j & (ns - 1)
            u, v = src[j], src[j + half]
            if k:
                v = v * pow(w, k * (n // (2 * ns)), R) % R
                made += 1
            o = (j // ns) * 2 * ns + k
            assert dst[o] is None and dst[o + ns] is None
            dst[o], dst[o + ns] = (u + v) % R, (u - v) % R
        assert None not in dst
        src = dst
    if inverse:
        src = [v * N.n_inverse(log_n) % R for v in src]
    return src, made


def points(logs):
    """s_k G1gen by the oracle: (affine words [n, 8], flags [n]), the identity as (0, 1) + its flag"""
    import groth16_model as G
    import kzg_prove_model as KP
    return KP.canonical_identity(*G.g1_gen_mul([v % R for v in logs]))


def expected(logs, log_n, inverse=False):
    """the transform of the points s_k G1gen: (words [n, 8], flags [n])"""
    return points(logs_ntt(logs, log_n, inverse))


def monomial_logs(tau, n):
    out, t = [], 1
    for _ in range(n):
        out.append(t)
        t = t * tau % R
    return out
