"""A CPU model of the KZG opening of ONE polynomial at SEVERAL points under one proof (sylow_amd/csrc/kzg_points.hip): integer arithmetic
mod r over Python ints, sharing nothing with sylow_amd.  Not collected by pytest.  For the points z_0 .. z_{k-1} of a polynomial f:

    Z = prod (X - z_i)      a_i = 1 / prod_{l != i} (z_i - z_l), inv(0) = 0      q_i = (f - f(z_i)) / (X - z_i)
    q = sum_i a_i q_i       R = sum_i f(z_i) a_i Z / (X - z_i)                    pi = q(tau) G1gen

For distinct points q = f div Z and R = f mod Z (long_division below, which the formula never calls).  A row with points repeated mod r is
DEFINED by the formula under inv(0) = 0: every point that collides with another one gets the weight 0.  Points of the curve are handled by
their DISCRETE LOGARITHMS to the base G1gen under a tau the maker knows; the expected words come from the C oracle's generator multiples
(kzg_prove_model.expected_*).  Every word is taken mod r."""
import os
import re

import kzg_prove_model as KP
from kzg_prove_model import P, R, TOP, ints, limbs  # noqa: F401  (re-exported for the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_WORDS = [0, 1, R - 1, R, R + 1, P, TOP]


def plan_constants():
    """the named constants of sylow_amd/csrc/kzg_points_plan.hpp, read from the source, and the scan's geometry beside them"""
    src = open(os.path.join(ROOT, "sylow_amd", "csrc", "kzg_points_plan.hpp")).read()
    out = dict(KP.plan_constants())
    for name in ("KZGPT_MAX_POINTS", "KZGPT_BLOCK", "KZGPT_ROW_BLOCK"):
        out[name] = int(re.search(r"constexpr (?:int|size_t) " + name + r" = (\d+);", src).group(1))
    out["KZGPT_GRID_CAP"] = 1 << int(re.search(r"constexpr size_t KZGPT_GRID_CAP = \(size_t\)1 << (\d+);", src).group(1))
    terms = re.search(r"constexpr size_t KZGPT_G2_BYTES_PER_TERM = ([\d +]+);", src).group(1)
    out["KZGPT_G2_BYTES_PER_TERM"] = sum(int(t) for t in terms.split("+"))
    return out


def inv0(v):
    v %= R
    return pow(v, R - 2, R) if v else 0


def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % R
    return out


def vanishing(zs):
    """Z = prod (X - z_i), k + 1 coefficients, lowest degree first; monic"""
    out = [1]
    for z in zs:
        out = poly_mul(out, [-z % R, 1])
    return out


def long_division(f, d):
    """(f div d, f mod d) for a monic d: len(f) coefficients of the quotient (padded with zeros), len(d) - 1 of the remainder"""
    assert d[-1] == 1
    rem, k = [c % R for c in f], len(d) - 1
    quo = [0] * len(f)
    for e in range(len(f) - 1, k - 1, -1):
        c = rem[e]
        quo[e - k] = c
        for i, dv in enumerate(d):
            rem[e - k + i] = (rem[e - k + i] - c * dv) % R
    rem = (rem + [0] * k)[:k]
    return quo, rem


def weights(zs):
    """(a_i under inv(0) = 0, distinct): the barycentric weights of one row and whether its points are distinct mod r"""
    zs = [z % R for z in zs]
    den = []
    for i, zi in enumerate(zs):
        d = 1
        for l, zl in enumerate(zs):
            if l != i:
                d = d * (zi - zl) % R
        den.append(d)
    return [inv0(d) for d in den], all(den)


def quotient_points(f, zs):
    """(q, y) of one polynomial by the formula: q = sum_i a_i q_i with q_i from kzg_prove_model's recurrence, y_i = f(z_i); len(q) == len(f)"""
    a, _ = weights(zs)
    q, y = [0] * len(f), []
    for ai, z in zip(a, zs):
        qi, yi = KP.quotient(f, z)
        y.append(yi)
        q = [(s + ai * v) % R for s, v in zip(q, qi)]
    return q, y


def remainder_points(zs, ys):
    """R = sum_i y_i a_i Z / (X - z_i), k coefficients: the interpolant for distinct points, the formula's value otherwise"""
    a, _ = weights(zs)
    Z, k = vanishing(zs), len(zs)
    out = [0] * k
    for ai, z, y in zip(a, zs, ys):
        qi, rem = long_division(Z, [-z % R, 1])
        assert rem == [0]
        c = (y % R) * ai % R
        out = [(s + c * v) % R for s, v in zip(out, qi[:k])]
    return out


def row_holds(c_log, zs, ys, pi_log, tau):
    """the check of one row in the exponent, as the verifier decides it: C - R(tau) = pi Z(tau), and the points distinct"""
    _, distinct = weights(zs)
    rt, zt = KP.evaluate(remainder_points(zs, ys), tau), KP.evaluate(vanishing(zs), tau)
    return distinct and (c_log - rt - pi_log * zt) % R == 0


def expected_open(polys, rows, tau):
    """(y [m][k] ints, pi words [m, 8], pi flags [m]) with pi_j = q_j(tau) G1gen"""
    qs = [quotient_points(f, zs) for f, zs in zip(polys, rows)]
    xy, inf = expected_points([KP.evaluate(q, tau) for q, _ in qs])
    return [y for _, y in qs], xy, inf


def expected_points(logs):
    """generator multiples by the C oracle: (affine words [n, 8], flags [n]), the identity as (0, 1) + its flag"""
    return KP.expected_commit([[v] for v in logs], 0)


def row_words(rows):
    """n rows of k ints (any 256-bit value) -> [n, k, 4] words"""
    return limbs([v for r in rows for v in r]).reshape(len(rows), -1, 4)
