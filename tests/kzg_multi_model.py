"""A CPU model of the folded KZG openings (sylow_amd/csrc/kzg_multi.hip): integer arithmetic mod r over Python ints, sharing nothing with
sylow_amd.  Not collected by pytest.  The m polynomials fall into G groups of consecutive polynomials given by their G + 1 offsets; group g
is opened at z_g and folded under gamma_g; with i the index of polynomial j inside its group and 0^0 = 1:

    F_g = sum_j gamma_g^i f_j      y_j = f_j(z_g)      pi_g = commit((F_g - F_g(z_g)) / (X - z_g))
    C_F,g = sum_j gamma_g^i C_j    y_F,g = sum_j gamma_g^i y_j

Points are handled by their DISCRETE LOGARITHMS to the base G1gen under a tau the maker knows (C_j = f_j(tau), pi_g = q_F,g(tau)); the
expected words come from the C oracle's generator multiples (kzg_prove_model.expected_*).  Every word is taken mod r."""
import os
import re

import kzg_prove_model as KP
from kzg_prove_model import P, R, TOP, ints, limbs  # noqa: F401  (re-exported for the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_WORDS = [0, 1, R - 1, R, R + 1, P, TOP]


def plan_constants():
    """the named constants of sylow_amd/csrc/kzg_multi_plan.hpp, read from the source"""
    src = open(os.path.join(ROOT, "sylow_amd", "csrc", "kzg_multi_plan.hpp")).read()
    out = {}
    for name in ("KZGM_BLOCK", "KZGM_LINCOMB_TILE", "KZGM_LINCOMB_FLUSH", "KZGM_GRID_Y_CAP", "KZGM_OFFSET_ARGS"):
        out[name] = int(re.search(r"constexpr (?:int|size_t) " + name + r" = (\d+);", src).group(1))
    for name in ("KZGM_GRID_X_CAP", "KZGM_LANE_GRID_CAP"):
        out[name] = 1 << int(re.search(r"constexpr size_t " + name + r" = \(size_t\)1 << (\d+);", src).group(1))
    terms = re.search(r"constexpr size_t KZGM_BYTES_PER_SLOT = ([\d +]+);", src).group(1)
    out["KZGM_BYTES_PER_SLOT"] = sum(int(t) for t in terms.split("+"))
    assert out["KZGM_LINCOMB_TILE"] == out["KZGM_BLOCK"]
    return out


def offsets(sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + s)
    return out


def groups_of(gs):
    """[(g, range of its polynomials)]"""
    return [(g, range(gs[g], gs[g + 1])) for g in range(len(gs) - 1)]


def powers(gamma, gs):
    """out_j = gamma_g^i, i = j - gs[g]; pow(0, 0) = 1"""
    out = []
    for g, js in groups_of(gs):
        out += [pow(gamma[g] % R, j - js.start, R) for j in js]
    return out


def lincomb(a, w, gs):
    """out_g[k] = sum_{j in g} w_j a_j[k] mod r; zeros for an empty group"""
    ln = len(a[0]) if a else 0
    return [[sum((w[j] % R) * (a[j][k] % R) for j in js) % R for k in range(ln)] for _, js in groups_of(gs)]


def fold(polys, gs, gamma):
    return lincomb(polys, powers(gamma, gs), gs)


def open_multi(polys, gs, z, gamma):
    """(y [m], F [G][len], q_F [G][len], y_F [G]): the values, the folded polynomials, their quotients at z_g and their values there"""
    y = [None] * len(polys)
    for g, js in groups_of(gs):
        for j in js:
            y[j] = KP.evaluate([c % R for c in polys[j]], z[g] % R)
    F = fold(polys, gs, gamma)
    qs = [KP.quotient(F[g], z[g]) for g in range(len(gs) - 1)]
    return y, F, [q for q, _ in qs], [v for _, v in qs]


def combine_logs(c_logs, y, gs, gamma):
    """(log of C_F,g, y_F,g) from the discrete logarithms of the C_j (None or 0: the identity) and the claimed values"""
    pw = powers(gamma, gs)
    cf = [sum(pw[j] * (c_logs[j] or 0) for j in js) % R for _, js in groups_of(gs)]
    yf = [sum(pw[j] * (y[j] % R) for j in js) % R for _, js in groups_of(gs)]
    return cf, yf


def row_holds(cf_log, z, yf, pi_log, tau):
    """the KZG relation of one row in the exponent: C_F - y_F = (tau - z) pi"""
    return (cf_log - yf - (tau - z) * pi_log) % R == 0


def expected_points(logs):
    """generator multiples by the C oracle: (affine words [n, 8], flags [n]), the identity as (0, 1) + its flag"""
    return KP.expected_commit([[v] for v in logs], 0)
