"""A CPU model of the check of many cells of many KZG blobs as one boolean over shared commitments (kzg_cells.hip).  Not collected by pytest,
and it shares nothing with sylow_amd.  It works in integers over tests/kzg_cosets_model.py: a commitment is the integer f(tau), a proof the
integer q_i(tau), the identity is 0.

A row is (idx, com_idx, vals, weight).  A row with idx >= c or com_idx >= n_com adds nothing to any sum and clears the range flag unless
its weight is 0 mod r.  fold() is the definition -- A = sum_k r_k interp_twist(row k) -- and fold_columns() the route of the device: the
keyed sums S_i, the inverse transform of each S_i WITHOUT the twist, and the Horner evaluation A[t] = sum_i a_i[t] (w^-t)^i, chunk by chunk
as the plan cuts it."""
import kzg_cosets_model as CM
import ntt_model as N
from ntt_model import R

HORNER_LANES_LOG = 4          # kzg_cells_plan.hpp


def live(row, log_c, n_com):
    idx, com, _, w = row
    return idx < (1 << log_c) and com < n_com and w % R != 0


def in_range(rows, log_c, n_com):
    """cleared by a row that is out of range and whose weight is not 0 mod r"""
    return all(w % R == 0 or (idx < (1 << log_c) and com < n_com) for idx, com, _, w in rows)


def scalars(rows, log_c, log_l, n_com):
    """(W [n_com], r [rows], rz [rows])"""
    v = CM.roots(log_c, log_l)[1]
    W, r, rz = [0] * n_com, [], []
    for row in rows:
        idx, com, _, w = row
        if live(row, log_c, n_com):
            W[com] = (W[com] + w) % R
            r.append(w % R)
            rz.append(w * pow(v, idx, R) % R)
        else:
            r.append(0)
            rz.append(0)
    return W, r, rz


def fold(rows, log_c, log_l, n_com):
    """A = sum_k r_k R_k over the live rows, R_k the interpolant of row k: the definition, and the route by rows"""
    A = [0] * (1 << log_l)
    for row in rows:
        if live(row, log_c, n_com):
            idx, _, vals, w = row
            A = [(a + w * x) % R for a, x in zip(A, CM.interp_twist(vals, idx, log_c, log_l))]
    return A


def keyed_sums(rows, log_c, log_l, n_com):
    """S_i[j] = sum_(k live, idx_k = i) r_k val_k[j]: c arrays of l values, zeros for a cell no row names"""
    S = [[0] * (1 << log_l) for _ in range(1 << log_c)]
    for row in rows:
        if live(row, log_c, n_com):
            idx, _, vals, w = row
            S[idx] = [(s + w * (x % R)) % R for s, x in zip(S[idx], vals)]
    return S


def horner_chunks(log_c):
    lanes_log = min(log_c, HORNER_LANES_LOG)
    chunk = (1 << log_c) >> lanes_log
    return [(q * chunk, chunk) for q in range(1 << lanes_log)]


def fold_columns(rows, log_c, log_l, n_com):
    """the route by columns: the keyed sums, the plain inverse transform of l points of each, the Horner fold in chunks"""
    c, l, n = 1 << log_c, 1 << log_l, 1 << (log_c + log_l)
    w = N.omega(log_c + log_l)
    a = [N.ntt_radix2(s, log_l, inverse=True) for s in keyed_sums(rows, log_c, log_l, n_com)]
    chunks = horner_chunks(log_c)
    assert sorted(i for first, size in chunks for i in range(first, first + size)) == list(range(c))
    A = []
    for t in range(l):
        g = pow(w, (n - t) % n, R)
        total = 0
        for first, size in chunks:
            acc = 0
            for k in reversed(range(size)):
                acc = (acc * g + a[first + k][t]) % R
            total = (total + acc * pow(w, ((n - t) % n) * first % n, R)) % R
        A.append(total)
    return A


def reduce(rows, com_logs, pi_logs, tau, log_c, log_l):
    """(F, P) in exponents: F = sum_b W_b C_b + sum_k rz_k pi_k - A(tau), P = sum_k r_k pi_k"""
    n_com = len(com_logs)
    W, r, rz = scalars(rows, log_c, log_l, n_com)
    A = fold(rows, log_c, log_l, n_com)
    F = (sum(a * b for a, b in zip(W, com_logs)) + sum(a * b for a, b in zip(rz, pi_logs)) - CM.evaluate(A, tau)) % R
    return F, sum(a * b for a, b in zip(r, pi_logs)) % R


def aggregate_holds(rows, com_logs, pi_logs, tau, log_c, log_l):
    """e(F, G2gen) e(-P, tau^l G2gen) == 1 in exponents: the row (F, z = 0, y = 0, P) of the single-point check under tau^l G2gen"""
    F, P = reduce(rows, com_logs, pi_logs, tau, log_c, log_l)
    return CM.single_point_holds(F, 0, P, tau, log_l)


def row_holds(row, com_logs, pi_log, tau, log_c, log_l):
    idx, com, vals, _ = row
    cred, z = CM.reduced_row(com_logs[com], idx, vals, tau, log_c, log_l)
    return CM.single_point_holds(cred, z, pi_log, tau, log_l)
