"""CPU: the model of the check of many cells of many blobs as one boolean (tests/kzg_cells_model.py).  A by columns -- the keyed sums, the
inverse transform without the twist, the Horner fold in the plan's chunks -- equals sum_k r_k interp_twist(row k), which is the route by rows;
the aggregated identity holds exactly when every live row satisfies the single-point identity of tests/kzg_cosets_model.py; rows out of
range and rows of weight 0 behave as the header says.  Every (log_c, log_l) with log_c + log_l <= 6."""
import random
import re

import pytest

import kzg_cells_model as M
import kzg_cosets_model as CM
from ntt_model import R

TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
SHAPES = [(log_c, log_l) for log_c in range(7) for log_l in range(7 - log_c)]


def batch(log_c, log_l, n_com, n_rows, seed):
    """(rows, commitment logarithms, proof logarithms): valid rows drawn with repetition from n_com random blobs"""
    rng = random.Random(seed)
    c = 1 << log_c
    blobs = [[rng.randrange(R) for _ in range(1 << (log_c + log_l))] for _ in range(n_com)]
    ys = [CM.cells(CM.values(f, log_c, log_l), log_c, log_l) for f in blobs]
    proofs = [CM.proof_logs(f, TAU, log_c, log_l) for f in blobs]
    rows, pis = [], []
    for _ in range(n_rows):
        b, i = rng.randrange(n_com), rng.randrange(c)
        rows.append((i, b, list(ys[b][i]), rng.randrange(1, 1 << 128)))
        pis.append(proofs[b][i])
    return rows, [CM.evaluate(f, TAU) for f in blobs], pis


@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_columns_rows_and_the_definition_agree(log_c, log_l):
    c = 1 << log_c
    rows, coms, pis = batch(log_c, log_l, 3, 2 * c + 3, 0xCE11 + 16 * log_c + log_l)
    rows[0] = (rows[0][0], rows[0][1], [x + R for x in rows[0][2]], rows[0][3] + R)          # words >= r
    rows.append(rows[1])                                                                      # a repeated row
    rows.append((c, 0, rows[2][2], 5))                                                        # no such cell
    rows.append((0, 3, rows[2][2], 7))                                                        # no such commitment
    rows.append((rows[3][0], rows[3][1], rows[3][2], 0))                                      # masked
    A = M.fold(rows, log_c, log_l, 3)
    assert M.fold_columns(rows, log_c, log_l, 3) == A
    if log_l <= 3:                                                                            # Lagrange's formula costs l^3 per row
        want = [0] * (1 << log_l)
        for idx, com, vals, w in rows:
            if idx < c and com < 3:
                want = [(a + w * x) % R for a, x in zip(want, CM.interp_lagrange(vals, idx, log_c, log_l))]
        assert want == A
    one_cell = [(1 % c, b, v, w) for _, b, v, w in rows[:5]]                                  # every row on one cell
    assert M.fold_columns(one_cell, log_c, log_l, 3) == M.fold(one_cell, log_c, log_l, 3)
    assert M.fold_columns([], log_c, log_l, 3) == [0] * (1 << log_l)


@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_the_aggregate_holds_exactly_when_every_live_row_does(log_c, log_l):
    c, l = 1 << log_c, 1 << log_l
    rows, coms, pis = batch(log_c, log_l, 3, c + 5, 0xCE12 + 16 * log_c + log_l)
    rows.append(rows[0])
    pis.append(pis[0])
    assert all(M.row_holds(r, coms, p, TAU, log_c, log_l) for r, p in zip(rows, pis))
    assert M.in_range(rows, log_c, 3) and M.aggregate_holds(rows, coms, pis, TAU, log_c, log_l)
    k = 2
    i, b, vals, w = rows[k]
    altered = {"value": ((i, b, [vals[0] + 1] + vals[1:], w), coms, pis[k]), "proof": (rows[k], coms, (pis[k] + 1) % R),
               "commitment": (rows[k], [x + (j == b) for j, x in enumerate(coms)], pis[k])}
    if c > 1:
        altered["cell index"] = ((i ^ 1, b, vals, w), coms, pis[k])
    altered["commitment index"] = ((i, (b + 1) % 3, vals, w), coms, pis[k])
    for name, (row, cm, pi) in altered.items():
        bad_rows, bad_pis = rows[:k] + [row] + rows[k + 1:], pis[:k] + [pi] + pis[k + 1:]
        holds = [M.row_holds(r, cm, p, TAU, log_c, log_l) for r, p in zip(bad_rows, bad_pis)]
        assert not M.row_holds(row, cm, pi, TAU, log_c, log_l), name
        assert M.aggregate_holds(bad_rows, cm, bad_pis, TAU, log_c, log_l) == all(holds), name
        masked = bad_rows[:k] + [row[:3] + (R,)] + bad_rows[k + 1:]                             # the weight 0 mod r removes the row
        assert M.aggregate_holds(masked, cm, bad_pis, TAU, log_c, log_l) == all(holds[:k] + holds[k + 1:]), name   # a commitment is shared
        assert name == "commitment" or all(holds[:k] + holds[k + 1:])


@pytest.mark.parametrize("log_c,log_l", [(0, 0), (2, 2), (3, 1), (1, 3)])
def test_dropped_and_masked_rows(log_c, log_l):
    c = 1 << log_c
    rows, coms, pis = batch(log_c, log_l, 2, 6, 0xCE13 + log_c)
    base = M.reduce(rows, coms, pis, TAU, log_c, log_l)
    W, r, rz = M.scalars(rows, log_c, log_l, 2)
    for extra, flag in (((c, 0, rows[0][2], 9), False), ((0, 2, rows[0][2], 9), False), ((1 << 63, 1 << 63, rows[0][2], 2 * R), True), ((c, 5, rows[0][2], 0), True)):
        more = rows + [extra]
        assert M.in_range(more, log_c, 2) == flag
        assert M.reduce(more, coms, pis + [12345], TAU, log_c, log_l) == base                  # a dropped row adds nothing to any sum
        assert M.scalars(more, log_c, log_l, 2) == (W, r + [0], rz + [0])
    zero = [row[:3] + (0,) for row in rows]
    assert M.reduce(zero, coms, pis, TAU, log_c, log_l) == (0, 0) and M.aggregate_holds(zero, coms, pis, TAU, log_c, log_l)
    assert M.reduce([], coms, [], TAU, log_c, log_l) == (0, 0) and M.in_range([], log_c, 2)
    assert M.scalars([rows[0]], log_c, log_l, 2)[0][1 - rows[0][1]] == 0                       # a commitment no row names


def test_the_chunks_are_the_plan_s():
    plan = open(CM.PLAN.replace("kzg_cosets_plan", "kzg_cells_plan")).read()
    assert int(re.search(r"constexpr int HORNER_LANES_LOG = (\d+);", plan).group(1)) == M.HORNER_LANES_LOG
    for log_c in range(9):
        chunks = M.horner_chunks(log_c)
        assert len(chunks) == 1 << min(log_c, M.HORNER_LANES_LOG) and sum(size for _, size in chunks) == 1 << log_c
