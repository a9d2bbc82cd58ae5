"""GPU: many cells of many KZG blobs checked as one boolean over shared commitments -- the entry points of include/sylow_hip_kzg_cells.h
(kzg_cells.hip).  The four outputs of the fold word for word against tests/kzg_cells_model.py on both forced routes and at three grid caps;
F and P against the oracle's generator products of the model's exponents under the test's known tau; the Gt words against
sylow_hip_kzg_batch_verify_weighted over the rows of sylow_hip_kzg_cosets_reduce_batch with each commitment gathered per row; the loop
open_cosets -> verify, five alterations each rejected alone and accepted again with that row's weight 0; rows out of range, flagged points,
all weights 0 and no row at all.  The order of the rows inside a group is not observable, and nothing here looks for it."""
import random

import numpy as np
import pytest

import kzg_cells_model as M
import kzg_cosets_model as CM
import kzg_prove_model as KP
from groth16_model import g2_gen_mul, ints, limbs
from ntt_model import R

pytestmark = pytest.mark.gpu
TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
U256 = (1 << 256) - 1
IDENTITY = limbs([0, 1]).reshape(8)
SHAPES = [(0, 0), (0, 2), (2, 0), (2, 2), (3, 1), (1, 3), (3, 3)]
_BLOBS = {}


def grouped(sizes, total):
    """keys 0, 1, .. with the given group sizes, the last key taking the rest, shuffled"""
    keys = [k for k, s in enumerate(sizes) for _ in range(s)]
    keys += [len(sizes)] * (total - len(keys))
    random.Random(total).shuffle(keys)
    return keys


def fold_rows(log_c, log_l, n_com, rows, flagged=False):
    """rows of (idx, com_idx, vals, weight) as ints.  Cell c - 1 and commitment n_com - 1 are named by nobody (where there is another);
    from 13 rows on: weights 0, r and >= r, values >= r, a repeated row, rows out of range with the weight 0 mod r -- and with a live weight
    when `flagged`."""
    c, l = 1 << log_c, 1 << log_l
    rng = random.Random(0xCE20 + 1000 * rows + 100 * n_com + 10 * log_c + log_l)
    idx = [rng.randrange(max(c - 1, 1)) for _ in range(rows)]
    com = [rng.randrange(max(n_com - 1, 1)) for _ in range(rows)]
    if (log_c, log_l, rows) == (2, 2, 300):                          # groups that cross the fold after 16 products; the planted rows join the rest
        idx = [c - 1] * 13 + grouped([15, 16, 17], rows - 13)
        com = [n_com - 1] * 13 + grouped([15, 16, 17, 33][:n_com - 1], rows - 13)
    out = [(idx[k], com[k], [rng.randrange(R) for _ in range(l)], rng.randrange(1, 1 << 128)) for k in range(rows)]
    if rows >= 13:
        out[3] = out[3][:3] + (0,)
        out[4] = out[4][:3] + (R,)
        out[5] = out[5][:3] + (R + 7,)
        out[6] = out[6][:2] + ([U256] + [x + R for x in out[6][2][1:]], U256)
        out[7] = out[2]
        out[8] = (c, out[8][1], out[8][2], 0)
        out[9] = (out[9][0], n_com, out[9][2], 2 * R)
        if flagged:
            out[10] = (c + 1, out[10][1], out[10][2], 5)
            out[11] = (out[11][0], 1 << 63, out[11][2], 6)
    return out


def arrays(rows, log_l):
    idx = np.array([r[0] for r in rows], dtype=np.uint64)
    com = np.array([r[1] for r in rows], dtype=np.uint64)
    cells = limbs([x for r in rows for x in r[2]]).reshape(len(rows), 1 << log_l, 4)
    return idx, com, cells, limbs([r[3] for r in rows]).reshape(len(rows), 4)


def check_fold(engine, rows, log_c, log_l, n_com, route, max_blocks, what):
    idx, com, cells, weights = arrays(rows, log_l)
    W, A, r, rz, flag = engine.kzg_cells_fold(idx, com, cells, weights, log_c, log_l, n_com, route=route, max_blocks=max_blocks)
    wW, wr, wrz = M.scalars(rows, log_c, log_l, n_com)
    assert ints(W) == wW, f"{what}: W"
    assert ints(r) == wr and ints(rz) == wrz, f"{what}: r, rz"
    assert ints(A) == M.fold(rows, log_c, log_l, n_com), f"{what}: A"
    assert flag == M.in_range(rows, log_c, n_com), f"{what}: the range flag"


@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_the_fold_is_the_model_on_both_routes(engine, log_c, log_l):
    for n_com in (1, 3, 5):
        for n_rows in (1, 2, 13, 300):
            rows = fold_rows(log_c, log_l, n_com, n_rows)
            check_fold(engine, rows, log_c, log_l, n_com, -1, -1, f"default ({n_com}, {n_rows})")
            for route in (0, 1):
                for cap in (1, 3, -1):
                    check_fold(engine, rows, log_c, log_l, n_com, route, cap, f"route {route} cap {cap} ({n_com}, {n_rows})")


def test_the_planted_groups_cross_the_fold_of_sixteen():
    """CPU side of the inputs"""
    rows = fold_rows(2, 2, 5, 300)
    live = [r for r in rows if M.live(r, 2, 5)]
    by_cell, by_com = [sum(r[0] == i for r in live) for i in range(4)], [sum(r[1] == b for r in live) for b in range(5)]
    assert by_cell[:3] == [15, 16, 17] and by_com[:4] == [15, 16, 17, 33] and len(live) < 300 and by_cell[3] > 33 and by_com[4] > 33
    rows = fold_rows(3, 1, 3, 13)
    assert not any(r[0] == 7 for r in rows) and not any(r[1] == 2 for r in rows), "a cell and a commitment nobody names"
    assert rows[7] == rows[2] and rows[3][3] == 0 and rows[4][3] % R == 0 and rows[5][3] > R and max(rows[6][2]) >= R
    assert M.in_range(rows, 3, 3) and not M.in_range(fold_rows(3, 1, 3, 13, flagged=True), 3, 3)


@pytest.mark.parametrize("log_c,log_l", [(2, 2), (3, 1), (0, 2)])
def test_rows_out_of_range_and_one_cell(engine, log_c, log_l):
    for route in (0, 1):
        check_fold(engine, fold_rows(log_c, log_l, 3, 13, flagged=True), log_c, log_l, 3, route, -1, f"a cleared flag, route {route}")
        one = [(0, b, v, w) for _, b, v, w in fold_rows(log_c, log_l, 3, 40)]
        check_fold(engine, one, log_c, log_l, 3, route, -1, f"every row on one cell, route {route}")
        zero = [r[:3] + (0,) for r in fold_rows(log_c, log_l, 3, 13)]
        check_fold(engine, zero, log_c, log_l, 3, route, -1, f"all weights 0, route {route}")
    W, A, r, rz, flag = engine.kzg_cells_fold(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 1 << log_l, 4), np.uint64), np.zeros((0, 4), np.uint64),
                                              log_c, log_l, 3)
    assert not W.any() and W.shape == (3, 4) and not A.any() and r.shape == (0, 4) and flag


# ---- points: three blobs under a known tau ---------------------------------------------------------------------------------------------
def blobs(engine, log_c, log_l):
    """tau, the SRS prefix, tau^l G2gen, three random blobs with their commitments, cells and proofs as logarithms and as points"""
    key = (log_c, log_l)
    if key not in _BLOBS:
        rng = random.Random(0xCE30 + 16 * log_c + log_l)
        n, l = 1 << (log_c + log_l), 1 << log_l
        fs = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
        srs, sinf = engine.g1_generator_mul(limbs(KP.srs_logs(TAU, n)))
        assert not sinf.any()
        com_logs = [CM.evaluate(f, TAU) for f in fs]
        pi_logs = [CM.proof_logs(f, TAU, log_c, log_l) for f in fs]
        coms = KP.canonical_identity(*engine.g1_generator_mul(limbs(com_logs)))
        pis = KP.canonical_identity(*engine.g1_generator_mul(limbs([p for row in pi_logs for p in row])))
        _BLOBS[key] = dict(fs=fs, srs=srs, srs_l=srs[:l], tau_l=np.asarray(g2_gen_mul([pow(TAU, l, R)])[0], dtype=np.uint64), com_logs=com_logs, pi_logs=pi_logs,
                           coms=coms, pis=(pis[0].reshape(3, -1, 8), pis[1].reshape(3, -1)),
                           cells=[CM.cells(CM.values(f, log_c, log_l), log_c, log_l) for f in fs])
    return _BLOBS[key]


def sample(b, log_c, picks, seed):
    """rows (model tuples), proof logarithms, proof words and flags for (blob, cell) picks with weights of 128 bits"""
    rng = random.Random(seed)
    rows = [(i, j, list(b["cells"][j][i]), rng.randrange(1, 1 << 128)) for j, i in picks]
    return rows, [b["pi_logs"][j][i] for j, i in picks], np.array([b["pis"][0][j][i] for j, i in picks]), np.array([b["pis"][1][j][i] for j, i in picks])


def reduce_points(engine, b, rows, pxy, pinf, log_c, log_l, cxy=None, cinf=None):
    idx, com, cells, weights = arrays(rows, log_l)
    cxy, cinf = (b["coms"][0], b["coms"][1]) if cxy is None else (cxy, cinf)
    return engine.kzg_cells_reduce(b["srs_l"], cxy, idx, com, cells, pxy, weights, log_c, log_l, c_inf=cinf, pi_inf=pinf)


def expect_points(got, F, P, what):
    f, fi, p, pi, _ = got
    for name, xy, inf, log in (("F", f, fi, F), ("P", p, pi, P)):
        wxy, winf = CM.points([log])
        assert bool(inf[0]) == bool(winf[0]) and (inf[0] or np.array_equal(xy[0], wxy[0])), f"{what}: {name}"


@pytest.mark.parametrize("log_c,log_l", [(0, 0), (2, 2), (3, 1), (1, 3)])
def test_f_and_p_are_the_generator_products_of_the_model(engine, log_c, log_l):
    b, c = blobs(engine, log_c, log_l), 1 << log_c
    rng = random.Random(0xCE31)
    for n_rows in (1, 2 * c + 3):
        picks = [(rng.randrange(3), rng.randrange(c)) for _ in range(n_rows)]
        rows, pi_logs, pxy, pinf = sample(b, log_c, picks, 0xCE32 + n_rows)
        rows[0] = rows[0][:2] + ([rows[0][2][0] + 1] + rows[0][2][1:],) + rows[0][3:]          # a wrong value: F is no multiple of P
        F, P = M.reduce(rows, b["com_logs"], pi_logs, TAU, log_c, log_l)
        got = reduce_points(engine, b, rows, pxy, pinf, log_c, log_l)
        expect_points(got, F, P, f"{n_rows} rows")
        assert got[4] and not M.aggregate_holds(rows, b["com_logs"], pi_logs, TAU, log_c, log_l)


@pytest.mark.parametrize("log_c,log_l", [(2, 2), (3, 3), (0, 2)])
def test_gt_words_are_those_of_the_per_row_route(engine, log_c, log_l):
    b, c = blobs(engine, log_c, log_l), 1 << log_c
    rng = random.Random(0xCE33)
    picks = [(rng.randrange(3), rng.randrange(c)) for _ in range(c + 6)]
    for wrong in (False, True):
        rows, _, pxy, pinf = sample(b, log_c, picks, 0xCE34)
        if wrong:
            rows[1] = rows[1][:2] + ([rows[1][2][0] + 1] + rows[1][2][1:],) + rows[1][3:]
        idx, com, cells, weights = arrays(rows, log_l)
        gt, ok, flag = engine.kzg_cells_verify_weighted(b["srs_l"], b["tau_l"], b["coms"][0], idx, com, cells, pxy, weights, log_c, log_l, c_inf=b["coms"][1], pi_inf=pinf)
        gathered, ginf = b["coms"][0][com.astype(np.int64)], b["coms"][1][com.astype(np.int64)]
        cred, cinf, z, in_rng = engine.kzg_cosets_reduce(b["srs_l"], gathered, idx, cells, log_c, log_l, c_inf=ginf)
        want, want_ok = engine.kzg_batch_verify_weighted(b["tau_l"], cred, z, np.zeros_like(z), pxy, weights, c_inf=cinf, pi_inf=pinf)
        assert in_rng.all() and flag and np.array_equal(gt, want) and ok == want_ok == (not wrong)


def test_open_verify_alter_and_mask(engine):
    """open_cosets of three blobs, every cell; the row (F, 0, 0, P) through KzgVerifier; five alterations rejected alone"""
    from sylow_amd import api
    api.set_engine(engine)
    log_c, log_l = 3, 2
    b, c, l = blobs(engine, log_c, log_l), 1 << log_c, 1 << log_l
    y, pxy, pinf = engine.kzg_open_cosets(engine.kzg_open_cosets_prepare(b["srs"], log_l), KP.poly_words(b["fs"]), log_l)
    commits = api.G1Affine(*engine.kzg_commit(b["srs"], KP.poly_words(b["fs"])))
    assert np.array_equal(commits.xy, b["coms"][0])
    verifier = api.KzgCellBatchVerifier(api.G1Affine(b["srs_l"]), api.G2Affine(b["tau_l"]), log_c, log_l)
    rng = random.Random(0xCE35)
    com = [j for j in range(3) for _ in range(c)]
    idx = [i for _ in range(3) for i in range(c)]
    cells = np.array([y[j].reshape(l, c, 4)[:, i] for j in range(3) for i in range(c)])               # value t of cell i at y[i + c t]
    pis = api.G1Affine(pxy.reshape(3 * c, 8), pinf.reshape(3 * c))
    weights = [rng.randrange(1, 1 << 128) for _ in com]
    assert verifier.verify(commits, com, idx, cells, pis, weights)
    assert verifier.verify_line_table(commits, com, idx, cells, pis, weights)
    f, p, ok = verifier.reduce(commits, com, idx, cells, pis, weights)
    zero = np.zeros((1, 4), dtype=np.uint64)
    assert ok and api.KzgVerifier(api.G2Affine(b["tau_l"])).verify((f, zero, zero, p)).all()
    W, A, r, rz, flag = verifier.fold(3, com, idx, cells, weights)
    assert flag and ints(r) == weights and ints(W) == [sum(weights[j * c:(j + 1) * c]) % R for j in range(3)]

    k = 11
    masked = [0 if j == k else w for j, w in enumerate(weights)]

    def rejected_alone(what, commits=commits, com=com, idx=idx, cells=cells, pis=pis):
        assert not verifier.verify(commits, com, idx, cells, pis, weights), what
        assert not verifier.verify_line_table(commits, com, idx, cells, pis, weights), what
        assert verifier.verify(commits, com, idx, cells, pis, masked), f"{what}: accepted again once the row's weight is 0"

    plus = cells.copy()
    plus[k, 1] = limbs([(ints(cells[k, 1:2])[0] + 1) % R])[0]
    rejected_alone("a value", cells=plus)
    other = pis.xy.copy()
    other[k] = pis.xy[k + 1]
    rejected_alone("a proof", pis=api.G1Affine(other, pis.infinity))
    # a commitment of the row's own: a fourth entry that only row k names, holding another blob's commitment
    four = api.G1Affine(np.concatenate([commits.xy, commits.xy[:1]]), np.concatenate([commits.infinity, commits.infinity[:1]]))
    assert com[k] == 1
    rejected_alone("a commitment", commits=four, com=[3 if j == k else v for j, v in enumerate(com)])
    rejected_alone("a cell index", idx=[(i + 1) % c if j == k else i for j, i in enumerate(idx)])
    rejected_alone("a commitment index", com=[2 if j == k else v for j, v in enumerate(com)])


def test_edge_rows(engine):
    log_c, log_l = 2, 2
    b, c = blobs(engine, log_c, log_l), 1 << log_c
    picks = [(j, i) for j in range(3) for i in range(c)]
    rows, pi_logs, pxy, pinf = sample(b, log_c, picks, 0xCE36)
    F, P = M.reduce(rows, b["com_logs"], pi_logs, TAU, log_c, log_l)
    base = reduce_points(engine, b, rows, pxy, pinf, log_c, log_l)
    expect_points(base, F, P, "the batch")
    assert base[4] and base[1][0] == 0 and base[3][0] == 0
    extra = lambda row: (rows + [row], np.concatenate([pxy, pxy[:1]]), np.concatenate([pinf, pinf[:1]]))
    for row, flag in (((c, 0, rows[0][2], 0), True), ((0, 3, rows[0][2], R), True), ((c, 0, rows[0][2], 9), False), ((0, 3, rows[0][2], 9), False),
                      ((1 << 63, 1 << 63, rows[0][2], 9), False)):
        got = reduce_points(engine, b, *extra(row), log_c, log_l)
        assert got[4] == flag and all(np.array_equal(a, w) for a, w in zip(got[:4], base[:4])), f"F, P are those of the batch without the row {row[:2]}"
        idx, com, cells, weights = arrays(extra(row)[0], log_l)
        _, ok, in_rng = engine.kzg_cells_verify_weighted(b["srs_l"], b["tau_l"], b["coms"][0], idx, com, cells, extra(row)[1], weights, log_c, log_l)
        assert ok == flag and in_rng == flag, "is_one = [the identity] AND the range flag"
    # a flagged pi reads as the identity whatever its words hold; a flagged C likewise
    fl = pinf.copy()
    fl[5] = 1
    logs = [0 if j == 5 else v for j, v in enumerate(pi_logs)]
    expect_points(reduce_points(engine, b, rows, pxy, fl, log_c, log_l), *M.reduce(rows, b["com_logs"], logs, TAU, log_c, log_l), "a flagged pi")
    cf = b["coms"][1].copy()
    cf[1] = 1
    expect_points(reduce_points(engine, b, rows, pxy, pinf, log_c, log_l, b["coms"][0], cf),
                  *M.reduce(rows, [0 if j == 1 else v for j, v in enumerate(b["com_logs"])], pi_logs, TAU, log_c, log_l), "a flagged C")
    # all weights 0: identity pairs, the identity of Gt
    zero = [r[:3] + (0,) for r in rows]
    idx, com, cells, weights = arrays(zero, log_l)
    got = reduce_points(engine, b, zero, pxy, pinf, log_c, log_l)
    assert got[1][0] == 1 and got[3][0] == 1 and got[4]
    gt, ok, in_rng = engine.kzg_cells_verify_weighted(b["srs_l"], b["tau_l"], b["coms"][0], idx, com, cells, pxy, weights, log_c, log_l)
    one = np.zeros((1, 48), dtype=np.uint64)
    one[0, 0] = 1
    assert ok and in_rng and np.array_equal(gt, one)
    # rows = 0
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros((0, 1 << log_l, 4), np.uint64), np.zeros((0, 8), np.uint64), np.zeros((0, 4), np.uint64))
    got = engine.kzg_cells_reduce(b["srs_l"], b["coms"][0], *none[:3], none[3], none[4], log_c, log_l)
    assert got[1][0] == 1 and got[3][0] == 1 and got[4] and np.array_equal(got[0][0], IDENTITY) and np.array_equal(got[2][0], IDENTITY)
    gt, ok, in_rng = engine.kzg_cells_verify_weighted(b["srs_l"], b["tau_l"], b["coms"][0], *none[:3], none[3], none[4], log_c, log_l)
    assert ok and in_rng and np.array_equal(gt, one)


def test_argument_errors(engine):
    lib, st = engine.lib, engine.stream
    E_ARG = -2
    log_c, log_l, rows, n_com = 2, 1, 3, 2
    u64 = lambda *shape: engine.to_device(np.zeros(shape, dtype=np.uint64))
    u8 = lambda n: engine.to_device(np.zeros(n, dtype=np.uint8))
    didx, dcom, dvals, dw, dsrs, dtau, dc, dpi = u64(rows), u64(rows), u64(rows, 4, 2), u64(4, rows), u64(8, 2), u64(16), u64(8, n_com), u64(8, rows)
    ow, oa, orr, orz, og, of, ofi, op, opi, ogt, ois = u64(4, n_com), u64(4, 2), u64(4, rows), u64(4, rows), u8(1), u64(8), u8(1), u64(8), u8(1), u64(48), u8(1)
    fold = lambda ix=didx.ptr, cm=dcom.ptr, v=dvals.ptr, w=dw.ptr, lc=log_c, ll=log_l, rt=-1, mb=-1, wo=ow.ptr, ao=oa.ptr, ro=orr.ptr, rz=orz.ptr, g=og.ptr: \
        lib.sylow_hip_kzg_cells_fold_batch_tuned(ix, cm, v, w, lc, ll, rows, n_com, rt, mb, wo, ao, ro, rz, g, st)
    red = lambda s=dsrs.ptr, c=dc.ptr, ix=didx.ptr, pi=dpi.ptr, lc=log_c, ll=log_l, f=of.ptr, fi=ofi.ptr, p=op.ptr, pf=opi.ptr, g=og.ptr: \
        lib.sylow_hip_kzg_cells_reduce_batch(s, c, None, ix, dcom.ptr, dvals.ptr, pi, None, dw.ptr, lc, ll, rows, n_com, f, fi, p, pf, g, st)
    ver = lambda s=dsrs.ptr, t=dtau.ptr, c=dc.ptr, lc=log_c, ll=log_l, gt=ogt.ptr, io=ois.ptr, g=None: \
        lib.sylow_hip_kzg_cells_verify_weighted(s, t, c, None, didx.ptr, dcom.ptr, dvals.ptr, dpi.ptr, None, dw.ptr, lc, ll, rows, n_com, gt, io, g, st)
    for call in (fold, red, ver):
        assert call(lc=-1) == E_ARG and call(ll=-1) == E_ARG and call(lc=14, ll=14) == E_ARG and call(lc=28, ll=0) == E_ARG
        assert b"bad argument" in lib.sylow_hip_last_error()
    assert fold(rt=2) == E_ARG and fold(mb=0) == E_ARG
    assert fold(ix=None) == E_ARG and fold(cm=None) == E_ARG and fold(v=None) == E_ARG and fold(w=None) == E_ARG
    assert fold(wo=None) == E_ARG and fold(ao=None) == E_ARG and fold(ro=None) == E_ARG and fold(rz=None) == E_ARG and fold(g=None) == E_ARG
    assert fold(ro=dw.ptr) == E_ARG and fold(ao=dvals.ptr + 8) == E_ARG and fold(rz=orr.ptr) == E_ARG and fold(wo=oa.ptr) == E_ARG, "overlapping outputs"
    assert red(s=None) == E_ARG and red(c=None) == E_ARG and red(ix=None) == E_ARG and red(pi=None) == E_ARG
    assert red(f=None) == E_ARG and red(fi=None) == E_ARG and red(p=None) == E_ARG and red(pf=None) == E_ARG and red(g=None) == E_ARG
    assert red(f=dpi.ptr) == E_ARG and red(p=of.ptr) == E_ARG and red(fi=og.ptr) == E_ARG
    assert ver(s=None) == E_ARG and ver(t=None) == E_ARG and ver(c=None) == E_ARG and ver(gt=None, io=None) == E_ARG and ver(gt=dtau.ptr) == E_ARG
    assert fold() == 0 and red() == 0 and ver(gt=None) == 0 and ver(io=None, g=og.ptr) == 0
    engine.sync()
