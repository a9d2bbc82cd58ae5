"""GPU: the recovery of a KZG polynomial from any half of the cells of its domain -- the entry points of include/sylow_hip_kzg_recover.h
(kzg_recover.hip) -- word for word against the model of tests/kzg_recover_model.py (the five steps in plain integers, itself checked against
long-hand evaluation and interpolation by tests/test_kzg_recover_model.py), and closed into a loop with the prover and the verifier of
the cells: open_cosets of a blob, half the cells dropped, recover_cells_and_proofs, KzgCosetVerifier.verify.  The blob, the masks and the
model's answers of a shape are made once per module and shared; nothing changes them.

The masks of a shape: nothing missing; one cell; exactly c / 2 as the first half, as the odd indices and at random; c / 2 + 1 (status 1).
Missing cells hold random 256-bit words, and some held values are written as v + r."""
import random

import numpy as np
import pytest

import kzg_prove_model as KP
import kzg_recover_model as M
from helpers import ints, limbs
from kzg_recover_model import R

pytestmark = pytest.mark.gpu
U256 = (1 << 256) - 1
TAU = 0x1F3C0A5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
# (9, 0) takes the vanishing kernel across a block and a staging round; (7, 6) is the 128 x 64 shape of a real blob
SHAPES = [(1, 0), (0, 1), (1, 1), (2, 2), (3, 1), (5, 3), (9, 0), (7, 6)]
MASKS = ["none", "one", "first_half", "odd", "random_half", "too_many"]
_CASES = {}


def mask_of(kind, rng, c):
    miss = {"none": [], "one": [rng.randrange(c)], "first_half": range(c // 2), "odd": range(1, c, 2), "random_half": rng.sample(range(c), c // 2),
            "too_many": rng.sample(range(c), c // 2 + 1)}[kind]
    miss = set(miss)
    return [0 if i in miss else 1 for i in range(c)]


def filled(rng, y, present, how="random"):
    """y with the words of the missing cells replaced"""
    c = len(present)
    junk = {"zero": lambda: 0, "ones": lambda: U256, "random": lambda: rng.randrange(1 << 256)}[how]
    return [v if present[j % c] else junk() for j, v in enumerate(y)]


def case(log_c, log_l):
    """the blob f with its values y, and per mask: (present, y with junk in the missing cells, the model's (status, coefficients))"""
    key = (log_c, log_l)
    if key not in _CASES:
        rng = random.Random(0x2EC0 + 32 * log_c + log_l)
        c, n = 1 << log_c, 1 << (log_c + log_l)
        f = [rng.randrange(R) for _ in range(n // 2)] + [0] * (n // 2)
        y = M.fft(f, log_c + log_l)
        rows = {}
        for kind in MASKS:
            present = mask_of(kind, rng, c)
            yy = filled(rng, y, present)
            rows[kind] = (present, yy, M.recover(yy, present, log_c, log_l))
        _CASES[key] = dict(f=f, y=y, rows=rows)
    return _CASES[key]


def run(engine, log_c, log_l, ys, presents, want_y=True):
    return engine.kzg_recover(KP.poly_words(ys), np.array(presents, dtype=np.uint8), log_c, log_l, want_y=want_y)


def check_rows(engine, log_c, log_l, kinds, what):
    c = case(log_c, log_l)
    rows = [c["rows"][k] for k in kinds]
    coeffs, y, status = run(engine, log_c, log_l, [r[1] for r in rows], [r[0] for r in rows])
    n = 1 << (log_c + log_l)
    assert coeffs.shape == (len(kinds), n, 4) and y.shape == coeffs.shape and status.shape == (len(kinds),)
    for j, (kind, (present, yy, (wst, wf))) in enumerate(zip(kinds, rows)):
        assert int(status[j]) == wst, f"{what}: the status of {kind}"
        assert ints(coeffs[j]) == wf, f"{what}: the coefficients of {kind}"
        if kind == "too_many":
            assert wst == M.TOO_FEW and not coeffs[j].any() and not y[j].any()
        elif log_c >= 1:
            assert wst == M.OK and wf == c["f"] and ints(y[j]) == c["y"], f"{what}: every cell of {kind} restored"
    return coeffs, y, status


def test_the_model_s_cases_are_what_they_claim():
    """CPU side of the inputs"""
    for log_c, log_l in SHAPES[:6]:
        c, cc = case(log_c, log_l), 1 << log_c
        for kind in MASKS:
            present, yy, (st, f) = c["rows"][kind]
            missing = cc - sum(present)
            assert missing == {"none": 0, "one": 1, "too_many": cc // 2 + 1}.get(kind, cc // 2), (kind, log_c)
            assert st == (M.TOO_FEW if missing > cc // 2 else M.OK)
            assert any(yy[j] != c["y"][j] for j in range(len(yy))) == (missing > 0)       # junk in the missing cells


@pytest.mark.parametrize("m", [1, 3, 5])
@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_against_the_model(engine, log_c, log_l, m):
    """a different mask per row; y_out is the forward transform of coeffs_out"""
    from sylow_amd import api
    api.set_engine(engine)
    groups = [[k] for k in MASKS] if m == 1 else [MASKS[:3], MASKS[3:]] if m == 3 else [MASKS[:5], MASKS[1:]]
    for kinds in groups:
        coeffs, y, status = check_rows(engine, log_c, log_l, kinds, f"m = {m}")
        assert np.array_equal(y, api.ntt(coeffs))
        again = run(engine, log_c, log_l, [case(log_c, log_l)["rows"][k][1] for k in kinds], [case(log_c, log_l)["rows"][k][0] for k in kinds], want_y=False)
        assert again[1] is None and np.array_equal(again[0], coeffs) and np.array_equal(again[2], status)


@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_a_changed_value_is_detected_below_half_and_is_another_blob_at_half(engine, log_c, log_l):
    c, cc, n = case(log_c, log_l), 1 << log_c, 1 << (log_c + log_l)
    rng = random.Random(0x2EC1 + 32 * log_c + log_l)
    kinds = [k for k in MASKS[:5] if any(c["rows"][k][0])]           # c = 1: a row that misses its one cell has no value to change
    ys, presents, wants = [], [], []
    for kind in kinds:
        present, yy, _ = c["rows"][kind]
        j = rng.choice([j for j in range(n) if present[j % cc]])
        yy = list(yy)
        yy[j] = (yy[j] + 1) % R
        ys.append(yy); presents.append(present); wants.append(M.recover(yy, present, log_c, log_l))
    coeffs, y, status = run(engine, log_c, log_l, ys, presents)
    for j, kind in enumerate(kinds):
        wst, wf = wants[j]
        missing = cc - sum(presents[j])
        if log_c >= 1:                                               # c = 1 has no half to miss: every changed value is caught
            assert wst == (M.INCONSISTENT if missing < cc // 2 else M.OK), kind
        if wst == M.OK:
            assert wf != c["f"] and not any(wf[n // 2:]), kind       # the model's other polynomial
        assert int(status[j]) == wst and ints(coeffs[j]) == wf, kind
        assert ints(y[j]) == M.fft(wf, log_c + log_l), kind


@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_the_words_of_missing_cells_and_multiples_of_r_change_no_byte(engine, log_c, log_l):
    c, cc = case(log_c, log_l), 1 << log_c
    rng = random.Random(0x2EC2 + 32 * log_c + log_l)
    kinds = ["one", "odd", "random_half", "too_many"]
    presents = [c["rows"][k][0] for k in kinds]
    base = run(engine, log_c, log_l, [c["rows"][k][1] for k in kinds], presents)
    for how in ("zero", "ones", "random"):
        got = run(engine, log_c, log_l, [filled(rng, c["y"], p, how) for p in presents], presents)
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), how
    lifted = [[v + (1 + rng.randrange(5)) * R if p[j % cc] else v for j, v in enumerate(c["rows"][k][1])] for k, p in zip(kinds, presents)]
    lifted = [[v if v <= U256 else v - R for v in row] for row in lifted]
    assert any(v >= R for row, p in zip(lifted, presents) for j, v in enumerate(row) if p[j % cc])
    got = run(engine, log_c, log_l, lifted, presents)
    assert all(np.array_equal(a, b) for a, b in zip(got, base)), "v + j r"
    flags = [[(7 * i + 1) % 256 or 1 if p else 0 for i, p in enumerate(row)] for row in presents]      # any non-zero byte holds a cell
    got = run(engine, log_c, log_l, [c["rows"][k][1] for k in kinds], flags)
    assert all(np.array_equal(a, b) for a, b in zip(got, base)), "mask bytes other than 1"


@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_vanishing_values_against_the_model(engine, log_c, log_l):
    c = case(log_c, log_l)
    presents = [c["rows"][k][0] for k in MASKS]
    zd, zc, status = engine.kzg_recover_vanish(np.array(presents, dtype=np.uint8), log_c, log_l)
    assert zd.shape == (len(MASKS), 1 << log_c, 4) and zc.shape == zd.shape
    for j, present in enumerate(presents):
        wd, wc, wst = M.vanish(present, log_c, log_l)
        assert (ints(zd[j]), ints(zc[j]), int(status[j])) == (wd, wc, wst), MASKS[j]
    one = engine.kzg_recover_vanish(np.array(presents[4], dtype=np.uint8), log_c, log_l)
    assert np.array_equal(one[0][0], zd[4]) and np.array_equal(one[1][0], zc[4]) and int(one[2][0]) == int(status[4])


def test_argument_errors_and_the_empty_batch(engine):
    lib, st = engine.lib, engine.stream
    E_ARG, SENTINEL = -2, 0x5A5A5A5A5A5A5A5A
    log_c, log_l, m = 2, 2, 2
    c = case(log_c, log_l)
    n, cc = 16, 4
    fill = lambda *shape: engine.to_device(np.full(shape, SENTINEL, dtype=np.uint64))
    flags = lambda count: engine.to_device(np.full(count, 7, dtype=np.uint8))
    dy = engine.to_device(np.ascontiguousarray(KP.poly_words([c["rows"]["one"][1], c["rows"]["odd"][1]]).transpose(0, 2, 1)))
    dp = engine.to_device(np.array([c["rows"]["one"][0], c["rows"]["odd"][0]], dtype=np.uint8))
    out_c, out_y, out_s, out_zd, out_zc = fill(m, 4, n), fill(m, 4, n), flags(m), fill(m, 4, cc), fill(m, 4, cc)
    rec = lambda y=dy.ptr, p=dp.ptr, lc=log_c, ll=log_l, mm=m, co=out_c.ptr, yo=out_y.ptr, s=out_s.ptr: lib.sylow_hip_kzg_recover_batch(y, p, lc, ll, mm, co, yo, s, st)
    van = lambda p=dp.ptr, lc=log_c, ll=log_l, mm=m, zd=out_zd.ptr, zc=out_zc.ptr, s=out_s.ptr: lib.sylow_hip_kzg_recover_vanish_batch(p, lc, ll, mm, zd, zc, s, st)
    for call in (rec, van):
        assert call(lc=-1) == E_ARG and call(ll=-1) == E_ARG and call(lc=0, ll=0) == E_ARG and call(lc=13, ll=0) == E_ARG and call(lc=12, ll=16) == E_ARG
        assert call(lc=0, ll=28) == E_ARG and call(lc=-1, ll=2) == E_ARG and call(p=None) == E_ARG and call(s=None) == E_ARG
        assert b"bad argument" in lib.sylow_hip_last_error()
    assert rec(y=None) == E_ARG and rec(co=None) == E_ARG
    assert rec(co=dy.ptr) == E_ARG and rec(co=dy.ptr + 8) == E_ARG and rec(yo=dy.ptr) == E_ARG and rec(yo=out_c.ptr) == E_ARG and rec(yo=out_c.ptr + 32 * n) == E_ARG
    assert rec(s=dp.ptr) == E_ARG and rec(s=out_c.ptr + 5) == E_ARG and rec(s=out_y.ptr) == E_ARG and rec(co=dp.ptr) == E_ARG, "outputs overlapping inputs or each other"
    assert van(zd=None) == E_ARG and van(zc=None) == E_ARG
    assert van(zd=out_zc.ptr) == E_ARG and van(zc=out_zd.ptr + 8) == E_ARG and van(s=out_zd.ptr) == E_ARG and van(s=dp.ptr + 1) == E_ARG and van(zd=dp.ptr) == E_ARG
    # the empty batch: OK, nothing launched, nothing written, whatever the pointers are
    assert rec(mm=0) == 0 and van(mm=0) == 0
    assert lib.sylow_hip_kzg_recover_batch(None, None, log_c, log_l, 0, None, None, None, st) == 0
    assert lib.sylow_hip_kzg_recover_vanish_batch(None, log_c, log_l, 0, None, None, None, st) == 0
    engine.sync()
    for dev in (out_c, out_y, out_zd, out_zc):
        assert (dev.download() == SENTINEL).all(), "nothing written"
    assert (out_s.download() == 7).all(), "nothing written"
    coeffs, y, status = engine.kzg_recover(np.zeros((0, n, 4), dtype=np.uint64), np.zeros((0, cc), dtype=np.uint8), log_c, log_l)
    assert coeffs.shape == (0, n, 4) and y.shape == (0, n, 4) and status.shape == (0,)
    assert rec(yo=None) == 0                                          # and the call as it is meant, y_out left out
    engine.sync()
    assert ints(np.ascontiguousarray(out_c.download().transpose(0, 2, 1))[0]) == c["f"] and list(out_s.download()) == [0, 0]


def test_the_api_takes_indices_and_cells(engine):
    from sylow_amd import api
    api.set_engine(engine)
    log_c, log_l = 3, 1
    c, cc, l = case(log_c, log_l), 8, 2
    cell = lambda i: [c["y"][i + cc * t] for t in range(l)]
    rec = api.KzgCellRecovery(log_c, log_l)
    idx = [6, 1, 3, 4]
    polys, status = rec.recover(idx, [cell(i) for i in idx])                                          # one blob, rows of integers
    assert polys.shape == (1, 16, 4) and list(status) == [0] and ints(polys[0]) == c["f"]
    many = [[0, 1, 2, 3, 4, 5, 6, 7], [7, 5, 3, 1], [2, 5, 7]]
    polys, status = rec.recover(many, [np.array([limbs(cell(i)) for i in ix]) for ix in many])       # three blobs, words
    assert list(status) == [0, 0, 1] and ints(polys[0]) == c["f"] and ints(polys[1]) == c["f"] and not polys[2].any()
    for bad in ([0, 1, 2, 8], [0, 1, 1, 2]):
        with pytest.raises(ValueError):
            rec.recover(bad, [cell(i % cc) for i in bad])
    with pytest.raises(ValueError):
        api.KzgCellRecovery(13, 0)
    with pytest.raises(ValueError):
        api.KzgCellRecovery(0, 0)


@pytest.mark.parametrize("log_c,log_l", [(2, 2), (3, 1)])
def test_the_loop_open_drop_recover_prove_verify(engine, log_c, log_l):
    """open_cosets of a random blob, half the cells dropped, recover_cells_and_proofs: every returned (cell, proof) verifies against the
    ORIGINAL commitment"""
    from groth16_model import g2_gen_mul
    from sylow_amd import api
    api.set_engine(engine)
    cc, l, n = 1 << log_c, 1 << log_l, 1 << (log_c + log_l)
    rng = random.Random(0x2EC3 + 32 * log_c + log_l)
    srs, sinf = engine.g1_generator_mul(limbs(KP.srs_logs(TAU, n)))
    assert not sinf.any()
    prover = api.KzgProver(api.G1Affine(srs))
    blobs = [[rng.randrange(R) for _ in range(n // 2)] + [0] * (n // 2) for _ in range(3)]
    commits = prover.commit(blobs)
    cells, proofs = prover.open_cosets(blobs, log_l)
    held = [sorted(rng.sample(range(cc), cc // 2)), list(range(cc // 2, cc)), sorted(rng.sample(range(cc), cc // 2 - 1))]
    status, got_cells, got_proofs = prover.recover_cells_and_proofs(held, [cells[j, ix] for j, ix in enumerate(held)], log_l)
    assert list(status) == [0, 0, 1] and got_proofs[2] is None and not got_cells[2].any()
    assert np.array_equal(got_cells[:2], cells[:2])
    tau_l = np.asarray(g2_gen_mul([pow(TAU, l, R)])[0], dtype=np.uint64)
    verifier = api.KzgCosetVerifier(api.G1Affine(srs[:l]), api.G2Affine(tau_l), log_c, log_l)
    for j in range(2):
        assert np.array_equal(got_proofs[j].xy, proofs[j].xy) and np.array_equal(got_proofs[j].infinity, proofs[j].infinity)
        cs = api.G1Affine(np.repeat(commits.xy[j:j + 1], cc, 0), np.repeat(commits.infinity[j:j + 1], cc, 0))
        assert verifier.verify(cs, list(range(cc)), got_cells[j], got_proofs[j]).all()
    wrong = api.G1Affine(np.repeat(commits.xy[1:2], cc, 0), np.repeat(commits.infinity[1:2], cc, 0))
    assert not verifier.verify(wrong, list(range(cc)), got_cells[0], got_proofs[0]).any()
