"""GPU: every argument error of sylow_hip_kzg_open_all_prepare, sylow_hip_kzg_open_all_batch and its _tuned form -- SYLOW_HIP_E_ARG, no launch,
nothing written (sentinel-filled outputs stay as they were) -- m = 0 with NULL pointers, y_out = NULL accepted, the Python layers' refusals.
And the input contract of tests/test_gpu_input_contract.py for the three: the coordinate words of the SRS and of the table are Fp values
(representatives x + k p give the same outputs), table_inf = NULL is an all-zero flag array.  The rows and the cases are registered in that
file's tables when the suite is collected, so its CPU completeness tests see them."""
import numpy as np
import pytest

import g1_ntt_model as G1M
import kzg_open_all_model as M
import kzg_prove_model as KP
import test_gpu_input_contract as T

E_ARG = -2
SENTINEL = 0x5A5A5A5A5A5A5A5A
LOG_N = 3
TAU = 0xC0FFEE0DDBA11
ROWS = {
    "sylow_hip_kzg_open_all_prepare": T.Row({"srs_g1_xy": T.G1A}),
    "sylow_hip_kzg_open_all_batch": T.Row({"table_xy": T.G1A}, ["table_inf"]),
    "sylow_hip_kzg_open_all_batch_tuned": T.Row({"table_xy": T.G1A}, ["table_inf"]),
}
T.CONTRACT.update(ROWS)
_DATA = []


def data():
    """the monomial SRS of 8 points, its table by the model (no identity in it) and two polynomials"""
    if not _DATA:
        rng = T.Xoshiro(T.SEED + 0x0A)
        srs, sinf = G1M.points(G1M.monomial_logs(TAU, 1 << LOG_N))
        txy, tinf = M.points(M.table_logs(TAU, LOG_N))
        polys = [[rng.u256() for _ in range(1 << LOG_N)] for _ in range(2)]
        assert not sinf.any() and not tinf.any()
        _DATA.append((srs, txy, tinf, polys))
    return _DATA[0]


@T.case("kzg_open_all_prepare")
def _prepare(eng, c, pool, nm):
    dt, dti = eng.kzg_open_all_prepare(c.fp("srs_g1_xy", data()[0]))
    return [np.ascontiguousarray(dt.download().T), dti.download()]


@T.case("kzg_open_all_batch", "kzg_open_all_batch_tuned")
def _open_all(eng, c, pool, nm):
    _, txy, tinf, polys = data()
    return list(eng.kzg_open_all((c.fp("table_xy", txy), c.flag("table_inf", tinf)), KP.poly_words(polys), max_blocks=1 if nm.endswith("_tuned") else -1))


def test_rows_name_real_parameters():
    from sylow_amd import _shapes
    from test_rust_ffi import parse_header
    protos, shapes = parse_header(), _shapes.parse()
    for name, row in ROWS.items():
        assert name in protos and T.CONTRACT[name] is row and name in T.CASES
        assert set(row.fp) | set(row.flags) <= {p[3] for p in protos[name][1]}, name
        assert {p for p, sh in shapes[name][1].items() if sh.optional and sh.dtype == "u8"} == set(row.flags), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_reduces_representatives_and_null_flags(engine, name):
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"
    if name.endswith("prepare"):
        _, txy, tinf, _ = data()
        assert np.array_equal(base[0], txy) and np.array_equal(base[1], tinf)
    else:
        polys = data()[3]
        for j, f in enumerate(polys):
            wxy, winf = M.points(M.proof_logs(f, TAU, LOG_N))
            assert np.array_equal(base[1][j], wxy) and np.array_equal(base[2][j], winf) and KP.ints(base[0][j]) == M.values(f, LOG_N)


@pytest.mark.gpu
def test_argument_errors_write_nothing_and_empty_batch(engine):
    lib = engine.lib
    n, log_n, m = 1 << LOG_N, LOG_N, 2
    srs, txy, tinf, polys = data()
    coeffs = np.ascontiguousarray(KP.poly_words(polys).transpose(0, 2, 1))                 # [m][4][n]
    dsrs, dtab, dti = engine.to_device_soa(srs, 8), engine.to_device_soa(txy, 8), engine.to_device(tinf)
    dc = engine.to_device(coeffs)
    fill_t, fill_y, fill_p = np.full((8, 2 * n), SENTINEL, np.uint64), np.full((m, 4, n), SENTINEL, np.uint64), np.full((m, 8, n), SENTINEL, np.uint64)
    dto, dtoi = engine.to_device(fill_t), engine.to_device(np.full((2 * n,), 7, np.uint8))
    dy, dp, dpi = engine.to_device(fill_y), engine.to_device(fill_p), engine.to_device(np.full((m, n), 7, np.uint8))
    prep = lambda *a: lib.sylow_hip_kzg_open_all_prepare(*a, engine.stream)
    plain = lambda *a: lib.sylow_hip_kzg_open_all_batch(*a, engine.stream)
    tuned = lambda *a: lib.sylow_hip_kzg_open_all_batch_tuned(*a, engine.stream)
    # prepare: log_n out of range, NULL where a pointer is required
    assert prep(dsrs.ptr, -1, dto.ptr, dtoi.ptr) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    assert prep(dsrs.ptr, 28, dto.ptr, dtoi.ptr) == E_ARG
    assert prep(None, log_n, dto.ptr, dtoi.ptr) == E_ARG and prep(dsrs.ptr, log_n, None, dtoi.ptr) == E_ARG and prep(dsrs.ptr, log_n, dto.ptr, None) == E_ARG
    # the batch
    assert plain(dtab.ptr, dti.ptr, dc.ptr, -1, m, dy.ptr, dp.ptr, dpi.ptr) == E_ARG and plain(dtab.ptr, dti.ptr, dc.ptr, 28, m, dy.ptr, dp.ptr, dpi.ptr) == E_ARG
    assert plain(dtab.ptr, dti.ptr, dc.ptr, 28, 0, dy.ptr, dp.ptr, dpi.ptr) == E_ARG        # log_n is checked before m = 0 returns
    assert plain(None, dti.ptr, dc.ptr, log_n, m, dy.ptr, dp.ptr, dpi.ptr) == E_ARG
    assert plain(dtab.ptr, dti.ptr, None, log_n, m, dy.ptr, dp.ptr, dpi.ptr) == E_ARG
    assert plain(dtab.ptr, dti.ptr, dc.ptr, log_n, m, dy.ptr, None, dpi.ptr) == E_ARG
    assert plain(dtab.ptr, dti.ptr, dc.ptr, log_n, m, dy.ptr, dp.ptr, None) == E_ARG
    assert tuned(dtab.ptr, dti.ptr, dc.ptr, log_n, m, 0, dy.ptr, dp.ptr, dpi.ptr) == E_ARG  # max_blocks == 0
    assert tuned(dtab.ptr, dti.ptr, dc.ptr, 28, m, 1, dy.ptr, dp.ptr, dpi.ptr) == E_ARG and tuned(dtab.ptr, dti.ptr, dc.ptr, -1, m, 1, dy.ptr, dp.ptr, dpi.ptr) == E_ARG
    assert plain(dtab.ptr, dti.ptr, dy.ptr, log_n, m, dy.ptr + 8, dp.ptr, dpi.ptr) == E_ARG # y_out inside the coefficients' byte range
    assert plain(dtab.ptr, dti.ptr, dp.ptr + 8, log_n, m, dy.ptr, dp.ptr, dpi.ptr) == E_ARG # pi_xy over the coefficients
    # m = 0: OK, nothing launched, NULL pointers and all
    assert plain(dtab.ptr, dti.ptr, dc.ptr, log_n, 0, dy.ptr, dp.ptr, dpi.ptr) == 0 and plain(None, None, None, log_n, 0, None, None, None) == 0
    assert tuned(None, None, None, 0, 0, 5, None, None, None) == 0
    engine.sync()
    assert np.array_equal(dto.download(), fill_t) and (dtoi.download() == 7).all(), "prepare wrote nothing"
    assert np.array_equal(dy.download(), fill_y) and np.array_equal(dp.download(), fill_p) and (dpi.download() == 7).all(), "the batch wrote nothing"
    assert np.array_equal(dc.download(), coeffs) and np.array_equal(np.ascontiguousarray(dtab.download().T), txy)
    # y_out = NULL is accepted: the proofs are written, y stays as it was
    assert plain(dtab.ptr, None, dc.ptr, log_n, m, None, dp.ptr, dpi.ptr) == 0
    engine.sync()
    assert np.array_equal(dy.download(), fill_y)
    got, flags = dp.download(), dpi.download()
    for j, f in enumerate(polys):
        wxy, winf = M.points(M.proof_logs(f, TAU, LOG_N))
        assert np.array_equal(np.ascontiguousarray(got[j].T), wxy) and np.array_equal(flags[j], winf)


@pytest.mark.gpu
def test_python_layers_refuse(engine):
    import sylow_amd
    from sylow_amd import api
    api.set_engine(engine)
    srs = data()[0]
    with pytest.raises(ValueError, match="power of two"):
        api.KzgProver(api.G1Affine(srs[:6])).open_all([[1] * 6])
    with pytest.raises(ValueError):
        api.KzgProver(api.G1Affine(srs)).open_all([[1] * 4])                                # one coefficient per SRS point
    y, pis = api.KzgProver(api.G1Affine(srs)).open_all(np.zeros((0, 8, 4), dtype=np.uint64))
    assert y.shape == (0, 8, 4) and pis == []
    dtab, dc, dshort, doi, dfew = engine.empty((8, 16)), engine.empty((1, 4, 8)), engine.empty((1, 8, 4)), engine.empty((8,), np.uint8), engine.empty((4,), np.uint8)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="pi_xy holds"):
        engine._call("sylow_hip_kzg_open_all_batch", dtab.ptr, None, dc.ptr, 3, 1, None, dshort.ptr, doi.ptr)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="table_inf holds"):
        engine._call("sylow_hip_kzg_open_all_prepare", dc.ptr, 2, dtab.ptr, dfew.ptr)
