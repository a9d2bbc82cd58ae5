"""The input contract (tests/test_gpu_input_contract.py) for the entry points of the evaluation-form KZG unit: sylow_hip_kzg_open_evals_batch
takes ONE Fp-valued argument, the coordinate words of the Lagrange-basis SRS, and no flag array; sylow_hip_fr_batch_inv and
sylow_hip_kzg_quotient_evals_batch have only Fr-valued arguments and are exempt (their edge words: tests/test_gpu_fr_batch_inv.py,
tests/test_gpu_kzg_evals.py).  The rows and the case are registered in that file's tables when the suite is collected, so its CPU
completeness tests see them.  And every argument error of the two KZG calls: SYLOW_HIP_E_ARG, nothing written; m = 0 is OK."""
import numpy as np
import pytest

import kzg_evals_model as E
import kzg_prove_model as M
import test_gpu_input_contract as T

FR_ONLY = "Fr-valued arguments: tested with their own edge values (test_gpu_fr_batch_inv.py, test_gpu_kzg_evals.py)"
ROWS = {
    "sylow_hip_fr_batch_inv": T.ex(FR_ONLY),
    "sylow_hip_kzg_quotient_evals_batch": T.ex(FR_ONLY),
    "sylow_hip_kzg_open_evals_batch": T.Row({"srs_lagrange_xy": T.G1A}),
}
T.CONTRACT.update(ROWS)
N, LOG_N = T.D, 4                                                  # 64 polynomials of 16 values
E_ARG = -2
SENTINEL = 0x5A5A5A5A5A5A5A5A
_DATA = []


def data():
    if not _DATA:
        import groth16_model as G
        rng = T.Xoshiro(T.SEED + 0x4C)
        n = 1 << LOG_N
        evals = [[rng.u256() for _ in range(n)] for _ in range(N)]
        evals[9] = [evals[9][0] % M.R + M.R * (i % 2) for i in range(n)]      # a constant: the identity among the proofs
        zs = [rng.u256() for _ in range(N)]
        zs[5] = pow(E.omega(LOG_N), 11, M.R)                        # a row inside the domain
        srs, inf = G.g1_gen_mul(E.lagrange_at(LOG_N, 0xC0FFEE0DDBA11))
        assert not inf.any()
        _DATA.append((srs, M.poly_words(evals), M.limbs(zs)))
    return _DATA[0]


@T.case("kzg_open_evals_batch")
def _open(eng, c, pool, nm):
    srs, evals, z = data()
    return list(eng.kzg_open_evals(c.fp("srs_lagrange_xy", srs), evals, z))


def test_rows_name_real_parameters():
    from sylow_amd import _shapes
    from test_rust_ffi import parse_header
    protos, shapes = parse_header(), _shapes.parse()
    for name, row in ROWS.items():
        assert name in protos and T.CONTRACT[name] is row
        if row.exempt:
            assert name not in T.CASES
            continue
        assert set(row.fp) <= {p[3] for p in protos[name][1]}, name
        assert not [p for p, sh in shapes[name][1].items() if sh.optional], name      # no optional array, so no flag argument to try as NULL
        assert name in T.CASES


@pytest.mark.gpu
def test_kzg_open_evals_reduces_representatives(engine):
    name = "sylow_hip_kzg_open_evals_batch"
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"
    assert list(np.flatnonzero(np.asarray(base[-1]))) == [9]       # the constant opens with the identity


@pytest.mark.gpu
def test_argument_errors_write_nothing_and_empty_batch(engine):
    lib = engine.lib
    n, log_n = 8, 3
    fill = np.full((2, 4, n), SENTINEL, dtype=np.uint64)            # two arrays' worth: the halves are adjacent, not overlapping
    de, dq, dz, dy = engine.to_device(fill), engine.to_device(fill), engine.to_device(fill[0]), engine.to_device(fill[0])
    quot = lambda *a: lib.sylow_hip_kzg_quotient_evals_batch(*a, engine.stream)
    assert quot(de.ptr, -1, 1, dz.ptr, dq.ptr, dy.ptr) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    assert quot(de.ptr, 29, 1, dz.ptr, dq.ptr, dy.ptr) == E_ARG
    assert quot(de.ptr, 29, 0, dz.ptr, dq.ptr, dy.ptr) == E_ARG     # log_n is checked before m = 0 returns
    assert quot(None, log_n, 1, dz.ptr, dq.ptr, dy.ptr) == E_ARG and quot(de.ptr, log_n, 1, None, dq.ptr, dy.ptr) == E_ARG
    assert quot(de.ptr, log_n, 1, dz.ptr, None, None) == E_ARG      # either output may be NULL, not both
    size = 32 * n
    for off in (0, 32, size - 8, -(size - 8)):                      # q_out inside evals' byte range, from either side
        base = de.ptr + size if off < 0 else de.ptr
        assert quot(base, log_n, 1, dz.ptr, base + off, dy.ptr) == E_ARG, off
    assert quot(de.ptr, log_n, 2, dz.ptr, de.ptr + size, dy.ptr) == E_ARG      # two polynomials: the second half is inside the range
    assert quot(de.ptr, log_n, 0, dz.ptr, dq.ptr, dy.ptr) == 0 and quot(None, log_n, 0, None, None, None) == 0      # m = 0: OK, nothing launched
    ds, dp, dpi = engine.to_device(np.zeros((8, n), dtype=np.uint64)), engine.to_device(fill[0]), engine.to_device(np.full(8, 7, np.uint8))
    opn = lambda *a: lib.sylow_hip_kzg_open_evals_batch(*a, engine.stream)
    assert opn(ds.ptr, de.ptr, -1, 1, dz.ptr, dy.ptr, dp.ptr, dpi.ptr) == E_ARG and opn(ds.ptr, de.ptr, 29, 1, dz.ptr, dy.ptr, dp.ptr, dpi.ptr) == E_ARG
    assert opn(None, de.ptr, log_n, 1, dz.ptr, dy.ptr, dp.ptr, dpi.ptr) == E_ARG and opn(ds.ptr, None, log_n, 1, dz.ptr, dy.ptr, dp.ptr, dpi.ptr) == E_ARG
    assert opn(ds.ptr, de.ptr, log_n, 1, None, dy.ptr, dp.ptr, dpi.ptr) == E_ARG and opn(ds.ptr, de.ptr, log_n, 1, dz.ptr, None, dp.ptr, dpi.ptr) == E_ARG
    assert opn(ds.ptr, de.ptr, log_n, 1, dz.ptr, dy.ptr, None, dpi.ptr) == E_ARG and opn(ds.ptr, de.ptr, log_n, 1, dz.ptr, dy.ptr, dp.ptr, None) == E_ARG
    assert opn(ds.ptr, de.ptr, log_n, 0, dz.ptr, dy.ptr, dp.ptr, dpi.ptr) == 0
    engine.sync()
    for d, want in ((de, fill), (dq, fill), (dz, fill[0]), (dy, fill[0]), (dp, fill[0])):
        assert np.array_equal(d.download(), want), "nothing written"
    assert (dpi.download() == 7).all()
    # adjacent halves of one allocation do not overlap: the call runs (the sentinel words mod r: a constant polynomial, q = 0)
    assert quot(de.ptr, log_n, 1, dz.ptr, de.ptr + size, dy.ptr) == 0
    engine.sync()
    v = int.from_bytes(np.full(4, SENTINEL, dtype=np.uint64).tobytes(), "little") % M.R
    got = de.download()
    assert np.array_equal(got[0], fill[0]) and not got[1].any()
    assert np.array_equal(dy.download().reshape(-1)[:4], M.limbs([v])[0])      # y is [4][m] with m = 1: the first four words
