"""The input contract (tests/test_gpu_input_contract.py) for the entry points of the Fr transform: sylow_hip_fr_ntt_batch and
sylow_hip_fr_ntt_batch_tuned have only Fr-valued arguments and are exempt (their edge words: tests/test_gpu_ntt.py);
sylow_hip_kzg_commit_evals_batch takes ONE Fp-valued argument, the coordinate words of the SRS, and no flag array.  The rows and the case are
registered in that file's tables when the suite is collected, so its CPU completeness tests see them; the case runs through the same check
(check_row: the SRS as representatives x + k p) at 64 arrays of 32 values."""
import numpy as np
import pytest

import kzg_prove_model as M
import test_gpu_input_contract as T

FR_ONLY = "Fr-valued arguments: tested with their own edge values (test_gpu_ntt.py)"
ROWS = {
    "sylow_hip_fr_ntt_batch": T.ex(FR_ONLY),
    "sylow_hip_fr_ntt_batch_tuned": T.ex(FR_ONLY),
    "sylow_hip_kzg_commit_evals_batch": T.Row({"srs_g1_xy": T.G1A}),
}
T.CONTRACT.update(ROWS)
N, LEN = T.D, 32                                                   # 64 arrays on the domain of 32 points
_DATA = []


def data():
    if not _DATA:
        rng = T.Xoshiro(T.SEED + 0x4E)
        evals = [[rng.u256() for _ in range(LEN)] for _ in range(N)]
        evals[5] = [0, M.R] * (LEN // 2)                           # the zero polynomial: the identity among the commitments
        _DATA.append((M.srs_points(0xC0FFEE0DDBA11, LEN), M.poly_words(evals)))
    return _DATA[0]


@T.case("kzg_commit_evals_batch")
def _commit_evals(eng, c, pool, nm):
    srs, evals = data()
    return list(eng.kzg_commit_evals(c.fp("srs_g1_xy", srs), evals))


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
def test_kzg_commit_evals_reduces_representatives(engine):
    name = "sylow_hip_kzg_commit_evals_batch"
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"
    assert list(np.flatnonzero(np.asarray(base[-1]))) == [5]
