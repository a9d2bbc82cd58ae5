"""The input contract (tests/test_gpu_input_contract.py) for the prover's KZG entry points: sylow_hip_kzg_commit_batch,
sylow_hip_kzg_commit_batch_tuned and sylow_hip_kzg_open_batch take ONE Fp-valued argument, the coordinate words of the SRS, and no flag
array; sylow_hip_kzg_quotient_batch has only Fr-valued arguments and is exempt (its edge words: tests/test_gpu_kzg_prove.py).  The rows and
their cases are registered in that file's tables when the suite is collected, so its CPU completeness tests see them; each runs through the
same check (check_row: the SRS as representatives x + k p) on the short route at 64 polynomials of 24 coefficients."""
import numpy as np
import pytest

import kzg_prove_model as M
import test_gpu_input_contract as T

SRS = {"srs_g1_xy": T.G1A}
ROWS = {
    "sylow_hip_kzg_commit_batch": T.Row(SRS),
    "sylow_hip_kzg_commit_batch_tuned": T.Row(SRS),
    "sylow_hip_kzg_open_batch": T.Row(SRS),
    "sylow_hip_kzg_quotient_batch": T.ex("Fr-valued arguments: tested with their own edge values (test_gpu_kzg_prove.py)"),
}
T.CONTRACT.update(ROWS)
N, LEN = T.D, 24                                                   # 64 polynomials
_DATA = []


def data():
    if not _DATA:
        rng = T.Xoshiro(T.SEED + 0x4B)
        polys = [[rng.u256() for _ in range(LEN)] for _ in range(N)]
        polys[3] = [0] * LEN                                       # the identity among the commitments
        polys[9] = [polys[9][0]] + [M.R] * (LEN - 1)               # a constant: the identity among the proofs
        _DATA.append((M.srs_points(0xC0FFEE0DDBA11, LEN), M.poly_words(polys), M.limbs([rng.u256() for _ in range(N)])))
    return _DATA[0]


@T.case("kzg_commit_batch")
def _commit(eng, c, pool, nm):
    srs, polys, _ = data()
    return list(eng.kzg_commit(c.fp("srs_g1_xy", srs), polys))


@T.case("kzg_commit_batch_tuned")
def _commit_tuned(eng, c, pool, nm):
    srs, polys, _ = data()
    return list(eng.kzg_commit(c.fp("srs_g1_xy", srs), polys, window=8, min_len=LEN + 1))      # pinned to the short route


@T.case("kzg_open_batch")
def _open(eng, c, pool, nm):
    srs, polys, z = data()
    return list(eng.kzg_open(c.fp("srs_g1_xy", srs), polys, z))


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
@pytest.mark.parametrize("name", sorted(n for n, r in ROWS.items() if not r.exempt))
def test_kzg_prove_reduces_representatives(engine, name):
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"
    flags = np.asarray(base[-1])
    want = [3, 9] if "open" in name else [3]                       # the zero polynomial commits and opens with the identity, the constant only opens with it
    assert list(np.flatnonzero(flags)) == want
