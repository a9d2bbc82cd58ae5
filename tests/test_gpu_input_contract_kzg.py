"""The input contract (tests/test_gpu_input_contract.py) for the four KZG entry points: sylow_hip_kzg_fold_batch,
sylow_hip_kzg_verify_batch, sylow_hip_kzg_verify_line_table_batch and sylow_hip_kzg_batch_verify_weighted.  The rows and their cases are
registered in that file's tables when the suite is collected, so its CPU completeness tests see them; each runs through the same check
(check_row: every Fp argument -- the coordinate words of C, pi and tau_g2 -- as representatives x + k p, NULL flags against all-zero flags)
at n = 64 on valid openings with a few invalid rows.  The line table is an opaque device array: it is built from the canonical tau_g2."""
import numpy as np
import pytest

import kzg_model as M
import test_gpu_input_contract as T

OPENINGS = {"c_xy": T.G1A, "pi_xy": T.G1A}
FLAGS = ["c_inf", "pi_inf"]
ROWS = {
    "sylow_hip_kzg_fold_batch": T.Row(OPENINGS, FLAGS),
    "sylow_hip_kzg_verify_batch": T.Row({"tau_g2_xy": T.G2A, **OPENINGS}, FLAGS),
    "sylow_hip_kzg_verify_line_table_batch": T.Row(OPENINGS, FLAGS),     # tau_table: opaque device digits from g2_line_table
    "sylow_hip_kzg_batch_verify_weighted": T.Row({"tau_g2_xy": T.G2A, **OPENINGS}, FLAGS),
}
T.CONTRACT.update(ROWS)
N = T.D                                                            # 64
_INST = []


def instance():
    if not _INST:
        _INST.append(M.plant(M.make_instance(N, seed=0xC1), {5: "c_negated", 20: "pi_swapped", 33: "y_plus_one"}))
    return _INST[0]


def _opening_args(c, g):
    return (c.fp("c_xy", g.c), g.z_words(), g.y_words(), c.fp("pi_xy", g.pi), c.flag("c_inf", T._flags(N, 1, 13)), c.flag("pi_inf", T._flags(N, 2, 17)))


@T.case("kzg_fold_batch")
def _fold(eng, c, pool, nm):
    return list(eng.kzg_fold(*_opening_args(c, instance())))


@T.case("kzg_verify_batch")
def _verify(eng, c, pool, nm):
    g = instance()
    return [eng.kzg_verify(c.fp("tau_g2_xy", g.tau_g2), *_opening_args(c, g))]


@T.case("kzg_verify_line_table_batch")
def _verify_table(eng, c, pool, nm):
    g = instance()
    return [eng.kzg_verify_line_table(eng.g2_line_table(g.tau_g2), *_opening_args(c, g))]


@T.case("kzg_batch_verify_weighted")
def _weighted(eng, c, pool, nm):
    g = instance()
    w = M.limbs([(0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1) for i in range(N)])
    cx, z, y, pi, ci, pii = _opening_args(c, g)
    gt, one = eng.kzg_batch_verify_weighted(c.fp("tau_g2_xy", g.tau_g2), cx, z, y, pi, w, ci, pii)
    return [gt, np.array([one])]


def test_rows_name_real_parameters():
    from sylow_amd import _shapes
    from test_rust_ffi import parse_header
    protos, shapes = parse_header(), _shapes.parse()
    for name, row in ROWS.items():
        assert name in protos and T.CONTRACT[name] is row
        assert set(row.fp) | set(row.flags) <= {p[3] for p in protos[name][1]}, name
        assert {p for p, sh in shapes[name][1].items() if sh.optional and sh.dtype == "u8" and p.endswith("_inf")} == set(row.flags), name
        assert name in T.CASES


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_kzg_reduces_representatives(engine, name):
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"
    if "verify_batch" in name or "line_table" in name:
        ok = np.asarray(base[0]).astype(bool)
        assert not ok[[5, 20, 21, 33]].any() and ok.sum() > N // 2     # planted rows fail, most others pass (flagged rows aside)
