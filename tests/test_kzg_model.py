"""CPU: the KZG model of tests/kzg_model.py stands on its own -- on a pool of 32 openings carrying every defect class the oracle's pairing
product gives exactly the booleans the classes dictate, so the expected flags of tests/test_gpu_kzg.py never rest on the engine; the weighted
product is the identity on valid openings and is not with one defect under a nonzero weight -- and the four entry points are exported by the
built library and carry a shape annotation in the header."""
import ctypes
import os

import numpy as np
import pytest

import kzg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL = 32
DEFECT_ROWS = {2: "y_plus_one", 5: "z_plus_one", 8: "pi_swapped", 12: "c_negated", 15: "c_identity_valid", 19: "pi_identity_valid",
               23: "pi_identity_invalid", 27: "f_identity"}
SYMBOLS = ["sylow_hip_kzg_fold_batch", "sylow_hip_kzg_verify_batch", "sylow_hip_kzg_verify_line_table_batch", "sylow_hip_kzg_batch_verify_weighted"]


@pytest.fixture(scope="module")
def valid():
    return M.make_instance(POOL, seed=0x4B5A)


def test_the_model_gives_the_booleans_the_defect_classes_dictate(valid):
    assert set(DEFECT_ROWS.values()) == set(M.DEFECTS)
    assert M.model_verify(valid).all()
    planted = M.plant(valid, DEFECT_ROWS)
    want = planted.expected()
    assert not want[[2, 5, 8, 9, 12, 23, 27]].any() and want[[15, 19]].all() and want.sum() == POOL - 7
    assert np.array_equal(M.model_verify(planted), want)
    # the identity rows are what they claim: F = 0 on rows 19 and 27, a flagged C on 15, flagged proofs on 19 and 23
    f_inf = M.G.is_identity(M.model_fold(planted))
    assert f_inf[19] and f_inf[27] and f_inf.sum() == 2
    assert planted.c_inf[15] and planted.pi_inf[19] and planted.pi_inf[23] and not planted.pi_inf[27]
    tiled = planted.take(np.arange(40) % POOL)
    assert np.array_equal(tiled.expected(), want[np.arange(40) % POOL])


def test_scalars_act_mod_r(valid):
    inst = valid.take(np.arange(4))
    inst.z = [inst.z[0] + M.R, inst.z[1], (1 << 256) - 1, inst.z[3]]
    inst.y = [inst.y[0], inst.y[1] + M.R, inst.y[2], 0]
    assert np.array_equal(M.model_verify(inst), [True, True, False, False])


def test_weighted_product_is_the_identity_iff_every_weighted_opening_is_valid(valid):
    w = [(0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1) | 1 for i in range(POOL)]
    assert np.array_equal(M.weighted_product(valid, w), M.ONE48)
    bad = M.plant(valid, {6: "c_negated"})
    assert not np.array_equal(M.weighted_product(bad, w), M.ONE48)
    w[6] = 0
    assert np.array_equal(M.weighted_product(bad, w), M.ONE48)
    assert np.array_equal(M.weighted_product(valid.take(np.zeros(0)), []), M.ONE48)


def test_the_built_library_exports_the_four_symbols():
    lib = ctypes.CDLL(os.path.join(ROOT, "sylow_amd", "libsylow_hip.so"))
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_header_carries_a_shape_line_for_each_symbol():
    from sylow_amd import _shapes
    shapes = _shapes.parse()
    for s in SYMBOLS:
        names, sh = shapes[s]
        assert {"c_xy", "z", "y", "pi_xy"} <= set(sh) and sh["c_inf"].optional and sh["pi_inf"].optional, s
