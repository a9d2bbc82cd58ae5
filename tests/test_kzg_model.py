"""CPU: the KZG model of tests/kzg_model.py stands on its own -- on a pool of 32 openings carrying every defect class the oracle's pairing
product gives exactly the booleans the classes dictate, so the expected flags of tests/test_gpu_kzg.py never rest on the engine; the weighted
product is the identity on valid openings and is not with one defect under a nonzero weight, and a tiled batch collapses onto its pool; the
crafted scalars of the fold tests (kzg_model.crafted_fold_scalars) carry the window digits their tags claim under the model of the device's
decomposition (tools/glv_model.py) and the two digit rules, and the digits recompose to what they were cut from -- and the four entry points are exported by the
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


def test_a_tiled_batch_collapses_onto_its_pool(valid):
    """n = 100 over the planted pool (flagged C, flagged pi, invalid rows): the weighted product of the tiled batch is the product of the 32
    pool rows under the per-row sums of the weights"""
    planted = M.plant(valid, DEFECT_ROWS)
    rng = np.random.default_rng(0xC011)
    idx = np.arange(100) % POOL
    w = [int(v) | 1 for v in rng.integers(1, 1 << 63, size=100, dtype=np.uint64)]
    w[3], w[40], w[41] = (1 << 256) - 1, M.R + 5, 0
    for pool in (planted, valid):
        got = M.weighted_product(pool, M.collapse_weights(idx, w, POOL))
        assert np.array_equal(got, M.weighted_product(pool.take(idx), w))
        assert np.array_equal(got, M.ONE48) == (pool is valid)
    bad = ~M.model_verify(planted)
    w0 = [0 if bad[i] else v for i, v in zip(idx, w)]                                    # every copy of an invalid row removed
    assert np.array_equal(M.weighted_product(planted, M.collapse_weights(idx, w0, POOL)), M.ONE48)


# ---- the crafted scalars of the fold ----------------------------------------------------------------------------------------------
def halves(tag):
    return [M.glv_halves(v) for t, v in M.crafted_fold_scalars().z if t == tag]


def test_crafted_z_carry_the_window_digits_their_tags_claim():
    import evm_model
    cs = M.crafted_fold_scalars()
    assert cs is M.crafted_fold_scalars() and len(cs.z) + len(cs.y) < 120 and all(0 <= v < M.R for _, v in cs.z)
    dig = M.glv_window_digits
    top = halves("k2_top")                                                               # window 32 of the k2 half, digit 31 = -8 with it
    assert len(top) >= 4 and all(dig(m2)[32] == 1 and dig(m2)[31] == -8 and dig(m1)[32] == 0 and n1 == n2 for (m1, n1), (m2, n2) in top)
    assert all(dig(m1)[31] == 7 for (m1, _), _ in halves("k1_digit31_7")) and len(halves("k1_digit31_7")) == 2
    assert all(dig(m2)[31] == 7 and dig(m2)[32] == 0 for _, (m2, _) in halves("k2_digit31_7")) and len(halves("k2_digit31_7")) == 2
    (_, (m2, n2)), = halves("k2_near_all_minus_8")
    assert dig(m2)[32] == 1 and sum(d == -8 for d in dig(m2)[:32]) == 31 and not n2
    (_, (m2, n2)), = halves("k2_near_all_7")
    assert dig(m2)[32] == 0 and sum(d == 7 for d in dig(m2)[:32]) == 31 and not n2
    assert dig(M.GLV_TOP) == [-8] * 32 + [1] and dig(M.GLV_SEVENS) == [7] * 32 + [0] and dig(M.GLV_TOP - 1) == [7] * 32 + [0]
    assert len(halves("k2_zero")) == 3 and all(m1 != 0 and m2 == 0 for (m1, _), (m2, _) in halves("k2_zero"))
    neg = halves("k2_negative")                                                          # flip2: n1 != n2
    assert len(neg) >= 2 and all(n2 and not n1 and 0 < m2 < 1 << 64 for (m1, n1), (m2, n2) in neg)
    assert [v for t, v in cs.z if t == "edge"] == [v % M.R for v in evm_model.glv_edge_scalars()]
    # what the docstring of crafted_fold_scalars says the model cannot reach: not in the list, and not in a seeded sample twenty times the
    # size of the searches that made the list, drawn where the halves are largest (the top sixteenth of [0, r)) and over all of [0, r)
    import random
    rng = random.Random(0x5EA)
    sample = [M.R - 1 - rng.randrange(M.R >> 4) for _ in range(20000)] + [rng.randrange(M.R) for _ in range(20000)] + [v for _, v in cs.z]
    hv = [M.glv_halves(v) for v in sample]
    assert max(m1 for (m1, _), _ in hv) < M.GLV_TOP                                      # window 32 of the k1 half
    assert not any(n1 for (_, n1), _ in hv)                                              # a negative k1
    assert all(m2 < 1 << 64 for _, (m2, n2) in hv if n2)                                 # a negative k2 of any size
    assert all(v == 0 for v, ((m1, _), _) in zip(sample, hv) if m1 == 0)                 # k1 = 0 beside k2 != 0
    assert sum(m2 >= M.GLV_TOP for _, (m2, _) in hv[:20000]) > 100                       # while the k2 window is there to be found


def test_crafted_y_carry_the_byte_digits_their_tags_claim():
    cs = M.crafted_fold_scalars()
    d = {t: M.comb_digits(v) for t, v in cs.y}
    below = lambda t, byte: all((v >> (8 * w)) & 255 == byte for tt, v in cs.y if tt == t for w in range(31))
    assert below("all_80", 0x80) and below("all_7f", 0x7F) and below("all_ff", 0xFF) and below("all_80_top_0", 0x80)
    assert d["all_80"][:31] == [-128] + [-127] * 30 and d["all_80_top_0"] == [-128] + [-127] * 30 + [1]
    assert d["all_7f"][:31] == [127] * 31                                                # entry 126 in every window, no carry
    assert d["all_ff"] == [-1] + [0] * 30 + [0x30]                                       # a carry chain through 30 zero digits
    assert d["alternating"].count(-128) == 2 and d["alternating"].count(127) == 1 and dict(cs.y)["alternating"] >= M.R
    assert d["alternating_807f"][:31] == [-128, -128] + [-127, -128] * 14 + [-127]       # entry 127 (the last) in 16 windows
    assert d["alternating_7f80"][:31] == [-128] + [-127, -128] * 15                      # and in the other 15, window 30 among them
    assert dict(cs.y)["r_minus_1"] == M.R - 1 and d["r_minus_1"][:3] == [0, 0, 0]
    # window 31: y mod r < r < 0x31 2^248, and a carry into it needs byte 30 >= 0x7f, which a top byte of 0x30 rules out (byte 30 of r is
    # 0x64): 0x30 is the largest digit, reached without and with a carry
    assert M.R >> 248 == 0x30 and (M.R >> 240) & 255 == 0x64
    assert d["top_digit_max"][31] == 0x30 and d["top_digit_max_by_carry"] == [-128] + [0] * 30 + [0x30]
    assert max(max(v) for v in d.values()) == 127 and min(min(v) for v in d.values()) == -128


def test_crafted_digits_recompose():
    cs = M.crafted_fold_scalars()
    lam = M.glv_model.lam
    for _, v in cs.z:
        (m1, n1), (m2, n2) = M.glv_halves(v)
        for m in (m1, m2):
            dg = M.glv_window_digits(m)
            assert len(dg) == 33 and all(-8 <= x <= 7 for x in dg[:32]) and dg[32] in (0, 1) and sum(x * 16 ** i for i, x in enumerate(dg)) == m
        assert ((-m1 if n1 else m1) + (-m2 if n2 else m2) * lam - v) % M.R == 0
    for _, v in cs.y:
        dg = M.comb_digits(v)
        assert len(dg) == 32 and all(-128 <= x <= 127 for x in dg) and 0 <= dg[31] <= 0x30 and sum(x * 256 ** i for i, x in enumerate(dg)) == v % M.R


def test_the_crafted_instance_is_what_its_maker_says():
    inst, valid = M.crafted_instance()
    cs = M.crafted_fold_scalars()
    assert inst.n < 257 and not inst.c_inf.any() and not inst.pi_inf.any() and 0.4 < valid.mean() < 0.6
    assert set(inst.z) >= {v for _, v in cs.z} and set(inst.y) >= {v for _, v in cs.y}
    gen = M.limbs(M.G.G1_GEN).reshape(8)
    plus = [i for i in range(inst.n) if np.array_equal(inst.pi[i], gen)]
    minus = [i for i in range(inst.n) if inst.dlog["pi"][i] == M.R - 1]
    assert len(plus) == len(minus) == inst.n // 4 and valid[plus].any() and not valid[plus].all() and valid[minus].any()
    assert np.array_equal(M.model_verify(inst), valid)


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
