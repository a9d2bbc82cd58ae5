"""GPU: the paths of kzg.hip that the batches of tests/test_gpu_kzg.py are too small or too random to reach.
  * the two digit walks of k_kzg_fold on scalars crafted for them (kzg_model.crafted_fold_scalars: window 32 of the GLV walk, digits -8 and 7
    in window 31, a zero half, a negative half; byte digits -128 / +127 / carry chains of the comb walk), bit for bit against the oracle
    and the four-call composition, with and without the optional flag pointers, and through the verifier row by row;
  * the grid stride of k_kzg_fold: n = 2 * CUs * 256 + 257, so that 257 lanes fold a second opening in their rebuilt window table, through
    the fold and through both verifiers (the second-trip -pi / flags);
  * the weighted test at n = 65 537: 257 partials (k_kzg_fr_join strides) and 131 074 terms on the bucket route of g1_msm, fed from device
    arrays; the expected Gt words come from the 32-row pool under collapsed weights (kzg_model.collapse_weights).
The host side is numpy throughout: the large batches are tiled as limb arrays, never as Python lists."""
import numpy as np
import pytest

import kzg_model as M
from test_gpu_kzg import POOL, TOP, composed_fold, fold_case, pools  # noqa: F401  (pools: the module fixture of the planted pool)

pytestmark = pytest.mark.gpu
BLOCK = 256
_CRAFTED = []


def crafted():
    """the crafted instance, the oracle's fold of it and the model's booleans, once"""
    if not _CRAFTED:
        inst, valid = M.crafted_instance()
        ok = M.model_verify(inst)
        assert np.array_equal(ok, valid)
        _CRAFTED.append((inst, M.C.g1_to_affine(M.model_fold(inst)), ok))
    return _CRAFTED[0]


def first_diff(got, want):
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(1))
    return None if len(bad) == 0 else int(bad[0])


def tags(inst):
    cs = M.crafted_fold_scalars()
    zt, yt = {v: t for t, v in cs.z}, {v: t for t, v in cs.y}
    return [zt.get(z) or yt.get(y) for z, y in zip(inst.z, inst.y)]


# ---- crafted digits ---------------------------------------------------------------------------------------------------------------
def test_fold_of_the_crafted_scalars_matches_the_oracle_and_the_composition(engine):
    inst, (want_xy, want_inf), _ = crafted()
    assert inst.n < 257 and not inst.c_inf.any() and not inst.pi_inf.any()
    c, z, y, pi = inst.c, inst.z_words(), inst.y_words(), inst.pi
    for flags in ((inst.c_inf, inst.pi_inf), (None, None)):                       # all-zero flags, then the pointers left out
        xy, inf = engine.kzg_fold(c, z, y, pi, *flags)
        row = first_diff(np.column_stack([xy, inf]), np.column_stack([want_xy, want_inf]))
        assert row is None, (row, tags(inst)[row], hex(inst.z[row]), hex(inst.y[row]))
    cxy, cinf = composed_fold(engine, inst)
    assert np.array_equal(xy, cxy) and np.array_equal(inf, cinf)
    assert not inf.any()                                                          # no row folds to the identity: every row was compared on its words


def test_verify_of_the_crafted_scalars_matches_the_model_row_by_row(engine):
    inst, _, want = crafted()
    assert 0.4 < want.mean() < 0.6
    c, z, y, pi = inst.c, inst.z_words(), inst.y_words(), inst.pi
    table = engine.g2_line_table(inst.tau_g2)
    for flags in ((inst.c_inf, inst.pi_inf), (None, None)):
        got = engine.kzg_verify(inst.tau_g2, c, z, y, pi, *flags).astype(bool)
        row = first_diff(got, want)
        assert row is None, (row, tags(inst)[row], hex(inst.z[row]), hex(inst.y[row]))
        got = engine.kzg_verify_line_table(table, c, z, y, pi, *flags).astype(bool)
        assert first_diff(got, want) is None, first_diff(got, want)


# ---- the grid stride --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes():
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * BLOCK


def test_fold_past_the_grid_cap_matches_the_oracle_on_every_row(engine, lanes):
    full, (want_xy, want_inf) = fold_case()
    pool = 257
    assert full.n == pool and lanes % pool != 0                                   # a lane's second opening is another pool row than its first
    n = lanes + pool
    idx = np.arange(n) % pool
    xy, inf = engine.kzg_fold(full.c[idx], full.z_words()[idx], full.y_words()[idx], full.pi[idx], full.c_inf[idx], full.pi_inf[idx])
    row = first_diff(np.column_stack([xy, inf]), np.column_stack([want_xy, want_inf])[idx])
    assert row is None, f"first differing row {row} (pool row {row % pool}), {'at or past' if row >= lanes else 'before'} the second trip at {lanes}"


def test_verify_past_the_grid_cap_matches_the_model_on_every_row(engine, pools, lanes):
    inst = pools.planted
    n = lanes + 257
    idx = np.arange(n) % POOL
    assert 257 % POOL != 0 and (~pools.want[idx[lanes:]]).any() and inst.pi_inf[idx[lanes:]].any()
    want = pools.want[idx]
    a = (inst.c[idx], inst.z_words()[idx], inst.y_words()[idx], inst.pi[idx], inst.c_inf[idx], inst.pi_inf[idx])
    got = engine.kzg_verify(inst.tau_g2, *a).astype(bool)
    row = first_diff(got, want)
    assert row is None, f"first differing row {row}, {'at or past' if row >= lanes else 'before'} the second trip at {lanes}"
    got = engine.kzg_verify_line_table(engine.g2_line_table(inst.tau_g2), *a).astype(bool)
    row = first_diff(got, want)
    assert row is None, f"line table: first differing row {row}, {'at or past' if row >= lanes else 'before'} the second trip at {lanes}"


# ---- the weighted test where the join strides and the multi-scalar multiplication takes buckets -------------------------------------
def test_weighted_at_65537_openings_matches_the_collapsed_pool(engine, pools):
    n = 65537
    assert (n + BLOCK - 1) // BLOCK == 257 > BLOCK and 2 * n > 1 << 16
    idx = np.arange(n) % POOL
    w64 = (2 * np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)        # odd times odd mod 2^64: distinct, odd
    assert len(np.unique(w64)) == n and (w64 & np.uint64(1)).all()
    w = w64.tolist()
    for k, v in ((0, TOP), (65536, TOP), (12, M.R + 1), (257, M.R + 3), (40000, M.R + 0xFFFF), (65535, M.R - 1)):
        w[k] = v
    wl = np.zeros((n, 4), dtype=np.uint64)
    wl[:, 0] = w64
    big = [k for k, v in enumerate(w) if v >> 64]
    wl[big] = M.limbs([w[k] for k in big])
    run = lambda inst, words: engine.kzg_batch_verify_weighted(inst.tau_g2, inst.c[idx], inst.z_words()[idx], inst.y_words()[idx], inst.pi[idx], words,
                                                               inst.c_inf[idx], inst.pi_inf[idx])
    collapsed = M.collapse_weights(idx, w, POOL)
    gt, one = run(pools.valid, wl)
    assert np.array_equal(gt[0], M.weighted_product(pools.valid, collapsed)) and np.array_equal(gt[0], M.ONE48) and one
    want = M.weighted_product(pools.planted, collapsed)
    gt, one = run(pools.planted, wl)
    assert not np.array_equal(want, M.ONE48)
    assert np.array_equal(gt[0], want) and not one
    bad = ~pools.want[idx]                                                        # every tiled copy of an invalid row leaves the batch
    w0 = wl.copy()
    w0[bad] = 0
    gt, one = run(pools.planted, w0)
    assert np.array_equal(gt[0], M.ONE48) and one
    assert np.array_equal(M.weighted_product(pools.planted, M.collapse_weights(idx, [0 if b else v for b, v in zip(bad, w)], POOL)), M.ONE48)
