"""GPU: batched KZG opening verification under one SRS -- sylow_hip_kzg_fold_batch, sylow_hip_kzg_verify_batch,
sylow_hip_kzg_verify_line_table_batch and sylow_hip_kzg_batch_verify_weighted (kzg.hip, plk_verify.hip) against the CPU model of
tests/kzg_model.py: the fold bit for bit against oracle scalar multiplications and additions and against the library's own four-call
composition, the per-opening flags row by row against model_verify on a pool of 32 openings with every defect class planted (tiled to the
batch sizes, on every route the call has), and the weighted test's Gt words against the oracle's glued_pairing over the two literal pairs.
The CPU-side instances are built once per module."""
import ctypes
import types

import numpy as np
import pytest

import kzg_model as M

pytestmark = pytest.mark.gpu
POOL = 32
DEFECT_ROWS = {2: "y_plus_one", 5: "z_plus_one", 8: "pi_swapped", 12: "c_negated", 15: "c_identity_valid", 19: "pi_identity_valid",
               23: "pi_identity_invalid", 27: "f_identity"}
E_ARG = -2
TOP = (1 << 256) - 1


@pytest.fixture(scope="module")
def pools():
    valid = M.make_instance(POOL, seed=0x4B5A)
    planted = M.plant(valid, DEFECT_ROWS)
    want = M.model_verify(planted)
    assert np.array_equal(want, planted.expected()) and M.model_verify(valid).all()
    return types.SimpleNamespace(valid=valid, planted=planted, want=want)


def tile(inst, n):
    return inst.take(np.arange(n) % inst.n)


def args(inst):
    return inst.c, inst.z_words(), inst.y_words(), inst.pi, inst.c_inf, inst.pi_inf


def verify(engine, inst):
    return engine.kzg_verify(inst.tau_g2, *args(inst)).astype(bool)


def weighted(engine, inst, w):
    c, z, y, pi, ci, pii = args(inst)
    return engine.kzg_batch_verify_weighted(inst.tau_g2, c, z, y, pi, M.limbs(w), ci, pii)


def composed_fold(engine, inst):
    """the four-call composition the fold replaces: y G1gen, z pi, C + z pi, - y G1gen"""
    yg, yg_inf = engine.g1_generator_mul(M.limbs([v % M.R for v in inst.y]))
    zp, zp_inf = engine.g1_scalar_mul(inst.pi, M.limbs([v % M.R for v in inst.z]), inst.pi_inf)
    s, s_inf = engine.g1_add(inst.c, zp, inst.c_inf, zp_inf)
    return engine.g1_sub(s, yg, s_inf, yg_inf)


# ---- the fold ---------------------------------------------------------------------------------------------------------------------
_FOLD = []


def fold_case():
    """257 openings whose first rows are the special ones (so that n = 1, 64, 65 see them too), and the oracle's F, once"""
    if _FOLD:
        return _FOLD[0]
    n = 257
    rng = np.random.default_rng(0xF01D)
    fr = lambda: int(rng.integers(1, 1 << 62)) * 0x9E3779B97F4A7C15 * int(rng.integers(1, 1 << 62)) % M.R
    c, z, y, pi = ([fr() for _ in range(n)] for _ in range(4))
    words = [0, M.R, M.R + 1, TOP]
    zz, yy = [int(v) for v in z], [int(v) for v in y]
    c[0] = z[0] * pi[0] % M.R                                   # C = z pi: the last additions double / cancel
    c[1] = -z[1] * pi[1] % M.R                                  # C = -z pi
    c[2] = y[2]                                                 # C = y G1gen
    pi[3], pi[4] = 1, M.R - 1                                   # pi = +-G1gen
    c[5], pi[5] = (y[5] - z[5]) % M.R, 1                        # F = 0 with pi = G1gen
    for k, v in enumerate(words):                               # z and y in {0, r, r + 1, 2^256 - 1}, one at a time and together
        zz[6 + k] = v
        yy[10 + k] = v
        zz[14 + k], yy[14 + k] = v, words[(k + 1) % 4]
    inst = M.Instance(fr(), c, zz, yy, pi)
    inst.c_inf[18], inst.c[18] = 1, M.GARBAGE                   # flagged inputs over garbage words
    inst.pi_inf[19], inst.pi[19] = 1, M.GARBAGE
    inst.c_inf[20], inst.c[20], inst.pi_inf[20], inst.pi[20] = 1, M.GARBAGE, 1, M.GARBAGE
    inst.c_inf[100], inst.pi_inf[200] = 1, 1
    _FOLD.append((inst, M.C.g1_to_affine(M.model_fold(inst))))
    return _FOLD[0]


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_fold_matches_the_oracle_and_the_four_call_composition(engine, n):
    full, (want_xy, want_inf) = fold_case()
    inst = full.take(np.arange(n))
    xy, inf = engine.kzg_fold(*args(inst))
    assert np.array_equal(inf, want_inf[:n]), np.flatnonzero(inf != want_inf[:n])
    assert np.array_equal(xy, want_xy[:n]), np.flatnonzero((xy != want_xy[:n]).any(1))
    cxy, cinf = composed_fold(engine, inst)
    assert np.array_equal(xy, cxy) and np.array_equal(inf, cinf)
    if n >= 6:
        assert inf[5] == 1 and M.ints(xy[5].reshape(2, 4)) == [0, 1] and not inf[:5].any()      # the canonical identity


# ---- per-opening flags ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 64, 67, 1025])
def test_verify_flags_match_the_model_row_by_row(engine, pools, n):
    inst = tile(pools.planted, n)
    want = pools.want[np.arange(n) % POOL]
    got = verify(engine, inst)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    table = engine.g2_line_table(inst.tau_g2)
    got_t = engine.kzg_verify_line_table(table, *args(inst)).astype(bool)
    assert np.array_equal(got_t, want), np.flatnonzero(got_t != want)
    assert verify(engine, tile(pools.valid, n)).all()


def test_verify_flags_are_the_same_on_every_route(engine, pools):
    """n = 67: the default is one wavefront per Miller loop (67 <= WIDE_VERIFY_MAX); WIDE_TAIL = 0 switches the one-wavefront routes off and
    the batch runs on lane quads (67 <= QUAD_MAX); with QUAD_MAX = 0 as well it is k_bls_verify_fused<true> on lane pairs"""
    inst, want = tile(pools.planted, 67), pools.want[np.arange(67) % POOL]
    table = engine.g2_line_table(inst.tau_g2)
    both = lambda: (verify(engine, inst), engine.kzg_verify_line_table(table, *args(inst)).astype(bool))
    try:
        for got in both():
            assert np.array_equal(got, want)
        engine.set_option("WIDE_TAIL", 0)
        for got in both():
            assert np.array_equal(got, want)
        engine.set_option("QUAD_MAX", 0)
        for got in both():
            assert np.array_equal(got, want)
    finally:
        for o in ("WIDE_TAIL", "QUAD_MAX"):
            engine.set_option(o, -1)


def test_verify_equals_fold_then_the_hashed_bls_check_with_tau_replicated(engine, pools):
    inst = tile(pools.planted, 67)
    f, f_inf = engine.kzg_fold(*args(inst))
    ok = engine.bls_verify_hashed(np.repeat(inst.tau_g2, inst.n, 0), inst.pi, f, h_inf=inst.pi_inf, sig_inf=f_inf).astype(bool)
    assert np.array_equal(ok, verify(engine, inst)) and np.array_equal(ok, pools.want[np.arange(67) % POOL])


# ---- scalars are words ------------------------------------------------------------------------------------------------------------
def weights64(n, seed):
    rng = np.random.default_rng(seed)
    return [int(v) | 1 for v in rng.integers(1, 1 << 63, size=n, dtype=np.uint64)]


def test_scalars_and_weights_are_any_256_bit_words(engine, pools):
    inst = tile(pools.planted, POOL)
    w = weights64(POOL, 3)
    ok, (gt, one) = verify(engine, inst), weighted(engine, inst, w)
    assert np.array_equal(ok, pools.want) and not one
    shifted = inst.take(np.arange(POOL))
    shifted.z = [v + M.R if v + M.R <= TOP else v for v in inst.z]
    shifted.y = [v + 2 * M.R if v + 2 * M.R <= TOP else v for v in inst.y]
    assert all(a != b for a, b in zip(shifted.z, inst.z))
    assert np.array_equal(verify(engine, shifted), ok)
    gt_s, one_s = weighted(engine, shifted, [v + M.R for v in w])
    assert np.array_equal(gt_s, gt) and one_s == one
    top = inst.take(np.arange(4))                                   # 2^256 - 1 is accepted, as z, as y and as a weight
    top.z[0], top.y[1] = TOP, TOP
    want = M.model_verify(top)
    assert np.array_equal(verify(engine, top), want) and not want[0] and not want[1]
    wt = [TOP, 3, TOP, 5]
    gt_t, _ = weighted(engine, top, wt)
    assert np.array_equal(gt_t[0], M.weighted_product(top, wt))


# ---- weighted ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 300])
def test_weighted_gt_is_the_oracle_product_over_the_literal_pairs(engine, pools, n):
    w = weights64(n, 40 + n)
    good = tile(pools.valid, n)
    one_bad = M.plant(pools.valid, {0: "c_negated"}).take([0] + [1 + k % (POOL - 1) for k in range(n - 1)])      # exactly one invalid row
    for inst, want_one in ((good, True), (one_bad, False)):
        want_gt = M.weighted_product(inst, w)
        gt, is_one = weighted(engine, inst, w)
        assert np.array_equal(gt[0], want_gt) and is_one == want_one and np.array_equal(want_gt, M.ONE48) == want_one
    w0 = [0] + w[1:]
    assert weighted(engine, one_bad, w0)[1]                                               # weight 0 removes the only invalid opening
    gt0, one0 = weighted(engine, one_bad, [0] * n)
    assert one0 and np.array_equal(gt0[0], M.ONE48)                                       # all-zero weights: the identity


def test_weighted_with_identity_rows_and_the_empty_batch(engine, pools):
    w = weights64(POOL, 77)
    gt, one = weighted(engine, pools.planted, w)
    assert np.array_equal(gt[0], M.weighted_product(pools.planted, w)) and not one
    ok_rows = np.flatnonzero(pools.want)                                                  # the valid rows, flagged C and flagged pi among them
    inst = pools.planted.take(ok_rows)
    gt, one = weighted(engine, inst, w[:inst.n])
    assert one and np.array_equal(gt[0], M.ONE48)
    empty = pools.valid.take(np.zeros(0, dtype=np.int64))
    gt_e, one_e = weighted(engine, empty, [])
    assert one_e and np.array_equal(gt_e[0], M.ONE48)
    assert verify(engine, empty).shape == (0,) and engine.kzg_fold(*args(empty))[0].shape == (0, 8)


# ---- whole-call errors ------------------------------------------------------------------------------------------------------------
def test_null_pointers_are_refused_and_nothing_is_written(engine, pools):
    inst = tile(pools.valid, 4)
    n = inst.n
    p = lambda x: ctypes.c_void_p(x.ptr) if x is not None else None
    d = dict(tau=engine.to_device_soa(inst.tau_g2, 16), c=engine.to_device_soa(inst.c, 8), z=engine.to_device_soa(inst.z_words(), 4),
             y=engine.to_device_soa(inst.y_words(), 4), pi=engine.to_device_soa(inst.pi, 8), w=engine.to_device_soa(M.limbs(weights64(n, 1)), 4))
    table = engine.g2_line_table(inst.tau_g2)
    fill = lambda k, dt: engine.to_device(np.full(k, 7, dtype=dt))
    out, oi, ok, gt, one = fill(8 * n, np.uint64), fill(n, np.uint8), fill(n, np.uint8), fill(48, np.uint64), fill(1, np.uint8)
    untouched = lambda *arrs: all((a.download() == 7).all() for a in arrs)
    lib = engine.lib

    def opening(drop):
        return [None if k == drop else p(d[k]) for k in ("c",)] + [None] + [None if k == drop else p(d[k]) for k in ("z", "y", "pi")] + [None]

    for drop in ("c", "z", "y", "pi"):
        c, ci, z, y, pi, pii = opening(drop)
        assert lib.sylow_hip_kzg_fold_batch(c, ci, z, y, pi, pii, p(out), p(oi), n, None) == E_ARG and untouched(out, oi), drop
        assert lib.sylow_hip_kzg_verify_batch(p(d["tau"]), c, ci, z, y, pi, pii, p(ok), n, None) == E_ARG and untouched(ok), drop
        assert lib.sylow_hip_kzg_verify_line_table_batch(p(table), c, ci, z, y, pi, pii, p(ok), n, None) == E_ARG and untouched(ok), drop
        assert lib.sylow_hip_kzg_batch_verify_weighted(p(d["tau"]), c, ci, z, y, pi, pii, p(d["w"]), n, p(gt), p(one), None) == E_ARG and untouched(gt, one), drop
    c, ci, z, y, pi, pii = opening(None)
    assert lib.sylow_hip_kzg_fold_batch(c, ci, z, y, pi, pii, None, p(oi), n, None) == E_ARG and untouched(oi)
    assert lib.sylow_hip_kzg_fold_batch(c, ci, z, y, pi, pii, p(out), None, n, None) == E_ARG and untouched(out)
    assert lib.sylow_hip_kzg_verify_batch(None, c, ci, z, y, pi, pii, p(ok), n, None) == E_ARG and untouched(ok)
    assert lib.sylow_hip_kzg_verify_batch(p(d["tau"]), c, ci, z, y, pi, pii, None, n, None) == E_ARG
    assert lib.sylow_hip_kzg_verify_line_table_batch(None, c, ci, z, y, pi, pii, p(ok), n, None) == E_ARG and untouched(ok)
    assert lib.sylow_hip_kzg_verify_line_table_batch(p(table), c, ci, z, y, pi, pii, None, n, None) == E_ARG
    assert lib.sylow_hip_kzg_batch_verify_weighted(None, c, ci, z, y, pi, pii, p(d["w"]), n, p(gt), p(one), None) == E_ARG and untouched(gt, one)
    assert lib.sylow_hip_kzg_batch_verify_weighted(p(d["tau"]), c, ci, z, y, pi, pii, None, n, p(gt), p(one), None) == E_ARG and untouched(gt, one)
    assert lib.sylow_hip_kzg_batch_verify_weighted(p(d["tau"]), c, ci, z, y, pi, pii, p(d["w"]), n, None, None, None) == E_ARG
    # the same arguments, complete: the calls run, and either output of the weighted call may be left out
    assert lib.sylow_hip_kzg_verify_batch(p(d["tau"]), c, ci, z, y, pi, pii, p(ok), n, None) == 0 and (ok.download() == 1).all()
    assert lib.sylow_hip_kzg_batch_verify_weighted(p(d["tau"]), c, ci, z, y, pi, pii, p(d["w"]), n, None, p(one), None) == 0 and one.download()[0] == 1
    assert lib.sylow_hip_kzg_batch_verify_weighted(p(d["tau"]), c, ci, z, y, pi, pii, p(d["w"]), n, p(gt), None, None) == 0
    assert np.array_equal(gt.download(), M.ONE48)


def test_api_holder(engine, pools):
    from sylow_amd import api
    inst = pools.planted
    kzg = api.KzgVerifier(api.G2Affine(inst.tau_g2))
    openings = (api.G1Affine(inst.c, inst.c_inf), inst.z, inst.y_words(), api.G1Affine(inst.pi, inst.pi_inf))
    ok = kzg.verify(openings)
    assert ok.dtype == bool and np.array_equal(ok, pools.want)
    assert np.array_equal(kzg.verify(openings), pools.want)                                # the cached table serves the second call
    w = weights64(POOL, 9)
    assert kzg.verify_weighted(openings, w) is False
    good = pools.valid
    assert kzg.verify_weighted((api.G1Affine(good.c), good.z, good.y, api.G1Affine(good.pi)), M.limbs(w)) is True
    with pytest.raises(ValueError):
        api.KzgVerifier(api.G2Affine(np.repeat(inst.tau_g2, 2, 0)))
