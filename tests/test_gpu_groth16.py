"""GPU: batched Groth16 verification under one verifying key -- sylow_hip_groth16_vk_x_batch, sylow_hip_groth16_verify_batch and
sylow_hip_groth16_batch_verify_weighted (groth16.hip, groth16_pair.hpp) against the CPU model of tests/groth16_model.py: vk_x bit for bit
against oracle scalar multiplications and additions, the per-proof flags row by row against model_verify on a pool of 64 instances with
every defect class planted (tiled to the batch sizes, on every route the call has and under a scratch limit that slices the tables), the
same booleans from the three EVM precompile batches, and the weighted test's Gt words against the oracle's glued_pairing over the literal
pairs.  The CPU-side instances are built once per module."""
import ctypes
import types

import numpy as np
import pytest

import groth16_model as M

pytestmark = pytest.mark.gpu
POOL = 64
L = 3
DEFECT_ROWS = {3: "c_swapped", 9: "input_plus_one", 17: "a_negated", 21: "b_swapped", 30: "a_identity", 41: "a_c_identity_valid", 55: "vk_x_identity"}
E_ARG = -2
TABLE_BYTES_PER_PROOF = 87 * 7 * 2 * 16                      # one slot of k_pair_lines' layout


@pytest.fixture(scope="module")
def pools():
    valid = M.make_instance(POOL, L, seed=0x67E6)
    planted = M.plant(valid, DEFECT_ROWS)
    want = M.model_verify(planted)
    assert np.array_equal(want, planted.expected()) and M.model_verify(valid).all()
    return types.SimpleNamespace(valid=valid, planted=planted, want=want)


def tile(inst, n):
    return inst.take(np.arange(n) % inst.n)


def verify(engine, inst):
    return engine.groth16_verify(inst.vk(), inst.a, inst.b, inst.c, inst.input_words(), inst.a_inf, inst.b_inf, inst.c_inf).astype(bool)


def weighted(engine, inst, w):
    return engine.groth16_batch_verify_weighted(inst.vk(), inst.a, inst.b, inst.c, inst.input_words(), M.limbs(w), inst.a_inf, inst.b_inf, inst.c_inf)


# ---- vk_x -------------------------------------------------------------------------------------------------------------------------
SPECIAL = [0, 1, M.R - 1, M.R, M.R + 1, M.P, (1 << 256) - 1]
_VKX = {}


def vkx_case(l):
    """257 rows of l inputs with the special words spread over rows and columns, and the oracle's vk_x, once per l"""
    if l not in _VKX:
        inst = M.make_instance(257, l, seed=0x1C00 + l)
        for k, v in enumerate(SPECIAL * 3):
            if l:
                inst.inputs[(11 * k + 1) % 257][k % l] = v
        if l:
            inst.inputs[0] = [SPECIAL[(j + 2) % 7] for j in range(l)]        # row 0 (the n = 1 case) is special words only
        _VKX[l] = (inst, M.C.g1_to_affine(M.model_vk_x(inst)))
    return _VKX[l]


@pytest.mark.parametrize("l", [0, 1, 3, 17])
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_vk_x_matches_the_oracle_and_lincomb(engine, n, l):
    inst, (want_xy, want_inf) = vkx_case(l)
    words = inst.input_words()[:n]
    xy, inf = engine.groth16_vk_x(inst.ic, words)
    assert np.array_equal(xy, want_xy[:n]) and np.array_equal(inf, want_inf[:n])
    # the composed route on replicated bases: term-major, scalar 1 for IC_0, inputs mod r
    bases = np.repeat(inst.ic, n, 0)
    k = M.limbs([1] * n + [inst.inputs[i][j] % M.R for j in range(l) for i in range(n)])
    cxy, cinf = engine.g1_lincomb(bases, k, n, l + 1)
    assert np.array_equal(xy, cxy) and np.array_equal(inf, cinf)


def test_vk_x_equal_bases_cancelling_bases_and_the_identity(engine):
    rng = np.random.default_rng(5)
    fr = lambda: int(rng.integers(1, 1 << 62)) * 0x9E3779B97F4A7C15 % M.R
    c0, c1, c3 = fr(), fr(), fr()
    inv = lambda v: pow(v % M.R, M.R - 2, M.R)
    x, y = fr(), fr()
    cases = [
        ([c0, c1, c1, c3], [[x, y, fr()], [x, x, 0], [0, 0, 0]]),                                   # IC_1 == IC_2
        ([c0, c1, M.R - c1, c3], [[x, x, y], [x, x, (-c0 * inv(c3)) % M.R], [M.R + x, x, 1]]),      # IC_2 == -IC_1, equal inputs; row 1 sums to 0
    ]
    for dl, rows in cases:
        inst = types.SimpleNamespace(ic=M.g1_gen_mul(dl)[0], n=len(rows), l=3, inputs=rows)
        want_xy, want_inf = M.C.g1_to_affine(M.model_vk_x(inst))
        xy, inf = engine.groth16_vk_x(inst.ic, M.limbs([v for r in rows for v in r]).reshape(len(rows), 3, 4))
        assert np.array_equal(xy, want_xy) and np.array_equal(inf, want_inf)
    assert inf[1] == 1 and M.ints(xy[1].reshape(2, 4)) == [0, 1] and not inf[0] and not inf[2]      # the canonical identity


# ---- verify_batch -----------------------------------------------------------------------------------------------------------------
# n <= 1024 (with 4 n <= WIDE_MAX = 6144) takes the composed route, 1025 the table route
@pytest.mark.parametrize("n", [1, 2, 64, 67, 1025])
def test_verify_flags_match_the_model_row_by_row(engine, pools, n):
    got = verify(engine, tile(pools.planted, n))
    want = pools.want[np.arange(n) % POOL]
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert verify(engine, tile(pools.valid, n)).all()


def test_verify_table_route_at_small_n_and_without_the_small_routes(engine, pools):
    inst, want = tile(pools.planted, 67), pools.want[np.arange(67) % POOL]
    try:
        engine.set_option("WIDE_MAX", 1)                      # no batch fits the one-wavefront route: 67 proofs go through the line tables
        assert np.array_equal(verify(engine, inst), want)
        engine.set_option("WIDE_MAX", -1)
        engine.set_option("WIDE_TAIL", 0)                     # every small-batch route off, the per-call Miller loop on a lane pair
        assert np.array_equal(verify(engine, inst), want)
        engine.set_option("WIDE_TAIL", -1)
        engine.set_option("MULTI_TABLES", 0)                  # no tables anywhere: the composed route on the in-register schedule
        assert np.array_equal(verify(engine, tile(pools.planted, 1025)), pools.want[np.arange(1025) % POOL])
    finally:
        for o in ("WIDE_MAX", "WIDE_TAIL", "MULTI_TABLES"):
            engine.set_option(o, -1)


def test_verify_flags_do_not_depend_on_the_scratch_limit(engine, pools):
    n = 1025
    inst, want = tile(pools.planted, n), pools.want[np.arange(n) % POOL]
    try:
        engine.set_scratch_limit(1024 * TABLE_BYTES_PER_PROOF)                # the smallest limit the table route honours: slices of 1024 + 1
        assert np.array_equal(verify(engine, inst), want)
        engine.set_scratch_limit(1024 * TABLE_BYTES_PER_PROOF - 1)            # below it: the composed route, no table at all
        assert np.array_equal(verify(engine, inst), want)
    finally:
        engine.set_scratch_limit(0)


def _w(v):
    return int(v).to_bytes(32, "big")


def _g1b(xy, inf=False):
    x, y = M.ints(np.asarray(xy).reshape(2, 4))
    return bytes(64) if inf else _w(x) + _w(y)


def _g2b(xy):
    x0, x1, y0, y1 = M.ints(np.asarray(xy).reshape(4, 4))
    return _w(x1) + _w(x0) + _w(y1) + _w(y0)


def test_the_evm_precompile_batches_give_the_same_booleans(engine, pools):
    from sylow_amd import evm
    inst = pools.planted
    n = inst.n
    vk_x = [_g1b(inst.ic[0])] * n
    for j in range(L):                                        # the Solidity verifier's loop, one batch per call site
        terms = evm.run_mul(engine, [_g1b(inst.ic[j + 1]) + _w(inst.inputs[i][j]) for i in range(n)])
        vk_x = evm.run_add(engine, [vk_x[i] + terms[i] for i in range(n)])
    na = inst.a.copy()
    na[:, 4:8] = M.limbs([(M.P - v) % M.P for v in M.ints(inst.a[:, 4:8])])
    jobs = [_g1b(na[i], inst.a_inf[i]) + _g2b(inst.b[i]) + _g1b(inst.alpha[0]) + _g2b(inst.beta[0]) + vk_x[i] + _g2b(inst.gamma[0])
            + _g1b(inst.c[i], inst.c_inf[i]) + _g2b(inst.delta[0]) for i in range(n)]
    assert vk_x[55] == bytes(64)                              # the identity row reaches ecPairing as (0, 0)
    res = evm.run_pair(engine, jobs)
    got = np.array([r == _w(1) for r in res], dtype=bool)
    assert np.array_equal(got, verify(engine, inst)) and np.array_equal(got, pools.want)


# ---- weighted ---------------------------------------------------------------------------------------------------------------------
def weights64(n, seed):
    rng = np.random.default_rng(seed)
    return [int(v) | 1 for v in rng.integers(1, 1 << 63, size=n, dtype=np.uint64)]


@pytest.mark.parametrize("n", [1, 5, 64, 300])
def test_weighted_gt_is_the_oracle_product_over_the_literal_pairs(engine, pools, n):
    w = weights64(n, 40 + n)
    good = tile(pools.valid, n)
    one_bad = M.plant(pools.valid, {0: "a_negated"}).take([0] + [1 + k % (POOL - 1) for k in range(n - 1)])      # exactly one invalid row
    for inst, want_one in ((good, True), (one_bad, False)):
        want_gt, literal = M.weighted_product(inst, w)
        assert literal, "the comparison uses non-identity literal pairs only"
        gt, is_one = weighted(engine, inst, w)
        assert np.array_equal(gt[0], want_gt) and is_one == want_one and np.array_equal(want_gt, M.ONE48) == want_one


def test_weighted_at_2049_proofs_joins_two_parts_of_every_column_sum(engine, pools):
    """2048 proofs are one part of a column sum (256 lanes of 8 rows); 2049 are two, so k_groth16_fr_sums_join adds more than one partial
    per column.  The batch is the pool tiled (row i is pool row i mod 64) under distinct odd 64-bit weights: the literal pairs are linear in
    r_i with the points and inputs fixed per pool row, so the product is the pool's under the sums of the weights that fall on each pool row,
    and canonical Gt words make the two equal word for word.  Once all valid; once with exactly ONE invalid row, the last one (the row
    past 2048), which the model carries as a 65th row under its own weight.  (The cap of 256 parts needs more than 524288 proofs: no GPU
    test reaches it, tests/test_weighted_plan.py pins it on the host.)"""
    n = 2049
    assert (n - 1 + 8 * 256 - 1) // (8 * 256) == 1 and (n + 8 * 256 - 1) // (8 * 256) == 2
    idx = np.arange(n) % POOL
    w64 = (2 * np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)        # odd times odd mod 2^64: distinct, odd
    assert len(np.unique(w64)) == n and (w64 & np.uint64(1)).all()
    w = w64.tolist()
    collapse = lambda rows: [sum(w[i] for i in rows if idx[i] == k) % M.R for k in range(POOL)]
    good = pools.valid.take(idx)
    gt, is_one = weighted(engine, good, w)
    want_gt, literal = M.weighted_product(pools.valid, collapse(range(n)))
    assert literal and np.array_equal(gt[0], want_gt) and np.array_equal(want_gt, M.ONE48) and is_one
    bad_row = n - 1
    one_bad = pools.valid.take(idx)
    one_bad.a[bad_row, 4:8] = M.limbs([M.P - M.ints(one_bad.a[bad_row, 4:8])[0]])[0]                   # A negated: that proof alone fails
    model = one_bad.take(list(range(POOL)) + [bad_row])
    want_gt, literal = M.weighted_product(model, collapse(range(n - 1)) + [w[bad_row]])
    assert literal and not np.array_equal(want_gt, M.ONE48)
    gt, is_one = weighted(engine, one_bad, w)
    assert np.array_equal(gt[0], want_gt) and not is_one


def test_weighted_inputs_and_weights_are_any_256_bit_words(engine, pools):
    """inputs r - 1, r, r + 1, p, 2^256 - 1 on the weighted path (the column sums reduce them mod r), weights of the same kind: the Gt words
    are the oracle's product over the literal pairs, and equal those of the same batch with every word reduced by hand"""
    n = 9
    inst = pools.valid.take(np.arange(n))
    words = [M.R - 1, M.R, M.R + 1, M.P, (1 << 256) - 1, (1 << 255) + 12345, 4 * M.R + 7]
    for k, v in enumerate(words):
        inst.inputs[k][k % L] = v
    inst.inputs[8] = [M.P, (1 << 256) - 1, M.R + 1]
    w = weights64(n, 91)
    w[2], w[5], w[7] = (1 << 256) - 1, M.P, M.R + 5
    want_gt, literal = M.weighted_product(inst, w)
    assert literal and not np.array_equal(want_gt, M.ONE48)           # the changed inputs make those proofs invalid
    gt, is_one = weighted(engine, inst, w)
    assert np.array_equal(gt[0], want_gt) and not is_one
    reduced = inst.take(np.arange(n))
    reduced.inputs = [[x % M.R for x in row] for row in inst.inputs]
    assert np.array_equal(weighted(engine, reduced, [v % M.R for v in w])[0], gt)
    assert np.array_equal(verify(engine, inst), verify(engine, reduced)) and np.array_equal(verify(engine, inst), M.model_verify(inst))


def test_weighted_zero_weights_shifted_weights_unit_vectors_and_empty(engine, pools):
    n = POOL
    w = weights64(n, 77)
    one_bad = M.plant(pools.valid, {4: "a_negated"})
    gt_bad, is_one = weighted(engine, one_bad, w)
    assert not is_one
    w0 = list(w)
    w0[4] = 0
    assert weighted(engine, one_bad, w0)[1]                                           # weight 0 removes the invalid proof
    gt0, one0 = weighted(engine, one_bad, [0] * n)
    assert one0 and np.array_equal(gt0[0], M.ONE48)                                   # all-zero weights: the identity
    gt_r, _ = weighted(engine, one_bad, [v + M.R for v in w])
    assert np.array_equal(gt_r, gt_bad)                                               # weights act mod r
    ok = verify(engine, pools.planted)
    for k in [0] + sorted(DEFECT_ROWS) + [22]:                                        # e_k gives the per-proof boolean
        e = [0] * n
        e[k] = 1
        assert weighted(engine, pools.planted, e)[1] == bool(ok[k]), k
    empty = pools.valid.take(np.zeros(0, dtype=np.int64))
    gt_e, one_e = weighted(engine, empty, [])
    assert one_e and np.array_equal(gt_e[0], M.ONE48)
    assert verify(engine, empty).shape == (0,)


# ---- whole-call errors ------------------------------------------------------------------------------------------------------------
def test_null_pointers_are_refused_and_nothing_is_written(engine, pools):
    inst = tile(pools.valid, 4)
    n = inst.n
    d = {k: engine.to_device_soa(v, v.shape[1]) for k, v in dict(alpha=inst.alpha, beta=inst.beta, gamma=inst.gamma, delta=inst.delta, ic=inst.ic,
                                                               a=inst.a, b=inst.b, c=inst.c).items()}
    dx = engine.to_device_soa(np.ascontiguousarray(inst.input_words().transpose(1, 0, 2)).reshape(L * n, 4), 4)
    ok = engine.to_device(np.full(n, 7, dtype=np.uint8))
    p = lambda x: ctypes.c_void_p(x.ptr) if x is not None else None
    call = lambda ic, okp: engine.lib.sylow_hip_groth16_verify_batch(p(d["alpha"]), p(d["beta"]), p(d["gamma"]), p(d["delta"]), ic, L, p(d["a"]), None, p(d["b"]),
                                                                    None, p(d["c"]), None, p(dx), n, okp, None)
    assert call(None, p(ok)) == E_ARG and (ok.download() == 7).all()
    assert call(p(d["ic"]), None) == E_ARG
    out, oi = engine.to_device(np.full(8 * n, 7, dtype=np.uint64)), engine.to_device(np.full(n, 7, dtype=np.uint8))
    assert engine.lib.sylow_hip_groth16_vk_x_batch(None, L, p(dx), n, p(out), p(oi), None) == E_ARG and (out.download() == 7).all() and (oi.download() == 7).all()
    gt, one = engine.to_device(np.full(48, 7, dtype=np.uint64)), engine.to_device(np.full(1, 7, dtype=np.uint8))
    dw = engine.to_device_soa(M.limbs(weights64(n, 1)), 4)
    rc = engine.lib.sylow_hip_groth16_batch_verify_weighted(p(d["alpha"]), p(d["beta"]), p(d["gamma"]), p(d["delta"]), None, L, p(d["a"]), None, p(d["b"]), None,
                                                            p(d["c"]), None, p(dx), p(dw), n, p(gt), p(one), None)
    assert rc == E_ARG and (gt.download() == 7).all() and one.download()[0] == 7
    assert call(p(d["ic"]), p(ok)) == 0 and (ok.download() == 1).all()               # the same arguments, complete: the call runs


def test_api_holder(engine, pools):
    from sylow_amd import api
    inst = pools.planted
    vk = api.Groth16VerifyingKey(api.G1Affine(inst.alpha), api.G2Affine(inst.beta), api.G2Affine(inst.gamma), api.G2Affine(inst.delta), api.G1Affine(inst.ic))
    assert vk.n_inputs == L
    ok = api.groth16_verify(vk, api.G1Affine(inst.a, inst.a_inf), api.G2Affine(inst.b), api.G1Affine(inst.c, inst.c_inf), inst.input_words())
    assert ok.dtype == bool and np.array_equal(ok, pools.want)
    with pytest.raises(ValueError):
        api.Groth16VerifyingKey(api.G1Affine(inst.a), api.G2Affine(inst.beta), api.G2Affine(inst.gamma), api.G2Affine(inst.delta), api.G1Affine(inst.ic))
