"""GPU parity of the two folded shapes of the aggregate verifiers (include/sylow_hip.h, "Aggregate verification"):

  committees  n_pk = c n, c >= 2: key j belongs to message j mod n, sig_i is committee i's aggregate signature; the keys of a committee
              are summed in G2 (k_g2_seg_fold) and the batch costs n + 1 Miller loops whatever c is;
  key reuse   n = c n_pk, n_pk >= 2: signature i is under key i mod n_pk; the hashes under one key are summed in G1 (k_g1_seg_fold).

The reference value is the oracle's glued_pairing over the LITERAL pairs (sig_i, G2gen), (-H(m_{j mod n}), pk_{j mod n_pk}) -- n + max(n, n_pk)
of them, with weights (w_i sig_i, G2gen), (-w_{j mod n} H, pk) -- and the Gt words must agree bit for bit.  A valid batch multiplies to the
identity under any weights (bilinearity; checked as is_one = 1 and the identity's words), so the oracle is spent where the value is not
trivial: on the same batch with ONE WRONG SIGNATURE (row 0 carries another row's, or for n = 1 another message's, signature).  Identities
follow pairing(): a flagged key adds nothing to its sum and an identity on either side of a pair contributes one, so such pairs are left out
of the oracle's list (its glued loop replays a G2 identity through the formulas instead).
Every committee / key-reuse call of this file returns SYLOW_HIP_E_ARG on a library without the feature."""
import numpy as np
import pytest

from helpers import P as PMOD, SEED, Xoshiro, fast_rand_fp_array, ints, limbs, pack, representatives
from oracle import pyref as R
from test_gpu_multi_pairing import G1, G2, proj1, proj2

pytestmark = pytest.mark.gpu

ONE = np.zeros(48, dtype=np.uint64); ONE[0] = 1
COMMITTEES = [(1, 2), (1, 3), (1, 63), (1, 64), (1, 65), (1, 1000), (3, 5), (64, 2), (257, 3), (1000, 7)]      # (n, c)
KEY_REUSE = [(2, 2), (3, 5), (64, 3), (500, 4)]                                                                # (n_pk, c)


def messages(n, tag=0):
    return [bytes([tag, i % 251, i // 251]) * (1 + i % 7) for i in range(n)]


def committees(engine, n, c, seed):
    """n committees of c signers: keys term-major (row t n + i = signer t of committee i), every signer's own signature of the committee's
    message (sylow_hip_bls_sign_batch), summed per committee (sylow_hip_g1_sum_batch)."""
    rng = Xoshiro(seed)
    sk = limbs([rng.fp() for _ in range(n * c)])
    msgs = messages(n)
    pk, _ = engine.g2_generator_mul(sk)
    each, _ = engine.bls_sign(sk, msgs * c)
    sig = np.concatenate([engine.g1_sum(each[i::n])[0] for i in range(n)], axis=0)
    return pk, msgs, sig


def key_reuse(engine, n_pk, c, seed):
    """n = c n_pk messages, message i signed under key i mod n_pk"""
    rng = Xoshiro(seed)
    sk = limbs([rng.fp() for _ in range(n_pk)])
    msgs = messages(n_pk * c, tag=1)
    pk, _ = engine.g2_generator_mul(sk)
    sig, _ = engine.bls_sign(np.tile(sk, (c, 1)), msgs)
    return pk, msgs, sig


def weights_for(n, mode, seed):
    """mode 1: 64-bit weights; mode 2: full-width (any 256-bit words, some >= p) with ONE weight 0 (n >= 2: a batch of one row keeps its weight)"""
    if mode == 0:
        return None
    rng = Xoshiro(seed)
    if mode == 1:
        return limbs([rng.next() | 1 for _ in range(n)])
    w = limbs([rng.u256() for _ in range(n)])
    if n >= 2:
        w[n // 2] = 0
    return w


def oracle_gt(coracle, pk, msgs, sig, w=None, pk_inf=None, sig_inf=None):
    """glued_pairing over the literal pairs; pairs with an identity on either side are left out (pairing() gives one for them)"""
    n, n_pk = len(msgs), pk.shape[0]
    h, h_inf = coracle.g1_to_affine(coracle.hash_to_curve(msgs))
    nh = h.copy(); nh[:, 4:] = coracle.fp_op("neg", h[:, 4:])
    s_inf = np.zeros(n, np.uint8) if sig_inf is None else np.asarray(sig_inf, np.uint8)
    s = sig
    if w is not None:
        w = limbs([v % PMOD for v in ints(w)])              # weights are Fp values: words >= p are reduced like Fp::new
        s, s_inf = coracle.g1_to_affine(coracle.g1_scalar_mul(proj1(sig, s_inf), w))
        nh, h_inf = coracle.g1_to_affine(coracle.g1_scalar_mul(proj1(nh, h_inf), w))
    m = max(n, n_pk)
    j = np.arange(m)
    q_inf = np.zeros(n_pk, np.uint8) if pk_inf is None else np.asarray(pk_inf, np.uint8)
    p = np.concatenate([s, nh[j % n]])
    q = np.concatenate([np.repeat(pack(G2, 16), n, 0), pk[j % n_pk]])
    keep = np.concatenate([np.asarray(s_inf) == 0, (np.asarray(h_inf)[j % n] == 0) & (q_inf[j % n_pk] == 0)])
    if not keep.any():
        return ONE
    p, q = p[keep], q[keep]
    return coracle.glued_pairing(proj1(p), proj2(q), np.array([0, p.shape[0]], dtype=np.uint64))[0]


def verify(engine, pk, msgs, sig, w=None, pk_inf=None, sig_inf=None):
    """the _verify_ entry point of the (un)weighted form -> (gt [48], is_one)"""
    if w is None:
        gt, ok = engine.bls_aggregate_verify(pk, msgs, sig, pk_inf=pk_inf, sig_inf=sig_inf)
    else:
        gt, ok = engine.bls_batch_verify_weighted(pk, msgs, sig, w, pk_inf=pk_inf, sig_inf=sig_inf)
    return np.asarray(gt).reshape(48), int(ok)


def partial_route(engine, shards):
    """the _partial_ entry point per shard + sylow_hip_fp12_product_final_exp -> (gt [48], is_one)"""
    parts = np.concatenate([engine.bls_aggregate_partial(pk, msgs, sig, weights=w) for pk, msgs, sig, w in shards], axis=0)
    gt, ok = engine.fp12_product_final_exp(parts)
    return np.asarray(gt).reshape(48), int(ok)


def cut_rows(pk, msgs, sig, w, lo, hi, n_pk_period):
    """message rows [lo, hi) of a batch with their keys: whole committees (n_pk_period = 0) or whole periods of a key-reuse batch"""
    n = len(msgs)
    if n_pk_period:
        assert lo % n_pk_period == 0 and hi % n_pk_period == 0
        keys = pk
    else:
        keys = pk.reshape(-1, n, 16)[:, lo:hi].reshape(-1, 16)
    return keys, msgs[lo:hi], sig[lo:hi], None if w is None else w[lo:hi]


def check_case(engine, coracle, pk, msgs, sig, period, seed):
    n = len(msgs)
    bad = sig.copy()
    bad[0] = sig[1] if n >= 2 else engine.bls_sign(limbs([7]), [b"another message"])[0][0]
    for mode in (0, 1, 2):
        w = weights_for(n, mode, seed + mode)
        gt, ok = verify(engine, pk, msgs, sig, w)
        assert ok == 1 and np.array_equal(gt, ONE), (n, pk.shape[0], mode)
        exp = oracle_gt(coracle, pk, msgs, bad, w)
        gt_b, ok_b = verify(engine, pk, msgs, bad, w)
        assert np.array_equal(gt_b, exp) and ok_b == 0 and not np.array_equal(exp, ONE), (n, pk.shape[0], mode, "verify")
        gt_p, ok_p = partial_route(engine, [(pk, msgs, bad, w)])
        assert np.array_equal(gt_p, exp) and ok_p == ok_b, (n, pk.shape[0], mode, "partial")
        unit = period if period else 1
        if n >= 2 * unit:                                   # two shards of whole committees / whole periods, combined
            mid = (n // unit // 2) * unit
            gt_s, ok_s = partial_route(engine, [cut_rows(pk, msgs, bad, w, 0, mid, period), cut_rows(pk, msgs, bad, w, mid, n, period)])
            assert np.array_equal(gt_s, exp) and ok_s == ok_b, (n, pk.shape[0], mode, "shards")


def raw_verify(engine, pk, n_pk, msgs, sig, pk_inf=None):
    """sylow_hip_bls_aggregate_verify_batch through Engine._call: no host-side shape check in the way"""
    n = len(msgs)
    dm, doff = engine._msgs(msgs)
    dpk = engine.to_device_soa(pk, 16) if pk.shape[0] else None
    dsig = engine.to_device_soa(sig, 8) if n else None
    dpi = engine._flags(pk_inf, n_pk) if pk_inf is not None else None
    dgt, done = engine.empty((48, 1)), engine.empty((1,), np.uint8)
    engine._call("sylow_hip_bls_aggregate_verify_batch", engine._ptr(dpk), engine._ptr(dpi), n_pk, dm.ptr, doff.ptr, engine._ptr(dsig), None, n, None, dgt.ptr, done.ptr)
    return engine.from_device_soa(dgt)[0], int(done.download()[0])


def test_one_message_eight_signers_is_accepted(engine):
    """n = 1, n_pk = 8: SYLOW_HIP_E_ARG before the committee shape existed; now the identity for a valid committee, through the raw entry
    point and through the host layers."""
    pk, msgs, sig = committees(engine, 1, 8, SEED + 300)
    gt, ok = raw_verify(engine, pk, 8, msgs, sig)
    assert ok == 1 and np.array_equal(gt, ONE)
    gt, ok = engine.bls_aggregate_verify(pk, msgs, sig)
    assert ok == 1 and np.array_equal(gt, ONE)
    from sylow_amd import api
    keys, one_sig = api.G2Affine(pk), api.G1Affine(sig)
    assert api.fast_aggregate_verify(keys, msgs[0], one_sig) is True
    assert api.fast_aggregate_verify(keys, b"not the message", one_sig) is False
    assert api.aggregate_verify(keys, msgs, one_sig) is True
    # individual signatures are summed first
    rng = Xoshiro(SEED + 300)
    sk = limbs([rng.fp() for _ in range(8)])
    each, _ = engine.bls_sign(sk, msgs * 8)
    assert api.fast_aggregate_verify(keys, msgs[0], api.G1Affine(each)) is True


@pytest.mark.parametrize("n,c", COMMITTEES)
def test_committees_bit_exact_vs_oracle(engine, coracle, n, c):
    pk, msgs, sig = committees(engine, n, c, SEED + 310 + 7 * n + c)
    check_case(engine, coracle, pk, msgs, sig, 0, SEED + 320 + n + c)


@pytest.mark.parametrize("n_pk,c", KEY_REUSE)
def test_key_reuse_bit_exact_vs_oracle(engine, coracle, n_pk, c):
    pk, msgs, sig = key_reuse(engine, n_pk, c, SEED + 330 + 7 * n_pk + c)
    check_case(engine, coracle, pk, msgs, sig, n_pk, SEED + 340 + n_pk + c)


def test_rejections(engine, coracle):
    """one wrong committee signature, one key replaced, one key moved to another committee, one key dropped by its flag: is_one = 0 and the
    Gt is still the oracle's"""
    n, c = 5, 4
    pk, msgs, sig = committees(engine, n, c, SEED + 350)
    other, _ = engine.g2_generator_mul(limbs([0xC0FFEE]))
    wrong = sig.copy(); wrong[2] = sig[3]
    replaced = pk.copy(); replaced[1 * n + 2] = other[0]
    moved = pk.copy(); moved[[2 * n + 0, 2 * n + 1]] = pk[[2 * n + 1, 2 * n + 0]]          # signer 2 of committees 0 and 1 change places
    flag = np.zeros(n * c, np.uint8); flag[3 * n + 4] = 1
    for keys, s, inf in ((pk, wrong, None), (replaced, sig, None), (moved, sig, None), (pk, sig, flag)):
        for w in (None, weights_for(n, 1, SEED + 351)):
            gt, ok = verify(engine, keys, msgs, s, w, pk_inf=inf)
            assert ok == 0 and np.array_equal(gt, oracle_gt(coracle, keys, msgs, s, w, pk_inf=inf))
    # key reuse: a wrong signature, a replaced key
    pk, msgs, sig = key_reuse(engine, 3, 4, SEED + 352)
    wrong = sig.copy(); wrong[7] = sig[8]
    replaced = pk.copy(); replaced[1] = other[0]
    for keys, s in ((pk, wrong), (replaced, sig)):
        gt, ok = verify(engine, keys, msgs, s)
        assert ok == 0 and np.array_equal(gt, oracle_gt(coracle, keys, msgs, s))


def test_identities(engine, coracle):
    """flagged keys with garbage coordinate words, a committee made of (pk, -pk) pairs, every key flagged, an identity signature"""
    n, c = 3, 6
    pk, msgs, sig = committees(engine, n, c, SEED + 360)
    g = np.random.default_rng(SEED % (1 << 32))
    # flagged rows hold garbage (any 256-bit words): they must be loaded as the identity, never through their words
    flag = np.zeros(n * c, np.uint8); flag[[0 * n + 1, 4 * n + 1, 2 * n + 2]] = 1
    junk = pk.copy()
    junk[flag == 1] = g.integers(0, 1 << 63, size=(3, 16), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    exp = oracle_gt(coracle, pk, msgs, sig, pk_inf=flag)
    gt_a, ok_a = verify(engine, pk, msgs, sig, pk_inf=flag)
    gt_b, ok_b = verify(engine, junk, msgs, sig, pk_inf=flag)
    assert ok_a == ok_b == 0 and np.array_equal(gt_a, exp) and np.array_equal(gt_b, exp)
    # committee 1 = three (pk, -pk) pairs: its key sum is the identity and its pair contributes one -- the product is what the OTHER pairs give
    neg = pk.copy()
    for t in (1, 3, 5):
        src = pk[(t - 1) * n + 1]
        neg[t * n + 1, :8] = src[:8]
        neg[t * n + 1, 8:] = limbs([(PMOD - y) % PMOD for y in [sum(int(src[8 + 4 * k + q]) << (64 * q) for q in range(4)) for k in range(2)]]).reshape(8)
    gone = np.zeros(n * c, np.uint8); gone[np.arange(c) * n + 1] = 1
    exp = oracle_gt(coracle, neg, msgs, sig)                               # the literal pairs: e(-H_1, pk) e(-H_1, -pk) = 1 in Gt
    assert np.array_equal(exp, oracle_gt(coracle, neg, msgs, sig, pk_inf=gone))
    gt, ok = verify(engine, neg, msgs, sig)
    assert ok == 0 and np.array_equal(gt, exp)
    # every key flagged: only e(sum sig, G2gen) is left
    allf = np.ones(n * c, np.uint8)
    gt, ok = verify(engine, junk, msgs, sig, pk_inf=allf)
    assert ok == 0 and np.array_equal(gt, oracle_gt(coracle, pk, msgs, sig, pk_inf=allf))
    # an identity signature (flagged, garbage words)
    sinf = np.array([0, 1, 0], np.uint8)
    sj = sig.copy(); sj[1] = junk[1, :8]
    for w in (None, weights_for(n, 1, SEED + 361)):
        gt, ok = verify(engine, pk, msgs, sj, w, sig_inf=sinf)
        assert ok == 0 and np.array_equal(gt, oracle_gt(coracle, pk, msgs, sig, w, sig_inf=sinf))
    # ... and with weight 0 on that very row committee 1 leaves the test altogether: what is left is valid
    w = weights_for(n, 2, SEED + 361)
    assert not w[1].any()
    gt, ok = verify(engine, pk, msgs, sj, w, sig_inf=sinf)
    assert ok == 1 and np.array_equal(gt, ONE) and np.array_equal(gt, oracle_gt(coracle, pk, msgs, sig, w, sig_inf=sinf))
    # key reuse with a flagged key
    pk2, msgs2, sig2 = key_reuse(engine, 2, 3, SEED + 362)
    gt, ok = verify(engine, pk2, msgs2, sig2, pk_inf=[0, 1])
    assert ok == 0 and np.array_equal(gt, oracle_gt(coracle, pk2, msgs2, sig2, pk_inf=[0, 1]))


def test_committee_call_agrees_with_the_per_row_call(engine):
    """2^14 signers of one message: the committee call (n = 1, the summed signature) and the call that existed before (n = n_pk rows, the
    message repeated, the individual signatures) give the same 48 words -- for the valid set and with one signature replaced"""
    m = 1 << 14
    sk = fast_rand_fp_array(SEED + 370, m, 1)
    msg = b"one message, many signers"
    pk, _ = engine.g2_generator_mul(sk)
    each, _ = engine.bls_sign(sk, [msg] * m)
    for bad in (False, True):
        sigs = each.copy()
        if bad:
            sigs[1234] = each[4321]
        total, tinf = engine.g1_sum(sigs)
        gt_c, ok_c = engine.bls_aggregate_verify(pk, [msg], total, sig_inf=tinf)
        gt_r, ok_r = engine.bls_aggregate_verify(pk, [msg] * m, sigs)
        assert np.array_equal(gt_c, gt_r) and ok_c == ok_r == (0 if bad else 1)
        assert np.array_equal(gt_c, ONE) == (not bad)


def test_input_contract_of_the_key_words(engine):
    """key words x + k p give bit-identical gt_out / is_one (Fp::new reduces); NULL pk_inf equals all-zero flags"""
    for pk, msgs, sig in (committees(engine, 3, 5, SEED + 380), key_reuse(engine, 3, 5, SEED + 381)):
        bad = sig.copy(); bad[0] = sig[1]
        for s in (sig, bad):
            gt, ok = verify(engine, pk, msgs, s)
            for reps in (representatives(pk, seed=5), representatives(pk, largest=True)):
                gt_r, ok_r = verify(engine, reps, msgs, s)
                assert np.array_equal(gt_r, gt) and ok_r == ok
            gt_z, ok_z = verify(engine, pk, msgs, s, pk_inf=np.zeros(pk.shape[0], np.uint8))
            assert np.array_equal(gt_z, gt) and ok_z == ok
            w = weights_for(len(msgs), 1, SEED + 382)
            gt_w, ok_w = verify(engine, pk, msgs, s, w)
            gt_wr, ok_wr = verify(engine, representatives(pk, seed=6), msgs, s, w)
            assert np.array_equal(gt_wr, gt_w) and ok_wr == ok_w


def _column_sums_mod_r(a):
    """sum over axis 0 of 256-bit values [m, k, 4] (uint64 limbs) mod r -> [k, 4] limbs"""
    lo = (a & np.uint64(0xFFFFFFFF)).sum(axis=0, dtype=np.uint64)
    hi = (a >> np.uint64(32)).sum(axis=0, dtype=np.uint64)
    vals = [sum((int(lo[j, q]) + (int(hi[j, q]) << 32)) << (64 * q) for q in range(4)) % R.R_ORDER for j in range(a.shape[1])]
    return limbs(vals)


@pytest.mark.parametrize("n,c", [(1, 1 << 20), (1 << 10, 1 << 10)])
def test_full_size(engine, n, c):
    """keys a_j G2gen and the signature under sum_j a_j mod r (no oracle pairing needed): is_one = 1; with one key's flag set, 0"""
    sk = fast_rand_fp_array(SEED + 390 + n, n * c, 1)
    pk, _ = engine.g2_generator_mul(sk)
    msgs = messages(n, tag=2)
    sig, _ = engine.bls_sign(_column_sums_mod_r(sk.reshape(c, n, 4)), msgs)
    gt, ok = engine.bls_aggregate_verify(pk, msgs, sig)
    assert ok == 1 and np.array_equal(gt, ONE)
    flag = np.zeros(n * c, np.uint8); flag[(c // 3) * n + n // 2] = 1
    gt, ok = engine.bls_aggregate_verify(pk, msgs, sig, pk_inf=flag)
    assert ok == 0 and not np.array_equal(gt, ONE)


def test_argument_errors(engine):
    from sylow_amd._lib import SylowHipError
    pk, _ = engine.g2_generator_mul(limbs(list(range(1, 9))))
    sig, _ = engine.g1_generator_mul(limbs(list(range(1, 9))))
    for n, n_pk in ((6, 4), (4, 6), (5, 0)):
        with pytest.raises(SylowHipError, match="bad argument"):
            raw_verify(engine, pk[:max(n_pk, 1)], n_pk, messages(n), sig[:n])
        assert not engine.aggregate_shape_ok(n, n_pk)
    for n_pk in (0, 1, 5, 8):                               # n = 0: the identity for any n_pk
        gt, ok = raw_verify(engine, pk[:n_pk], n_pk, [], sig[:0])
        assert ok == 1 and np.array_equal(gt, ONE)
