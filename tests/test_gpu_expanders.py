"""Hashing, signing and verifying under a caller-chosen RFC 9380 expander and tag (sylow_hip_*_expander_batch, sylow_hip_expand_message_batch,
sylow_hip_bls_verify_hashed_batch) on the GPU, judged row by row by the byte-level model of tests/expander_model.py (hashlib + the
oracle's Keccak-256, SvdW map and group law) and by the reference's own RFC 9380 literals (tests/golden/expander_kats.json)."""
import json
import os

import numpy as np
import pytest

import expander_model as M
from helpers import fast_rand_fp_array, ints, limbs, pack
from oracle import pyref as R
from test_hash_chain import load_chain, words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "expander_kats.json")))["vectors"]
EXPANDERS = [M.XMD_KECCAK256, M.XMD_SHA256, M.XOF_SHAKE128]
G1 = [1, 2]
G2 = list(R.G2_GEN_AFF[0]) + list(R.G2_GEN_AFF[1])
# the longest tag whose b_i is one block, and the first that is not: 33 + (len + 1) + 9 <= 64 (SHA-256), 33 + (len + 1) <= 135 (Keccak-256);
# SHAKE128 has no b_i: the pair around its rate less a short message
ONE_BLOCK_EDGE = {M.XMD_KECCAK256: (101, 102), M.XMD_SHA256: (21, 22), M.XOF_SHAKE128: (164, 165)}


def rows(rng, lengths):
    return [rng.integers(0, 256, size=int(l), dtype=np.uint8).tobytes() for l in lengths]


def check_expand(engine, e, msgs, dst, length, k=128):
    got = engine.expand_message(msgs, length, e, dst, k)
    assert got.shape == (len(msgs), length)
    tag = R.DST if dst is None else dst
    for i, m in enumerate(msgs):                       # every row
        assert got[i].tobytes() == M.expand_message(e, m, tag, length, k), (M.NAMES[e], i, len(m), len(tag), length)


def model_points(e, msgs, dst=R.DST):
    pts = [M.hash_to_curve_affine(e, m, dst) for m in msgs]
    assert all(p is not None for p in pts)
    return pack([c for p in pts for c in p], 8)


def proj1(xy):
    one = np.zeros((xy.shape[0], 4), dtype=np.uint64); one[:, 0] = 1
    return np.concatenate([xy, one], axis=1)


def test_reference_literals_inside_a_batch(engine):
    rng = np.random.default_rng(1)
    for key in sorted({v["set"] for v in KATS}):
        vs = [v for v in KATS if v["set"] == key]
        filler = rows(rng, [5, 70, 0, 200])
        msgs = filler[:2] + [v["msg"].encode() for v in vs] + filler[2:]
        got = engine.expand_message(msgs, 0x20, vs[0]["expander_id"], vs[0]["dst"].encode(), 128)
        for j, v in enumerate(vs):
            assert got[2 + j].tobytes().hex() == v["expected"], (key, v["msg"][:8])


@pytest.mark.parametrize("e", EXPANDERS, ids=M.NAMES.get)
def test_expand_message_ragged_lengths(engine, e):
    """message lengths 0 .. 200 (every residue of the end of msg' modulo 64, 136 and 168, so every block edge of the three hashes) and up to 600"""
    rng = np.random.default_rng(10 + e)
    msgs = rows(rng, list(range(0, 201)) + [255, 256, 300, 447, 448, 511, 512, 600])
    check_expand(engine, e, msgs, None, 96)
    check_expand(engine, e, msgs, b"QUUX-V01-CS02-with-expander-x", 32)


@pytest.mark.parametrize("e", EXPANDERS, ids=M.NAMES.get)
def test_expand_message_output_lengths(engine, e):
    rng = np.random.default_rng(20 + e)
    msgs = rows(rng, [0, 3, 64, 133, 200] if e == M.XMD_KECCAK256 else [0, 1, 3, 55, 56, 64, 133, 135, 136, 167, 168, 200])
    for length in (1, 31, 32, 33, 48, 96, 128, 167, 168, 169, 255, 8160):
        check_expand(engine, e, msgs, b"len-sweep", length)
    if e == M.XOF_SHAKE128:
        check_expand(engine, e, msgs[:3], b"len-sweep", 65535)


def test_xmd_refuses_8161_bytes(engine):
    import sylow_amd
    for e in (M.XMD_KECCAK256, M.XMD_SHA256):
        with pytest.raises(sylow_amd.SylowHipError, match="> 255"):
            engine.expand_message([b"abc"], 8161, e, b"tag")
    check_expand(engine, M.XOF_SHAKE128, [b"abc"], b"tag", 8161)


@pytest.mark.parametrize("e", EXPANDERS, ids=M.NAMES.get)
def test_expand_message_tag_lengths(engine, e):
    rng = np.random.default_rng(30 + e)
    msgs = rows(rng, [0, 1, 2, 3, 31, 32, 33, 64, 100, 133, 136, 168, 200, 300])
    for tl in (1,) + ONE_BLOCK_EDGE[e] + (255, 256, 300):
        dst = rng.integers(0, 256, size=tl, dtype=np.uint8).tobytes()
        check_expand(engine, e, msgs, dst, 96)
        check_expand(engine, e, msgs, dst, 32)
    check_expand(engine, M.XOF_SHAKE128, msgs[:4], bytes(300), 64, k=1020)        # a 255-byte shortened tag


@pytest.mark.parametrize("e", EXPANDERS, ids=M.NAMES.get)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_expand_message_batch_sizes(engine, e, n):
    rng = np.random.default_rng(40 + e + n)
    check_expand(engine, e, rows(rng, rng.integers(0, 80, size=n)), None, 48)


def test_expander_zero_is_the_existing_suite_bit_for_bit(engine):
    rng = np.random.default_rng(50)
    for n in (1, 300, 17000):                        # 17000: past the eight-lanes-per-message route of the existing entry point
        msgs = rows(rng, rng.integers(0, 150, size=n))
        for dst in (None, b"another-tag", bytes(range(200)), bytes(300)):
            assert np.array_equal(engine.hash_to_field(msgs, dst, expander=0), engine.hash_to_field(msgs, dst))
            a, ai = engine.hash_to_g1(msgs, dst, expander=0)
            b, bi = engine.hash_to_g1(msgs, dst)
            assert np.array_equal(a, b) and np.array_equal(ai, bi)
            if n == 300:
                em = engine.expand_message(msgs, 96, 0, dst)
                u = engine.hash_to_field(msgs, dst)
                exp = [[int.from_bytes(r[48 * j:48 * j + 48].tobytes(), "big") % R.P for j in range(2)] for r in em]
                assert np.array_equal(u, pack([v for pair in exp for v in pair], 8))
    ch = load_chain()
    for name, hexdst in ch["dsts"].items():
        es = [x for x in ch["entries"] if x["dst"] == name]
        msgs = [bytes.fromhex(x["msg"]) for x in es]
        d = None if name == "sylow" else bytes.fromhex(hexdst)
        assert np.array_equal(engine.hash_to_field(msgs, d, expander="xmd_keccak256"), words([[x["u0"], x["u1"]] for x in es])), name
        h, inf = engine.hash_to_g1(msgs, d, expander="xmd_keccak256")
        assert not inf.any() and np.array_equal(h, words([x["h"] for x in es])), name
        if name == "sylow":
            s, inf = engine.bls_sign(words([[x["sk"]] for x in es]), msgs, expander=0)
            assert not inf.any() and np.array_equal(s, words([x["sig"] for x in es]))
            s, inf = engine.bls_sign(words([[x["sk"]] for x in es]), msgs, expander=0, dst=bytes.fromhex(hexdst))      # the two-launch route
            assert not inf.any() and np.array_equal(s, words([x["sig"] for x in es]))


@pytest.mark.parametrize("e", [M.XMD_SHA256, M.XOF_SHAKE128], ids=M.NAMES.get)
def test_hash_to_field_and_g1_against_the_model(engine, e):
    rng = np.random.default_rng(60 + e)
    msgs = rows(rng, list(range(0, 140)) + [167, 168, 169, 255, 256, 600])
    for dst in (None, b"BN254G1_XMD:SHA-256_SVDW_RO_TESTS", b"t", bytes(range(21)), bytes(range(22)), bytes(256)):
        tag = R.DST if dst is None else dst
        sub = msgs if dst is None else msgs[::7]
        u = engine.hash_to_field(sub, dst, expander=e)
        assert np.array_equal(u, pack([v for m in sub for v in M.hash_to_field(e, m, tag)], 8))
        h, inf = engine.hash_to_g1(sub, dst, expander=e)
        assert not inf.any() and np.array_equal(h, model_points(e, sub, tag))
        c = ints(h)
        assert all(R.g1_is_on_curve_affine(c[2 * i], c[2 * i + 1]) for i in range(len(sub)))


@pytest.mark.parametrize("e", [M.XMD_SHA256, M.XOF_SHAKE128], ids=M.NAMES.get)
def test_sign_is_the_oracles_product_of_the_models_hash(engine, coracle, e):
    rng = np.random.default_rng(70 + e)
    for n, dst in ((1, None), (37, b"sig-tag"), (300, bytes(260))):
        msgs = rows(rng, rng.integers(0, 100, size=n))
        sk = limbs([int.from_bytes(rng.bytes(32), "big") % R.R_ORDER for _ in range(n)])
        sig, inf = engine.bls_sign(sk, msgs, expander=e, dst=dst)
        exp, einf = coracle.g1_to_affine(coracle.g1_scalar_mul(proj1(model_points(e, msgs, R.DST if dst is None else dst)), sk))
        assert np.array_equal(sig, exp) and np.array_equal(inf, einf)


def keys(engine, sk):
    pk, inf = engine.g2_scalar_mul(np.repeat(pack(G2, 16), sk.shape[0], 0), sk)
    assert not inf.any()
    return pk


def test_verify_expander_valid_forged_and_cross_suite(engine):
    rng = np.random.default_rng(80)
    n = 200
    msgs = rows(rng, rng.integers(0, 90, size=n))
    sk = limbs([int.from_bytes(rng.bytes(32), "big") % R.R_ORDER for _ in range(n)])
    pk = keys(engine, sk)
    tag = b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"
    for e in (M.XMD_SHA256, M.XOF_SHAKE128):
        sig, _ = engine.bls_sign(sk, msgs, expander=e, dst=tag)
        assert engine.bls_verify(pk, msgs, sig, expander=e, dst=tag).all()
        forged = rng.random(n) < 0.2
        bad = sig.copy()
        bad[forged] = engine.g1_add(sig[forged], np.repeat(pack(G1, 8), int(forged.sum()), 0))[0]
        assert np.array_equal(engine.bls_verify(pk, msgs, bad, expander=e, dst=tag).astype(bool), ~forged)
    sig, _ = engine.bls_sign(sk, msgs, expander=M.XMD_SHA256, dst=tag)
    assert not engine.bls_verify(pk, msgs, sig, expander=M.XMD_KECCAK256, dst=tag).any()
    assert not engine.bls_verify(pk, msgs, sig, expander=M.XOF_SHAKE128, dst=tag).any()
    assert not engine.bls_verify(pk, msgs, sig, expander=M.XMD_SHA256, dst=tag + b"x").any()
    assert not engine.bls_verify(pk, msgs, sig, pipelined=False).any()


def test_verify_expander_identities_read_as_bls_verify_batch(engine):
    rng = np.random.default_rng(81)
    n = 64
    msgs = rows(rng, rng.integers(0, 60, size=n))
    sk = limbs([int.from_bytes(rng.bytes(32), "big") % R.R_ORDER for _ in range(n)])
    pk = keys(engine, sk)
    pki, sigi = (rng.random(n) < 0.3).astype(np.uint8), (rng.random(n) < 0.3).astype(np.uint8)
    pki[:2], sigi[:2] = 1, 1                                                   # both identities: 1 == 1
    sig0, _ = engine.bls_sign(sk, msgs)
    base = engine.bls_verify(pk, msgs, sig0, pk_inf=pki, sig_inf=sigi, pipelined=False)
    assert base[:2].all() and not base.all()
    assert np.array_equal(engine.bls_verify(pk, msgs, sig0, pk_inf=pki, sig_inf=sigi, expander=0), base)
    for e in (M.XMD_SHA256, M.XOF_SHAKE128):
        sig, _ = engine.bls_sign(sk, msgs, expander=e)
        assert np.array_equal(engine.bls_verify(pk, msgs, sig, pk_inf=pki, sig_inf=sigi, expander=e), base)


@pytest.mark.parametrize("n", [5, 4500, 17000], ids=["one-wavefront", "lane-quads", "rounds-and-tail"])
def test_verify_expander_zero_on_each_size_route(engine, n):
    """sylow_hip_bls_verify_batch picks by size (up to 4096: a wavefront per loop; up to 16384: a lane quad per element; above: whole rounds on
    lane pairs + a quad tail); expander 0 with a NULL tag answers the same flags on each, forged rows included."""
    assert engine.get_option("WIDE_VERIFY_MAX") < 0 and engine.get_option("QUAD_MAX") < 0 and engine.get_option("TAIL_SPLIT") < 0    # the defaults
    rng = np.random.default_rng(82 + n)
    d = min(n, 256)
    msgs_d = rows(rng, rng.integers(0, 70, size=d))
    sk = limbs([int.from_bytes(rng.bytes(32), "big") % R.R_ORDER for _ in range(d)])
    pk_d, (sig_d, _) = keys(engine, sk), engine.bls_sign(sk, msgs_d)
    idx = np.arange(n) % d
    sig = sig_d[idx].copy()
    forged = rng.random(n) < 0.1
    sig[forged] = sig_d[(idx[forged] + 1) % d]
    msgs = [msgs_d[i] for i in idx]
    base = engine.bls_verify(pk_d[idx], msgs, sig, pipelined=False)
    assert np.array_equal(base.astype(bool), ~forged)
    assert np.array_equal(engine.bls_verify(pk_d[idx], msgs, sig, expander=0), base)
    sig1, _ = engine.bls_sign(sk, msgs_d, expander=M.XMD_SHA256)
    sig = sig1[idx].copy()
    sig[forged] = sig1[(idx[forged] + 1) % d]
    assert np.array_equal(engine.bls_verify(pk_d[idx], msgs, sig, expander=M.XMD_SHA256), base)


def test_verify_hashed(engine, coracle):
    rng = np.random.default_rng(90)
    n = 150
    msgs = rows(rng, rng.integers(0, 90, size=n))
    sk = limbs([int.from_bytes(rng.bytes(32), "big") % R.R_ORDER for _ in range(n)])
    pk = keys(engine, sk)
    forged = rng.random(n) < 0.2
    for e in EXPANDERS:
        sig, _ = engine.bls_sign(sk, msgs, expander=e, dst=b"hashed")
        sig[forged] = engine.g1_add(sig[forged], np.repeat(pack(G1, 8), int(forged.sum()), 0))[0]
        h, hinf = engine.hash_to_g1(msgs, b"hashed", expander=e)
        want = engine.bls_verify(pk, msgs, sig, expander=e, dst=b"hashed")
        assert np.array_equal(want.astype(bool), ~forged)
        assert np.array_equal(engine.bls_verify_hashed(pk, h, sig), want)
        assert np.array_equal(engine.bls_verify_hashed(pk, h, sig, h_inf=hinf), want)
    # H from the oracle alone: another hash-to-curve as far as the library knows (SHA-256 XMD of a tag it never sees)
    h = model_points(M.XMD_SHA256, msgs, b"oracle-only")
    sig, _ = coracle.g1_to_affine(coracle.g1_scalar_mul(proj1(h), sk))
    assert engine.bls_verify_hashed(pk, h, sig).all()
    assert not engine.bls_verify_hashed(pk, h, np.roll(sig, 1, axis=0)).any()
    # h_inf = 1: the right-hand pairing is the identity -- ok exactly where the signature is the identity too
    hinf, sigi = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    hinf[::3] = 1; sigi[::6] = 1
    got = engine.bls_verify_hashed(pk, h, sig, h_inf=hinf, sig_inf=sigi)
    assert np.array_equal(got.astype(bool), (hinf == sigi))


def test_one_large_launch_sha256(engine, coracle):
    """2^18 messages through SHA-256 hash_to_g1 and verify in single launches; 256 sampled rows against the model"""
    n = 1 << 18
    g = np.random.default_rng(100)
    tag = b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"
    blob = g.integers(0, 256, size=(n, 32), dtype=np.uint8)
    dm, doff = engine.to_device(blob.reshape(-1)), engine.to_device(np.arange(n + 1, dtype=np.uint64) * np.uint64(32))
    sk_aos = fast_rand_fp_array(101, n, 1)
    sk = engine.to_device_soa(sk_aos, 4)
    g2 = engine.to_device_soa(np.repeat(pack(G2, 16), n, 0), 16)
    pk, pki = engine.empty((16, n)), engine.empty((n,), np.uint8)
    h, hi = engine.empty((8, n)), engine.empty((n,), np.uint8)
    sig, sigi = engine.empty((8, n)), engine.empty((n,), np.uint8)
    engine._call("sylow_hip_g2_scalar_mul_batch", g2.ptr, None, sk.ptr, pk.ptr, pki.ptr, n)
    engine._call("sylow_hip_hash_to_g1_expander_batch", M.XMD_SHA256, dm.ptr, doff.ptr, tag, len(tag), 128, h.ptr, hi.ptr, n)
    engine._call("sylow_hip_bls_sign_expander_batch", M.XMD_SHA256, tag, len(tag), 128, sk.ptr, dm.ptr, doff.ptr, sig.ptr, sigi.ptr, n)
    idx = np.sort(g.choice(n, 256, replace=False))
    smsgs = [blob[i].tobytes() for i in idx]
    exp_h = model_points(M.XMD_SHA256, smsgs, tag)
    h_aos, sig_aos = engine.from_device_soa(h), engine.from_device_soa(sig)
    assert not hi.download().any() and not sigi.download().any()
    assert np.array_equal(h_aos[idx], exp_h)
    exp_sig, _ = coracle.g1_to_affine(coracle.g1_scalar_mul(proj1(exp_h), sk_aos[idx]))
    assert np.array_equal(sig_aos[idx], exp_sig)
    plant = g.random(n) < 1 / 1024
    plant[idx[:32]] = True
    sig_aos[plant] = engine.g1_add(sig_aos[plant], np.repeat(pack(G1, 8), int(plant.sum()), 0))[0]
    sig2, ok = engine.to_device_soa(sig_aos, 8), engine.empty((n,), np.uint8)
    engine._call("sylow_hip_bls_verify_expander_batch", M.XMD_SHA256, tag, len(tag), 128, pk.ptr, None, dm.ptr, doff.ptr, sig2.ptr, None, ok.ptr, n)
    flags = ok.download().astype(bool)
    assert np.array_equal(flags, ~plant)
    # the sampled rows' flags by the oracle's two pairings on the model's hash
    pk_aos = engine.from_device_soa(pk)[idx]
    one4 = np.zeros((256, 4), dtype=np.uint64); one4[:, 0] = 1
    zero4 = np.zeros((256, 4), dtype=np.uint64)
    lhs = coracle.pairing(proj1(sig_aos[idx]), np.concatenate([np.repeat(pack(G2, 16), 256, 0), one4, zero4], axis=1))
    rhs = coracle.pairing(proj1(exp_h), np.concatenate([pk_aos, one4, zero4], axis=1))
    assert np.array_equal(flags[idx], (lhs == rhs).all(axis=1))
    engine._call("sylow_hip_bls_verify_hashed_batch", pk.ptr, None, h.ptr, hi.ptr, sig2.ptr, None, ok.ptr, n)
    assert np.array_equal(ok.download().astype(bool), ~plant)


def test_public_layer_round_trip(engine):
    """sylow_amd.api: the expander classes, and expander=None leaving every existing call as it is"""
    from sylow_amd import api
    api.set_engine(engine)
    msgs = [b"", b"abc", bytes(100), b"q" * 133]
    kp = api.KeyPair.generate(len(msgs), seed=11)
    for ex, e in ((api.XMDExpander("sha256", b"api-tag"), M.XMD_SHA256), (api.XOFExpander("shake128", b"api-tag", k=128), M.XOF_SHAKE128),
                  (api.XMDExpander("keccak256", b"api-tag"), M.XMD_KECCAK256)):
        em = ex.expand_message(msgs, 40)
        assert [r.tobytes() for r in em] == [M.expand_message(e, m, b"api-tag", 40) for m in msgs]
        assert np.array_equal(ex.hash_to_field(msgs), pack([v for m in msgs for v in M.hash_to_field(e, m, b"api-tag")], 8))
        h = api.G1Projective.hash_to_curve(msgs, expander=ex)
        assert np.array_equal(h.xy, model_points(e, msgs, b"api-tag"))
        sig = api.sign(kp.secret_key, msgs, expander=ex)
        assert api.verify(kp.public_key, msgs, sig, expander=ex).all()
        assert api.verify_hashed(kp.public_key, h, sig).all()
        assert not api.verify(kp.public_key, msgs, sig).any()
    sig = api.sign(kp.secret_key, msgs)
    assert api.verify(kp.public_key, msgs, sig).all()
    assert np.array_equal(api.G1Projective.hash_to_curve(msgs).xy, engine.hash_to_g1(msgs)[0])
    with pytest.raises(ValueError):
        api.XMDExpander("sha512", b"x")
