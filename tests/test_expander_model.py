"""CPU side of the caller-chosen expanders: the byte-level model (tests/expander_model.py) reproduces the reference's twelve RFC 9380
literals (tests/golden/expander_kats.json, hasher.rs:345-388) and the oracle's Keccak routines; the library exports the six entry
points and refuses every whole-call error with SYLOW_HIP_E_ARG and a reason -- before it touches a device, so also without one."""
import json
import os
import random

import pytest

import expander_model as M
from oracle import pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "expander_kats.json")))["vectors"]
ENTRY_POINTS = ["sylow_hip_expand_message_batch", "sylow_hip_hash_to_field_expander_batch", "sylow_hip_hash_to_g1_expander_batch",
                "sylow_hip_bls_sign_expander_batch", "sylow_hip_bls_verify_expander_batch", "sylow_hip_bls_verify_hashed_batch"]


def test_fixture_is_the_twelve_literals():
    assert len(KATS) == 12
    assert sorted({(v["expander"], len(v["dst"])) for v in KATS}) == [("xmd_sha256", 38), ("xmd_sha256", 256), ("xof_shake128", 36), ("xof_shake128", 256)]
    assert all(v["len_in_bytes"] == 0x20 and v["k"] == 128 and len(v["expected"]) == 64 for v in KATS)


@pytest.mark.parametrize("v", KATS, ids=lambda v: f"{v['set']}-{len(v['msg'])}")
def test_model_reproduces_the_reference_literals(v):
    got = M.expand_message(v["expander_id"], v["msg"].encode(), v["dst"].encode(), v["len_in_bytes"], v["k"])
    assert got.hex() == v["expected"]


def test_model_keccak_path_equals_the_oracle():
    rng = random.Random(9380)
    for _ in range(60):
        msg = rng.randbytes(rng.randrange(0, 300))
        dst = rng.randbytes(rng.choice([1, 30, 101, 102, 103, 255, 256, 300]))
        length = rng.choice([1, 32, 33, 96, 255, 8160])
        assert M.expand_message(M.XMD_KECCAK256, msg, dst, length) == R.expand_message_xmd(msg, dst, length)
        assert M.expand_message(M.XMD_SHA256, msg, dst, length) == R.expand_message_xmd(msg, dst, length, "sha256")
        assert M.hash_to_field(M.XMD_KECCAK256, msg, dst) == R.hash_to_field(msg, dst)
    for msg in (b"", b"abc", bytes(200)):
        assert M.hash_to_curve(M.XMD_KECCAK256, msg) == R.hash_to_curve(msg)
        for e in (M.XMD_SHA256, M.XOF_SHAKE128):
            x, y = M.hash_to_curve_affine(e, msg, b"tag")
            assert R.g1_is_on_curve_affine(x, y)


def test_library_exports_the_entry_points():
    import sylow_amd
    from sylow_amd import _lib
    lib = sylow_amd.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


# (expander, security_bits, len_in_bytes) of every whole-call error, and a word of the reason sylow_hip_last_error() must name
WHOLE_CALL_ERRORS = [((3, 128, 32), b"unknown expander"), ((-1, 128, 32), b"unknown expander"), ((1, 128, 0), b"len_in_bytes == 0"),
                     ((2, 128, 0), b"len_in_bytes == 0"), ((2, 128, 65536), b"65535"), ((1, 128, 8161), b"> 255"), ((0, 128, 8161), b"> 255"),
                     ((1, 129, 32), b"security_bits > 256"), ((0, 129, 32), b"security_bits > 256"), ((1, 0, 32), b"security_bits < 1"),
                     ((2, -5, 32), b"security_bits < 1"), ((2, 1021, 32), b"/ 8) > 255")]


@pytest.mark.parametrize("args,reason", WHOLE_CALL_ERRORS, ids=lambda a: "-".join(map(str, a)) if isinstance(a, tuple) else None)
def test_whole_call_errors_are_refused_before_any_launch(args, reason):
    """No pointer of these calls is valid and n = 4: an implementation that launched anything would fault, one that checked the pointers
    first would not name the reason."""
    import sylow_amd
    lib = sylow_amd.load()
    e, k, length = args
    assert lib.sylow_hip_expand_message_batch(e, None, None, b"tag", 3, k, length, None, 4, None) == -2
    assert b"bad argument" in lib.sylow_hip_last_error() and reason in lib.sylow_hip_last_error(), lib.sylow_hip_last_error()
    if length == 32:                                   # the conditions that do not depend on len_in_bytes: every entry point with an expander
        for call in (lambda: lib.sylow_hip_hash_to_field_expander_batch(e, None, None, None, 0, k, None, 4, None),
                     lambda: lib.sylow_hip_hash_to_g1_expander_batch(e, None, None, None, 0, k, None, None, 4, None),
                     lambda: lib.sylow_hip_bls_sign_expander_batch(e, None, 0, k, None, None, None, None, None, 4, None),
                     lambda: lib.sylow_hip_bls_verify_expander_batch(e, None, 0, k, None, None, None, None, None, None, None, 4, None)):
            assert call() == -2
            assert reason in lib.sylow_hip_last_error(), lib.sylow_hip_last_error()


def test_lengths_at_the_limits_are_not_refused_for_their_length():
    """8160 = 255 * 32 bytes of XMD output and 65535 bytes of XOF output pass the whole-call check (the NULL pointers are what is refused)"""
    import sylow_amd
    lib = sylow_amd.load()
    for e, length in ((0, 8160), (1, 8160), (2, 8161), (2, 65535), (1, 1)):
        assert lib.sylow_hip_expand_message_batch(e, None, None, None, 0, 128, length, None, 4, None) == -2
        assert b"msgs && msg_offsets && out" in lib.sylow_hip_last_error()
    assert lib.sylow_hip_bls_verify_hashed_batch(None, None, None, None, None, None, None, 4, None) == -2
