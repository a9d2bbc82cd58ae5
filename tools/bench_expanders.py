"""Timing of hashing and verifying under a caller-chosen RFC 9380 expander against the fixed Keccak-256 suite, same process, same inputs,
calls interleaved round by round: hash-to-G1 of n 32-byte messages through sylow_hip_hash_to_g1_batch and through
sylow_hip_hash_to_g1_expander_batch for each expander id (tag = a 40-byte suite name; expander 0 is the existing route behind the new
entry point), sylow_hip_bls_verify_expander_batch (SHA-256) against sylow_hip_bls_verify_batch, and the n = 1 latency of both hash-to-G1
entry points (the existing one runs eight lanes per message there, the new expanders one lane).  Device events around each call, warm-up
calls first, the median and the minimum of --reps.  Prints ONE JSON object (kept as profiles/expanders/bench_expanders.json).

    python tools/bench_expanders.py [--log2n 20] [--verify-log2n 20] [--warmup 2] [--reps 7]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_msm import Timer  # noqa: E402

TAG = b"BLS_SIG_BN254G1_XMD:SHA-256_SVDW_RO_NUL_"
NAMES = {0: "xmd_keccak256", 1: "xmd_sha256", 2: "xof_shake128"}


def interleaved(timer, eng, fns, warmup, reps):
    """{name: sorted times}: every round runs each call once, in turn, so that drift of the clocks hits all of them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    eng.sync()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            res[k].append(timer.time_ms(fn))
    return {k: sorted(v) for k, v in res.items()}


def summary(res):
    return {k: {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--verify-log2n", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    rng = np.random.default_rng(9380)
    n = 1 << max(args.log2n, args.verify_log2n)
    blob = rng.integers(0, 256, size=n * 32, dtype=np.uint8)
    dm, doff = eng.to_device(blob), eng.to_device(np.arange(n + 1, dtype=np.uint64) * np.uint64(32))
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "message_bytes": 32, "tag_bytes": len(TAG)}

    def hash_calls(m, h, hi):
        fns = {"existing_hash_to_g1_batch": lambda: eng._call("sylow_hip_hash_to_g1_batch", dm.ptr, doff.ptr, TAG, len(TAG), h.ptr, hi.ptr, m)}
        for e, name in NAMES.items():
            fns["expander_" + name] = (lambda e=e: eng._call("sylow_hip_hash_to_g1_expander_batch", e, dm.ptr, doff.ptr, TAG, len(TAG), 128, h.ptr, hi.ptr, m))
        return fns

    m = 1 << args.log2n
    h, hi = eng.empty((8, m)), eng.empty((m,), np.uint8)
    out["hash_to_g1"] = {"n": m, **summary(interleaved(timer, eng, hash_calls(m, h, hi), args.warmup, args.reps))}
    out["hash_to_g1_single"] = {"n": 1, **summary(interleaved(timer, eng, hash_calls(1, h, hi), args.warmup, max(args.reps, 21)))}
    h.free(); hi.free()

    m = 1 << args.verify_log2n
    sk = rng.integers(0, 1 << 63, size=(m, 4), dtype=np.uint64)
    sk[:, 3] &= np.uint64((1 << 60) - 1)
    dsk = eng.to_device_soa(sk, 4)
    pk, pki = eng.empty((16, m)), eng.empty((m,), np.uint8)
    eng._call("sylow_hip_g2_generator_mul_batch", dsk.ptr, pk.ptr, pki.ptr, m)
    sig0, sig1, si = eng.empty((8, m)), eng.empty((8, m)), eng.empty((m,), np.uint8)
    eng._call("sylow_hip_bls_sign_batch", dsk.ptr, dm.ptr, doff.ptr, sig0.ptr, si.ptr, m)
    eng._call("sylow_hip_bls_sign_expander_batch", 1, TAG, len(TAG), 128, dsk.ptr, dm.ptr, doff.ptr, sig1.ptr, si.ptr, m)
    ok0, ok1 = eng.empty((m,), np.uint8), eng.empty((m,), np.uint8)
    fns = {"existing_bls_verify_batch": lambda: eng._call("sylow_hip_bls_verify_batch", pk.ptr, None, dm.ptr, doff.ptr, sig0.ptr, None, ok0.ptr, m),
           "verify_expander_xmd_sha256": lambda: eng._call("sylow_hip_bls_verify_expander_batch", 1, TAG, len(TAG), 128, pk.ptr, None, dm.ptr, doff.ptr,
                                                           sig1.ptr, None, ok1.ptr, m)}
    out["bls_verify"] = {"n": m, **summary(interleaved(timer, eng, fns, args.warmup, args.reps))}
    out["bls_verify"]["all_valid"] = [bool(ok0.download().all()), bool(ok1.download().all())]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
