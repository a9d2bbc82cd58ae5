"""Timing of the committee shape of sylow_hip_bls_aggregate_verify_batch -- m signers of ONE message, n = 1 and n_pk = m: one hash, one
segmented G2 sum and two Miller loops -- against the call that existed before it on the same signers (n = n_pk = m rows, the message
repeated, the individual signatures: m hashes and m Miller loops), at m = 2^10 .. 2^20 (or --sizes).  Keys are a_j G2gen, signatures
a_j H(msg); the committee call gets their sum (sylow_hip_g1_sum_batch, timed on its own as `sig_sum_ms`: a caller who holds individual
signatures pays it).  Device events around each call, warm-up calls first, the median of --reps.  Every row checks that the two calls give the
same 48 Gt words and is_one = 1.  The G2 sum has no entry point of its own; its kernels (k_g2_seg_fold) are read off a kernel trace of
`--only committee` (profiles/README.md).  Prints ONE JSON object.

    python tools/bench_committee.py [--sizes 10,11,...,20] [--warmup 2] [--reps 7] [--only committee|rows]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_msm import Timer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(x) for x in range(10, 21)))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=("committee", "rows"), default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    rng = np.random.default_rng(20261016)
    sizes = [int(x) for x in args.sizes.split(",")]
    top = 1 << max(sizes)
    msg = b"one message, many signers"
    sk = rng.integers(0, 1 << 63, size=(top, 4), dtype=np.uint64)
    sk[:, 3] &= np.uint64((1 << 60) - 1)
    pk, _ = eng.g2_generator_mul(sk)
    blob = np.frombuffer(msg * top, dtype=np.uint8)
    off = np.arange(top + 1, dtype=np.uint64) * np.uint64(len(msg))
    dblob, doff = eng.to_device(blob), eng.to_device(off)
    dsk = eng.to_device_soa(sk, 4)
    dall, dalli = eng.empty((8, top)), eng.empty((top,), np.uint8)
    eng._call("sylow_hip_bls_sign_batch", dsk.ptr, dblob.ptr, doff.ptr, dall.ptr, dalli.ptr, top)
    each = eng.from_device_soa(dall)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "sizes": {}}
    for lg in sizes:
        m = 1 << lg
        dpk, dsig = eng.to_device_soa(pk[:m], 16), eng.to_device_soa(each[:m], 8)
        dsum, dsumi = eng.empty((8, 1)), eng.empty((1,), np.uint8)
        gt_c, one_c = eng.empty((48, 1)), eng.empty((1,), np.uint8)
        gt_r, one_r = eng.empty((48, 1)), eng.empty((1,), np.uint8)

        def sig_sum():
            eng._call("sylow_hip_g1_sum_batch", dsig.ptr, None, m, dsum.ptr, dsumi.ptr)

        def committee():
            eng._call("sylow_hip_bls_aggregate_verify_batch", dpk.ptr, None, m, dblob.ptr, doff.ptr, dsum.ptr, dsumi.ptr, 1, None, gt_c.ptr, one_c.ptr)

        def rows():
            eng._call("sylow_hip_bls_aggregate_verify_batch", dpk.ptr, None, m, dblob.ptr, doff.ptr, dsig.ptr, None, m, None, gt_r.ptr, one_r.ptr)

        sig_sum()
        res = {}
        for name, fn in (("sig_sum", sig_sum), ("committee", committee), ("rows", rows)):
            if args.only and name not in ("sig_sum", args.only):
                continue
            for _ in range(args.warmup):
                fn()
            eng.sync()
            res[name] = sorted(timer.time_ms(fn) for _ in range(args.reps))
        row = {"signers": m}
        for k, v in res.items():
            row[k + "_ms"] = round(v[len(v) // 2], 4)
            row[k + "_ms_min"] = round(v[0], 4)
        if not args.only:
            row["speedup"] = round(row["rows_ms"] / row["committee_ms"], 2)
            row["same_gt"] = bool(np.array_equal(gt_c.download(), gt_r.download()))
            row["is_one"] = [int(one_c.download()[0]), int(one_r.download()[0])]
            row["committee_signers_per_s"] = round(m / row["committee_ms"] * 1e3)
            row["rows_signers_per_s"] = round(m / row["rows_ms"] * 1e3)
        out["sizes"][str(m)] = row
        for d in (dpk, dsig, dsum, dsumi, gt_c, one_c, gt_r, one_r):
            d.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
