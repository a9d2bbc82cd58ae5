"""Timing of batched Poseidon and its Merkle trees (poseidon.hip, include/sylow_poseidon.h) on device-resident arrays.
  (H)  sylow_poseidon_hash_batch_tuned at t = 3 and t = 5, on the narrow and on the wide route, n = 2^6 .. 2^22: hashes per second, and the
       CROSSOVER: the largest n at which the wide route is still no slower than the narrow one -- the default wide_max of the width's class
       (poseidon_plan.hpp: WIDE_MAX_*).
  (T)  sylow_poseidon_merkle_build_batch_tuned: one tree of 2^20 leaves and 4096 trees of 2^8 leaves, with the default wide_max and with
       wide_max = 0 (every level narrow).
  (P)  sylow_poseidon_merkle_verify_batch: q = 2^10 and 2^16 paths of depth 20 and 28 (28 is the deepest tree the header accepts).
The inputs are random words; the first hashes of every shape are checked against tests/poseidon_model.py before anything is timed.  Device
events around each call, warm-up calls first; the candidates ALTERNATE inside every repetition in one process, the median of --reps is
reported with its minimum and maximum.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_poseidon.py [--max-log 22] [--warmup 2] [--reps 7] [--out profiles/poseidon/bench_poseidon.json]
    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES -d DIR -- python tools/bench_poseidon.py --only-hash 3,0,20      (t, route, log2 n: counters alone)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_kzg_evals import measure  # noqa: E402
from bench_msm import Timer, words_to_ints  # noqa: E402

NARROW, WIDE = 0, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-log", type=int, default=6)
    ap.add_argument("--max-log", type=int, default=22)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-hash", default=None, help="t,route,log2 n: run that hash call warmup + reps times and time nothing (for a counter run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import poseidon_model as P
    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    rng = np.random.default_rng(20261021)
    tables = {t: eng.poseidon_table(t) for t in (3, 5)}
    top = 1 << (int(args.only_hash.split(",")[2]) if args.only_hash else max(args.max_log, 20))
    words = rng.integers(0, 1 << 64, size=4 * 4 * top, dtype=np.uint64, endpoint=False)        # the largest input: k = 4 inputs of 2^max_log items
    din, dout = eng.to_device(words), eng.empty((4, top))

    def hash_call(t, route, n):
        return lambda: eng._call("sylow_poseidon_hash_batch_tuned", tables[t].ptr, t - 1, din.ptr, None, n, route, -1, dout.ptr)

    if args.only_hash:
        t, route, lg = (int(x) for x in args.only_hash.split(","))
        fn = hash_call(t, route, 1 << lg)
        for _ in range(args.warmup + args.reps):
            fn()
        eng.sync()
        return

    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "hash": {}, "trees": [], "paths": []}
    # ---- (H) ------------------------------------------------------------------------------------------------------------------------------
    for t in (3, 5):
        rows = []
        for lg in range(args.min_log, args.max_log + 1):
            n = 1 << lg
            got = []
            for route in (NARROW, WIDE):
                hash_call(t, route, n)()
                got.append(dout.download().reshape(-1)[:4 * n].reshape(4, n).copy())         # out is [4][n], whatever the buffer holds beyond
            assert np.array_equal(got[0], got[1]), (t, n, "the routes give the same words")
            ins = words[:4 * (t - 1) * n].reshape(t - 1, 4, n)
            for j in range(min(n, 2)):
                assert words_to_ints(got[0][:, j][None])[0] == P.hash(words_to_ints(np.ascontiguousarray(ins[:, :, j]))), (t, n, j)
            row = {"n": n}
            row.update(measure(timer, eng, [("narrow", hash_call(t, NARROW, n)), ("wide", hash_call(t, WIDE, n))], args.warmup, args.reps))
            row["narrow_mhash_s"] = round(n / row["narrow_ms"] / 1e3, 3)
            row["wide_mhash_s"] = round(n / row["wide_ms"] / 1e3, 3)
            row["wide_over_narrow"] = round(row["wide_ms"] / row["narrow_ms"], 3)
            rows.append(row)
        no_slower = [r["n"] for r in rows if r["wide_ms"] <= r["narrow_ms"]]
        first_loss = next((r["n"] for r in rows if r["wide_ms"] > r["narrow_ms"]), None)
        out["hash"]["t%d" % t] = {"rows": rows, "wide_no_slower_at": no_slower, "narrow_first_faster_at": first_loss,
                                  "crossover_wide_max": max([n for n in no_slower if first_loss is None or n < first_loss], default=0)}
    # ---- (T) ------------------------------------------------------------------------------------------------------------------------------
    for depth, m in ((20, 1), (8, 4096)):
        n = 1 << depth
        dnodes, droot = eng.empty((m, 4, n - 1)), eng.empty((4, m))

        def build(wide_max):
            return lambda: eng._call("sylow_poseidon_merkle_build_batch_tuned", tables[3].ptr, din.ptr, depth, m, wide_max, -1, dnodes.ptr, droot.ptr)

        build(-1)()
        a = dnodes.download().copy()
        build(0)()
        assert np.array_equal(a, dnodes.download()), "the same nodes with every level narrow"
        leaves0 = words_to_ints(np.ascontiguousarray(words[:4 * n].reshape(4, n)[:, :2].T))
        assert words_to_ints(a[0, :, 0][None])[0] == P.hash(leaves0), "node 0 of tree 0 against the model"
        row = {"depth": depth, "trees": m, "leaves": n * m}
        row.update(measure(timer, eng, [("default", build(-1)), ("all_narrow", build(0)), ("all_wide", build(1 << 40))], args.warmup, args.reps))
        row["default_over_all_narrow"] = round(row["default_ms"] / row["all_narrow_ms"], 4)
        row["mhash_s_default"] = round((n - 1) * m / row["default_ms"] / 1e3, 3)
        out["trees"].append(row)
        dnodes.free()
        droot.free()
    # ---- (P) ------------------------------------------------------------------------------------------------------------------------------
    for depth in (20, 28):
        for lq in (10, 16):
            q = 1 << lq
            index = eng.to_device(rng.integers(0, 1 << depth, size=q, dtype=np.uint64))
            dok, dst = eng.empty((q,), np.uint8), eng.empty((q,), np.uint8)

            def verify(route):
                return lambda: eng._call("sylow_poseidon_merkle_verify_batch_tuned", tables[3].ptr, dout.ptr, index.ptr, din.ptr, depth, q, dout.ptr, q, route, -1,
                                         dok.ptr, dst.ptr)

            row = {"depth": depth, "q": q}
            row.update(measure(timer, eng, [("default", verify(-1)), ("narrow", verify(NARROW)), ("wide", verify(WIDE))], args.warmup, args.reps))
            row["us_per_path_default"] = round(row["default_ms"] * 1e3 / q, 4)
            row["mhash_s_default"] = round(q * depth / row["default_ms"] / 1e3, 3)
            out["paths"].append(row)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
