"""Timing of sylow_hip_g1_msm against the composed route (sylow_hip_g1_scalar_mul_batch + sylow_hip_g1_sum_batch) on the same device
buffers, at n = 2^12, 2^16 ... 2^20 (or --sizes), random full-width scalars.  Every row times the default route (`msm_ms`), the bucket route
forced (`bucket_ms`, sylow_hip_g1_msm_tuned with min_n = 0) and the composed route; the crossover is read off the bucket_ms / composed_ms
columns.  At 2^20 two hot-bucket scalar sets follow: every scalar equal (one bucket per window takes every point) and scalars from {0, 1}
(bit commitments: half the points in ONE bucket of window 0).  Device events around each call, warm-up calls first, the median of --reps.
Every row checks that the routes give the same point; 2^20 also checks it against ((sum_i (k_i mod p) a_i) mod r) G from one big-int sum
and one oracle scalar multiplication (P_i = a_i G).  Prints ONE JSON object.

    python tools/bench_msm.py [--sizes 12,16,17,18,19,20] [--warmup 2] [--reps 7]

--g2 times sylow_hip_g2_msm the same way (default --sizes 10..20): the bucket route forced (`bucket_ms`, min_n = 0), the composed route
(`composed_ms`: sylow_hip_g2_scalar_mul_batch + sylow_hip_g2_sum_batch) and a third column, `subgroup_ms`: sylow_hip_g2_scalar_mul_subgroup_batch
+ the sum, the fastest way a caller with r-torsion points has without the bucket route (the points here are generator multiples, so all three
give the same point, and every row checks that).  --sweep 16,20 adds, for those sizes, the bucket route at every window width 4..16.

    python tools/bench_msm.py --g2 [--sizes 10,11,...,20] [--sweep 16,20] [--warmup 1] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import msm_model as M  # noqa: E402

P, R = M.P, M.R


class Timer:
    """a pair of device events around a call on the engine's stream (torch's HIP runtime is the one the process has loaded)"""

    def __init__(self, stream):
        import torch
        self.torch = torch
        self.stream = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()

    def time_ms(self, fn):
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        fn()
        b.record(self.stream)
        b.synchronize()
        return a.elapsed_time(b)


def words_to_ints(w):
    w = w.astype(object)
    return list(w[:, 0] + (w[:, 1] << 64) + (w[:, 2] << 128) + (w[:, 3] << 192))


def main_g2(args):
    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    rng = np.random.default_rng(20261017)
    sizes = [int(x) for x in (args.sizes or ",".join(map(str, range(10, 21)))).split(",")]
    sweep = [int(x) for x in args.sweep.split(",")] if args.sweep else []
    out = {"device": "cuda:0", "group": "G2", "warmup": args.warmup, "reps": args.reps, "default_min_n": M.G2_DEFAULT_MIN, "sizes": {}, "window_sweep": {}}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        eng.sync()
        v = sorted(timer.time_ms(fn) for _ in range(args.reps))
        return round(v[len(v) // 2], 4), round(v[0], 4)

    for lg in sorted(set(sizes) | set(sweep)):
        n = 1 << lg
        aw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        aw[:, 3] &= np.uint64((1 << 60) - 1)
        kw = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        xy, _ = eng.g2_generator_mul(aw)
        dp, dk = eng.to_device_soa(xy, 16), eng.to_device_soa(kw, 4)
        outs = {k: (eng.empty((16, 1)), eng.empty((1,), np.uint8)) for k in ("msm", "bucket", "composed", "subgroup", "sweep")}
        t, ti = eng.empty((16, n)), eng.empty((n,), np.uint8)

        def msm():
            eng._call("sylow_hip_g2_msm", dp.ptr, None, dk.ptr, n, outs["msm"][0].ptr, outs["msm"][1].ptr)

        def bucket(c=-1, key="bucket"):
            eng._call("sylow_hip_g2_msm_tuned", dp.ptr, None, dk.ptr, n, c, 0, outs[key][0].ptr, outs[key][1].ptr)

        def composed(sym="sylow_hip_g2_scalar_mul_batch", key="composed"):
            eng._call(sym, dp.ptr, None, dk.ptr, t.ptr, ti.ptr, n)
            eng._call("sylow_hip_g2_sum_batch", t.ptr, ti.ptr, n, outs[key][0].ptr, outs[key][1].ptr)

        def point(key):
            return outs[key][0].download().tobytes() + outs[key][1].download().tobytes()

        if lg in sizes:
            cols = {"msm": timed(msm), "bucket": timed(bucket), "composed": timed(composed),
                    "subgroup": timed(lambda: composed("sylow_hip_g2_scalar_mul_subgroup_batch", "subgroup"))}
            c = M.g2_default_window(n)
            row = {"n": n, "route": "bucket" if n >= M.G2_DEFAULT_MIN else "scalar mul per lane pair + sum"}
            for k, (med, lo) in cols.items():
                row[k + "_ms"], row[k + "_ms_min"] = med, lo
            row.update({"bucket_vs_composed": round(cols["composed"][0] / cols["bucket"][0], 3),
                        "bucket_vs_subgroup": round(cols["subgroup"][0] / cols["bucket"][0], 3),
                        "same_point": len({point(k) for k in ("msm", "bucket", "composed", "subgroup")}) == 1,
                        "c": c, "windows": M.windows(c), "chunks": -(-n // M.g2_plan(n, c)[0])})
            out["sizes"][str(n)] = row
            print(json.dumps(row), file=sys.stderr, flush=True)
        if lg in sweep:
            bucket()
            ref = point("bucket")
            sw = {}
            for c in range(M.C_MIN, M.C_MAX + 1):
                med, lo = timed(lambda: bucket(c, "sweep"))
                sw[str(c)] = {"bucket_ms": med, "bucket_ms_min": lo, "same_point": point("sweep") == ref}
            out["window_sweep"][str(n)] = {"default_c": M.g2_default_window(n), "by_c": sw}
            print(json.dumps({"n": n, "sweep": sw}), file=sys.stderr, flush=True)
        for d in [dp, dk, t, ti] + [x for pair in outs.values() for x in pair]:
            d.free()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--g2", action="store_true", help="time sylow_hip_g2_msm (three columns) instead of sylow_hip_g1_msm")
    ap.add_argument("--sweep", default="", help="with --g2: log2 sizes at which every window width 4..16 is timed on the bucket route")
    args = ap.parse_args()
    if args.g2:
        return main_g2(args)
    args.sizes = args.sizes or "12,16,17,18,19,20"

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    rng = np.random.default_rng(20261015)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "sizes": {}}
    cases = [(lg, "random") for lg in (int(x) for x in args.sizes.split(","))]
    if any(lg == 20 for lg, _ in cases):
        cases += [(20, "all_equal"), (20, "zero_one")]
    for lg, kind in cases:
        n = 1 << lg
        aw = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
        aw[:, 3] &= np.uint64((1 << 60) - 1)
        if kind == "random":
            kw = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        elif kind == "all_equal":
            kw = np.repeat(rng.integers(0, 1 << 64, size=(1, 4), dtype=np.uint64), n, 0)
        else:
            kw = np.zeros((n, 4), dtype=np.uint64)
            kw[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint64)
        xy, _ = eng.g1_generator_mul(aw)
        dp, dk = eng.to_device_soa(xy, 8), eng.to_device_soa(kw, 4)
        mo, moi = eng.empty((8, 1)), eng.empty((1,), np.uint8)
        qo, qoi = eng.empty((8, 1)), eng.empty((1,), np.uint8)
        t, ti = eng.empty((8, n)), eng.empty((n,), np.uint8)
        bo, boi = eng.empty((8, 1)), eng.empty((1,), np.uint8)

        def msm():
            eng._call("sylow_hip_g1_msm", dp.ptr, None, dk.ptr, n, mo.ptr, moi.ptr)

        def bucket():
            eng._call("sylow_hip_g1_msm_tuned", dp.ptr, None, dk.ptr, n, -1, 0, qo.ptr, qoi.ptr)

        def composed():
            eng._call("sylow_hip_g1_scalar_mul_batch", dp.ptr, None, dk.ptr, t.ptr, ti.ptr, n)
            eng._call("sylow_hip_g1_sum_batch", t.ptr, ti.ptr, n, bo.ptr, boi.ptr)

        res = {}
        for name, fn in (("msm", msm), ("bucket", bucket), ("composed", composed)):
            for _ in range(args.warmup):
                fn()
            eng.sync()
            res[name] = sorted(timer.time_ms(fn) for _ in range(args.reps))
        med = {k: round(v[len(v) // 2], 4) for k, v in res.items()}
        ref = (bo.download(), boi.download())
        same = all(bool(np.array_equal(a.download(), ref[0]) and np.array_equal(ai.download(), ref[1])) for a, ai in ((mo, moi), (qo, qoi)))
        c = M.default_window(n)
        row = {"n": n, "scalars": kind, "route": "bucket" if n >= M.DEFAULT_MIN else "per-lane scalar mul + sum",
               "msm_ms": med["msm"], "bucket_ms": med["bucket"], "composed_ms": med["composed"],
               "msm_ms_min": round(res["msm"][0], 4), "bucket_ms_min": round(res["bucket"][0], 4), "composed_ms_min": round(res["composed"][0], 4),
               "speedup": round(med["composed"] / med["msm"], 3), "bucket_speedup": round(med["composed"] / med["bucket"], 3), "same_point": same,
               "c": c, "windows": M.windows(c), "buckets_per_window": M.buckets(c), "top_window_bits": M.top_bits(c),
               "adds_per_point": M.additions_per_point(c), "chunks": -(-n // M.plan(n, c)[0])}
        if lg == 20:
            from oracle import coracle as C
            C.build()
            e = sum((k % P) * a for k, a in zip(words_to_ints(kw), words_to_ints(aw))) % R
            exy, einf = C.g1_to_affine(C.g1_scalar_mul(C.to_limbs([1, 2, 1]).reshape(1, 12), C.to_limbs([e])))
            row["oracle_check"] = bool(np.array_equal(eng.from_device_soa(mo).reshape(1, 8), exy.reshape(1, 8)) and moi.download()[0] == einf[0])
        out["sizes"][f"{n}" if kind == "random" else f"{n}_{kind}"] = row
        for d in (dp, dk, mo, moi, qo, qoi, t, ti, bo, boi):
            d.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
