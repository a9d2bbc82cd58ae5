"""Timing of the KZG prover's calls -- sylow_hip_kzg_quotient_batch, sylow_hip_kzg_commit_batch, sylow_hip_kzg_open_batch -- at
(m, len) = (1, 2^20), (64, 2^14), (4096, 2^8) (or --shapes), beside what they are measured against:
  (a) the commitment against what a host could do before it: m calls of sylow_hip_g1_msm, one per polynomial (the ONE condition of
      DESIGN.md §4.8: commit_batch must be no slower, within the spread of this same alternating run);
  (b) the quotient beside its multi-scalar multiplication (the commitment of the same shape) and beside sylow_hip_fr_mul_batch over the
      same number of elements -- recorded, not gated.
The SRS is tau^k G1gen through sylow_hip_g1_generator_mul_batch, coefficients and points z are random 256-bit words.  Device events around
each call, warm-up calls first; the candidates ALTERNATE inside every repetition in one process, the median of --reps is reported with its
minimum and maximum.  Every row checks that the two commitments agree bit for bit.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_kzg_prove.py [--shapes 1x20,64x14,4096x8] [--warmup 1] [--reps 5] [--out profiles/kzg_prove/bench_kzg_prove.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_groth16 import R  # noqa: E402
from bench_msm import Timer  # noqa: E402


def srs_points(eng, n, tau):
    """tau^k G1gen, k < n, as affine words [n, 8]"""
    buf, t = bytearray(), 1
    for _ in range(n):
        buf += t.to_bytes(32, "little")
        t = t * tau % R
    xy, inf = eng.g1_generator_mul(np.frombuffer(bytes(buf), dtype=np.uint64).reshape(n, 4))
    assert not inf.any()
    return xy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x20,64x14,4096x8")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "rows": []}
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    srs = srs_points(eng, 1 << max(lg for _, lg in shapes), 0x2F1E0D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978 % R)
    for m, lg in shapes:
        n = 1 << lg
        rng = np.random.default_rng(m + lg)
        dc = eng.to_device(rng.integers(0, 1 << 64, size=(m, 4, n), dtype=np.uint64, endpoint=False))      # [m][4][len], any words
        dz = eng.to_device_soa(rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64, endpoint=False), 4)
        ds = eng.to_device_soa(srs[:n], 8)
        dq, dy = eng.empty((m, 4, n)), eng.empty((4, m))
        pt = lambda: (eng.empty((8, m)), eng.empty((m,), np.uint8))
        (c, ci), (pi, pii) = pt(), pt()
        each, eachi = eng.empty((m, 8)), eng.empty((m,), np.uint8)       # m outputs of [8][1]
        da = eng.empty((4, m * n))                                        # fr_mul_batch over the same number of elements

        def quotient():
            eng._call("sylow_hip_kzg_quotient_batch", dc.ptr, n, m, dz.ptr, dq.ptr, dy.ptr)

        def commit():
            eng._call("sylow_hip_kzg_commit_batch", ds.ptr, dc.ptr, n, m, c.ptr, ci.ptr)

        def msm_each():
            for j in range(m):
                eng._call("sylow_hip_g1_msm", ds.ptr, None, dc.ptr + 32 * n * j, n, each.ptr + 64 * j, eachi.ptr + j)

        def open_():
            eng._call("sylow_hip_kzg_open_batch", ds.ptr, dc.ptr, n, m, dz.ptr, dy.ptr, pi.ptr, pii.ptr)

        def fr_mul():
            eng._call("sylow_hip_fr_mul_batch", dc.ptr, dc.ptr, da.ptr, m * n)

        fns = (("quotient", quotient), ("commit", commit), ("msm_each", msm_each), ("open", open_), ("fr_mul", fr_mul))
        for _ in range(args.warmup):
            for _, fn in fns:
                fn()
        eng.sync()
        res = {name: [] for name, _ in fns}
        for _ in range(args.reps):                                       # the candidates alternate inside every repetition
            for name, fn in fns:
                res[name].append(timer.time_ms(fn))
        row = {"m": m, "len": n}
        for name, v in res.items():
            v = sorted(v)
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_ms_min"], row[name + "_ms_max"] = round(v[0], 4), round(v[-1], 4)
        spread = max(row["commit_ms_max"] - row["commit_ms_min"], row["msm_each_ms_max"] - row["msm_each_ms_min"])
        row["commit_vs_msm_each"] = round(row["msm_each_ms"] / row["commit_ms"], 3)
        row["spread_ms"] = round(spread, 4)
        row["commit_no_slower"] = bool(row["commit_ms"] <= row["msm_each_ms"] + spread)
        row["quotient_vs_its_msm"] = round(row["quotient_ms"] / row["commit_ms"], 4)
        row["quotient_vs_fr_mul"] = round(row["quotient_ms"] / row["fr_mul_ms"], 2)
        row["coefficients_per_s"] = {k: round(m * n / row[k + "_ms"] * 1e3) for k in ("quotient", "commit", "open")}
        # sylow_hip_g1_msm reduces a scalar word >= p like Fp::new first, the KZG rule takes it mod r: equal only on words below p, so the
        # comparison runs on the quotients (canonical)
        eng._call("sylow_hip_kzg_commit_batch", ds.ptr, dq.ptr, n, m, c.ptr, ci.ptr)
        for j in range(m):
            eng._call("sylow_hip_g1_msm", ds.ptr, None, dq.ptr + 32 * n * j, n, each.ptr + 64 * j, eachi.ptr + j)
        row["same_points"] = bool(np.array_equal(c.download().T, each.download()) and np.array_equal(ci.download(), eachi.download())
                                  and np.array_equal(pi.download(), c.download()))
        out["rows"].append(row)
        for d in (dc, dz, ds, dq, dy, c, ci, pi, pii, each, eachi, da):
            d.free()
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
