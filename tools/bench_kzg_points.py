"""Timing of the several-point KZG opening -- sylow_hip_kzg_quotient_points_batch and sylow_hip_kzg_open_points_batch -- against what a caller
writes without them, at five shapes (m polynomials, len, k points):  1 x 2^20 at 2, 4 and 16 points;  64 x 2^14 at 4;  4096 x 2^8 at 4.
  (a) kzg_quotient_points_batch against its composition: the coefficients replicated k times on the device (NOT timed; k times the memory),
      then sylow_hip_kzg_points_weights_batch, sylow_hip_kzg_quotient_batch over the m k rows and sylow_hip_fr_lincomb_batch under the
      weights -- three calls and an [m k][len] intermediate where the new call has none;
  (b) kzg_open_points_batch against k calls of sylow_hip_kzg_open_batch, one per point: k proofs where the protocol wants one.
Two conditions per shape: each new call is no slower than its composition by more than the spread of this same alternating run, and the two
sides agree bit for bit -- (a) q and y word for word, (b) y word for word and pi against sum_i a_i pi_i formed with
sylow_hip_g1_lincomb_batch.  The composition cannot serve as a fallback (it needs k times the memory), so a shape that misses a condition is
reported, not routed away.  Coefficients and points are random canonical words, the SRS is tau^e G1gen through
sylow_hip_g1_generator_mul_batch.  Device events around each call, warm-up calls first; the candidates ALTERNATE inside every repetition in
one process; medians with minimum and maximum.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_kzg_points.py [--shapes 1x20x2,1x20x4,1x20x16,64x14x4,4096x8x4] [--warmup 1] [--reps 5] [--out profiles/kzg_points/bench_kzg_points.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_groth16 import R  # noqa: E402
from bench_kzg_multi import canonical_words  # noqa: E402
from bench_kzg_prove import srs_points  # noqa: E402
from bench_msm import Timer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x20x2,1x20x4,1x20x16,64x14x4,4096x8x4")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    props = torch.cuda.get_device_properties(0)
    out = {"device": "cuda:0", "name": props.name, "clock_rate_khz": getattr(props, "clock_rate", None), "constant_rate_khz": eng.wall_clock_khz(),
           "warmup": args.warmup, "reps": args.reps, "rows": []}
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    srs = srs_points(eng, 1 << max(lg for _, lg, _ in shapes), 0x2F1E0D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978 % R)
    for m, lg, k in shapes:
        n, mk = 1 << lg, m * k
        rng = np.random.default_rng(m + lg + k)
        coeffs = np.ascontiguousarray(canonical_words(rng, (m, n, 4)).transpose(0, 2, 1))                   # [m][4][len]
        z = canonical_words(rng, (m, k, 4))
        dc, dz, ds = eng.to_device(coeffs), eng.to_device_soa(z.reshape(mk, 4), 4), eng.to_device_soa(srs[:n], 8)
        drep = eng.to_device(np.repeat(coeffs, k, axis=0))                                                  # [m k][4][len]: the composition's input
        dzi = [eng.to_device_soa(np.ascontiguousarray(z[:, i]), 4) for i in range(k)]                       # point i of every polynomial, [4][m]
        gs = (np.arange(m + 1) * k).astype(np.uint64)
        dq, dy, dpi, dpii = eng.empty((m, 4, n)), eng.empty((4, mk)), eng.empty((8, m)), eng.empty((m,), np.uint8)
        dqi, dyi, da, dq2 = eng.empty((mk, 4, n)), eng.empty((4, mk)), eng.empty((4, mk)), eng.empty((m, 4, n))
        dy1, dpi1, dpii1 = [eng.empty((4, m)) for _ in range(k)], [eng.empty((8, m)) for _ in range(k)], [eng.empty((m,), np.uint8) for _ in range(k)]
        dyo = eng.empty((4, mk))

        def quotient_points():
            eng._call("sylow_hip_kzg_quotient_points_batch", dc.ptr, n, m, dz.ptr, k, dq.ptr, dy.ptr)

        def composition():
            eng._call("sylow_hip_kzg_points_weights_batch", dz.ptr, k, m, da.ptr, None)
            eng._call("sylow_hip_kzg_quotient_batch", drep.ptr, n, mk, dz.ptr, dqi.ptr, dyi.ptr)
            eng._call("sylow_hip_fr_lincomb_batch", dqi.ptr, n, mk, da.ptr, gs.ctypes.data, m, dq2.ptr)

        def open_points():
            eng._call("sylow_hip_kzg_open_points_batch", ds.ptr, dc.ptr, n, m, dz.ptr, k, dyo.ptr, dpi.ptr, dpii.ptr)

        def open_each():
            for i in range(k):
                eng._call("sylow_hip_kzg_open_batch", ds.ptr, dc.ptr, n, m, dzi[i].ptr, dy1[i].ptr, dpi1[i].ptr, dpii1[i].ptr)

        fns = (("quotient_points", quotient_points), ("composition", composition), ("open_points", open_points), ("open_each", open_each))
        for _ in range(args.warmup):
            for _, fn in fns:
                fn()
        eng.sync()
        res = {name: [] for name, _ in fns}
        for _ in range(args.reps):                                       # the candidates alternate inside every repetition
            for name, fn in fns:
                res[name].append(timer.time_ms(fn))
        row = {"m": m, "len": n, "k": k, "replicated_mb": round(32 * mk * n / 2**20, 1)}
        for name, v in res.items():
            v = sorted(v)
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_ms_min"], row[name + "_ms_max"] = round(v[0], 4), round(v[-1], 4)
        for new, old in (("quotient_points", "composition"), ("open_points", "open_each")):
            spread = max(row[new + "_ms_max"] - row[new + "_ms_min"], row[old + "_ms_max"] - row[old + "_ms_min"])
            row[f"{old}_over_{new}"] = round(row[old + "_ms"] / row[new + "_ms"], 3)
            row[f"{new}_spread_ms"] = round(spread, 4)
            row[f"{new}_no_slower"] = bool(row[new + "_ms"] <= row[old + "_ms"] + spread)
        # (a) word for word
        row["quotient_same_words"] = bool(np.array_equal(dq.download(), dq2.download()) and np.array_equal(dy.download(), dyi.download()))
        # (b) the values word for word, and the one proof against sum_i a_i pi_i of the k proofs (term i of job j at i m + j)
        y_each = np.stack([eng.from_device_soa(d) for d in dy1], axis=1).reshape(mk, 4)
        same = np.array_equal(eng.from_device_soa(dyo), y_each)
        a = eng.from_device_soa(da).reshape(m, k, 4)
        terms = np.concatenate([eng.from_device_soa(d) for d in dpi1]), np.concatenate([d.download() for d in dpii1])
        sxy, sinf = eng.g1_lincomb(terms[0], np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(mk, 4), m, k, terms[1])
        row["open_same_points"] = bool(same and np.array_equal(sxy, eng.from_device_soa(dpi)) and np.array_equal(sinf, dpii.download()))
        out["rows"].append(row)
        for d in [dc, dz, ds, drep, dq, dy, dpi, dpii, dqi, dyi, da, dq2, dyo] + dzi + dy1 + dpi1 + dpii1:
            d.free()
    out["all_no_slower"] = all(r["quotient_points_no_slower"] and r["open_points_no_slower"] for r in out["rows"])
    out["all_same"] = all(r["quotient_same_words"] and r["open_same_points"] for r in out["rows"])
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
