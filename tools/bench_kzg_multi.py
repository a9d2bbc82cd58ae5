"""Timing of the folded KZG openings -- sylow_hip_fr_lincomb_batch and sylow_hip_kzg_open_multi_batch -- against what a caller writes without
them, at four shapes (polynomials in groups, len):  8 in one group at 2^20;  32 in two groups of 16 at 2^20;  28 in groups of 24 and 4 at
2^16;  512 in 64 groups of 8 at 2^12.
  (a) fr_lincomb_batch against the fold by Horner's rule over the library's element-wise calls, F <- F gamma + f_j: sylow_hip_fr_mul_batch
      against gamma replicated to [4][len] and sylow_hip_fr_add_batch, two launches per polynomial;
  (b) kzg_open_multi_batch against sylow_hip_kzg_open_batch over all m polynomials (z_g spread to them), which is m proofs where the
      protocol wants G.
Two conditions per shape: each new call is no slower than its composition by more than the spread of this same alternating run, and the two
sides agree bit for bit -- (a) word for word, (b) through sum_j gamma^i pi_j formed with sylow_hip_g1_scalar_mul_batch and
sylow_hip_g1_sum_batch.  Recorded beside them: the ratios, the GB/s of the linear combination against the 32 (m + G) len bytes it must move,
and the device's clocks.  Coefficients are random canonical words (the element-wise calls are compared on values both sides take alike), the
SRS is tau^k G1gen through sylow_hip_g1_generator_mul_batch.  Device events around each call, warm-up calls first; the candidates ALTERNATE
inside every repetition in one process; medians with minimum and maximum.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_kzg_multi.py [--shapes 8@20,16+16@20,24+4@16,64x8@12] [--warmup 1] [--reps 5] [--out profiles/kzg_multi/bench_kzg_multi.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_groth16 import R  # noqa: E402
from bench_kzg_prove import srs_points  # noqa: E402
from bench_msm import Timer  # noqa: E402


def parse_shape(text):
    """'16+16@20' -> ([16, 16], 20); '64x8@12' -> 64 groups of 8"""
    groups, lg = text.split("@")
    sizes = []
    for part in groups.split("+"):
        if "x" in part:
            count, size = part.split("x")
            sizes += [int(size)] * int(count)
        else:
            sizes.append(int(part))
    return sizes, int(lg)


def canonical_words(rng, shape):
    """random words below 2^253 < r in the last axis of 4"""
    a = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64, endpoint=False)
    a[..., 3] &= np.uint64((1 << 61) - 1)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8@20,16+16@20,24+4@16,64x8@12")
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
    shapes = [parse_shape(s) for s in args.shapes.split(",")]
    srs = srs_points(eng, 1 << max(lg for _, lg in shapes), 0x2F1E0D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978 % R)
    for sizes, lg in shapes:
        n, m, G = 1 << lg, sum(sizes), len(sizes)
        gs = np.cumsum([0] + sizes).astype(np.uint64)
        rng = np.random.default_rng(m + lg)
        dc = eng.to_device(np.ascontiguousarray(canonical_words(rng, (m, n, 4)).transpose(0, 2, 1)))        # [m][4][len]
        z, gamma = canonical_words(rng, (G, 4)), canonical_words(rng, (G, 4))
        dz, dg = eng.to_device_soa(z, 4), eng.to_device_soa(gamma, 4)
        group_of = np.repeat(np.arange(G), sizes)
        dzs = eng.to_device_soa(z[group_of], 4)                                                              # z_g spread to its polynomials
        grep = [eng.to_device(np.ascontiguousarray(np.repeat(gamma[g][:, None], n, axis=1))) for g in range(G)]      # gamma_g as [4][len]
        ds = eng.to_device_soa(srs[:n], 8)
        dpow, df, dh, dt = eng.empty((4, m)), eng.empty((G, 4, n)), eng.empty((G, 4, n)), eng.empty((4, n))
        dy, dpi, dpii = eng.empty((4, m)), eng.empty((8, G)), eng.empty((G,), np.uint8)
        dy1, dpi1, dpii1 = eng.empty((4, m)), eng.empty((8, m)), eng.empty((m,), np.uint8)
        eng._call("sylow_hip_fr_group_powers_batch", dg.ptr, gs.ctypes.data, G, m, dpow.ptr)
        row_bytes = 32 * n

        def lincomb():
            eng._call("sylow_hip_fr_lincomb_batch", dc.ptr, n, m, dpow.ptr, gs.ctypes.data, G, df.ptr)

        def horner():
            for g in range(G):
                j0, j1 = int(gs[g]), int(gs[g + 1])
                acc = dh.ptr + g * row_bytes
                src = dc.ptr + (j1 - 1) * row_bytes                       # the last polynomial enters as it lies: no copy
                for j in range(j1 - 2, j0 - 1, -1):
                    eng._call("sylow_hip_fr_mul_batch", src, grep[g].ptr, dt.ptr, n)
                    eng._call("sylow_hip_fr_add_batch", dt.ptr, dc.ptr + j * row_bytes, acc, n)
                    src = acc

        def open_multi():
            eng._call("sylow_hip_kzg_open_multi_batch", ds.ptr, dc.ptr, n, m, gs.ctypes.data, G, dz.ptr, dg.ptr, dy.ptr, dpi.ptr, dpii.ptr)

        def open_each():
            eng._call("sylow_hip_kzg_open_batch", ds.ptr, dc.ptr, n, m, dzs.ptr, dy1.ptr, dpi1.ptr, dpii1.ptr)

        fns = (("lincomb", lincomb), ("horner", horner), ("open_multi", open_multi), ("open_each", open_each))
        for _ in range(args.warmup):
            for _, fn in fns:
                fn()
        eng.sync()
        res = {name: [] for name, _ in fns}
        for _ in range(args.reps):                                       # the candidates alternate inside every repetition
            for name, fn in fns:
                res[name].append(timer.time_ms(fn))
        row = {"groups": sizes if len(set(sizes)) > 1 or G <= 2 else f"{G} x {sizes[0]}", "m": m, "G": G, "len": n}
        for name, v in res.items():
            v = sorted(v)
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_ms_min"], row[name + "_ms_max"] = round(v[0], 4), round(v[-1], 4)
        for new, old in (("lincomb", "horner"), ("open_multi", "open_each")):
            spread = max(row[new + "_ms_max"] - row[new + "_ms_min"], row[old + "_ms_max"] - row[old + "_ms_min"])
            row[f"{old}_over_{new}"] = round(row[old + "_ms"] / row[new + "_ms"], 3)
            row[f"{new}_spread_ms"] = round(spread, 4)
            row[f"{new}_no_slower"] = bool(row[new + "_ms"] <= row[old + "_ms"] + spread)
        row["lincomb_gb_per_s"] = round(32 * (m + G) * n / row["lincomb_ms"] / 1e6, 1)
        # (a) word for word; a group of one is the polynomial itself (canonical words), which Horner's loop never touches
        f, h = df.download(), dh.download()
        for g in range(G):
            if sizes[g] == 1:
                h[g] = dc.download()[int(gs[g])]
        row["lincomb_same_words"] = bool(np.array_equal(f, h))
        # (b) the G proofs against sum_j gamma^i pi_j of the m proofs, and the values
        pw, pi1, pii1 = eng.from_device_soa(dpow), eng.from_device_soa(dpi1), dpii1.download()
        same = np.array_equal(dy.download(), dy1.download())
        pi, pii = eng.from_device_soa(dpi), dpii.download()
        for g in range(G):
            j0, j1 = int(gs[g]), int(gs[g + 1])
            xy, inf = eng.g1_scalar_mul(pi1[j0:j1], pw[j0:j1], pii1[j0:j1])
            sxy, sinf = eng.g1_sum(xy, inf)
            same = same and np.array_equal(sxy[0], pi[g]) and int(sinf[0]) == int(pii[g])
        row["open_same_points"] = bool(same)
        out["rows"].append(row)
        for d in [dc, dz, dg, dzs, ds, dpow, df, dh, dt, dy, dpi, dpii, dy1, dpi1, dpii1] + grep:
            d.free()
    out["all_no_slower"] = all(r["lincomb_no_slower"] and r["open_multi_no_slower"] for r in out["rows"])
    out["all_same"] = all(r["lincomb_same_words"] and r["open_same_points"] for r in out["rows"])
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
