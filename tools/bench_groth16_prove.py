"""Timing of the Groth16 prover -- sylow_hip_fr_spmv_batch, sylow_hip_groth16_quotient_batch, sylow_hip_groth16_prove_batch -- at
(m, log_n, n_vars) = (1, 20, 2^20), (8, 16, 2^16), (64, 12, 2^12) (or --shapes), three entries per row in each matrix.
  (a) the sparse product alone (one matrix, m vectors) on the default lanes per row and pinned to 1, 4 and 64, in entries/s and bytes/s
      beside the HBM peak (entries: 8 B column + 32 B value + 32 B gathered; rows: 8 B offset + 32 B out per vector);
  (b) the quotient beside THE SAME ARITHMETIC COMPOSED BY A CALLER from the public calls on device arrays: three sylow_hip_fr_ntt_batch
      inverses, three forwards with shift 5, then per array sylow_hip_fr_mul_batch, sylow_hip_fr_sub_batch and a product by an array of the
      constant, and one shifted inverse.  THE CONDITION: the library's call is no slower than that composition within the spread of the run;
  (c) each of the five multi-scalar multiplications of ONE witness; the whole proof of m witnesses; the share of each part in it.
The key's points are generator multiples (sylow_hip_g1_generator_mul_batch; one array serves every G1 query), values are random 256-bit
words.  Device events around each call, warm-up calls first; the candidates ALTERNATE inside every repetition in one process, the median of
--reps is reported with its minimum and maximum.  Every row checks that the quotient equals the composition word for word and that every
lane pin gives the default's words.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_groth16_prove.py [--shapes 1x20x20,8x16x16,64x12x12] [--warmup 1] [--reps 5] [--out profiles/groth16_prove/bench_groth16_prove.json]"""
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

HBM_PEAK = 8.0e12                                                       # bytes/s, MI355X
DENSITY = 3
ZINV = lambda lg: pow((pow(5, 1 << lg, R) - 1) % R, R - 2, R)


def limbs(v):
    return np.array([[(x >> (64 * k)) & ((1 << 64) - 1) for k in range(4)] for x in v], dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x20x20,8x16x16,64x12x12")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "entries_per_row": DENSITY, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": []}
    for m, lg, lv in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        n, nv, l = 1 << lg, 1 << lv, 1
        nnz, nl, nh = DENSITY * n, nv - l - 1, n - 1
        rng = np.random.default_rng(m + lg)
        u64 = lambda *shape: rng.integers(0, 1 << 64, size=shape, dtype=np.uint64, endpoint=False)
        # three matrices of n rows (the same arrays serve all three), 3 entries per row
        drp = eng.to_device(np.arange(n + 1, dtype=np.uint64) * DENSITY)
        dcol, dval = eng.to_device(rng.integers(0, nv, size=nnz, dtype=np.uint64)), eng.to_device(u64(4, nnz))
        dz, dr, ds = eng.to_device(u64(m, 4, nv)), eng.to_device(u64(4, m)), eng.to_device(u64(4, m))
        # the key: generator multiples
        npts = max(nv, n)
        dk, dk2 = eng.to_device(u64(4, npts)), eng.to_device(u64(4, nv))
        g1, g1i, g2, g2i = eng.empty((8, npts)), eng.empty((npts,), np.uint8), eng.empty((16, nv)), eng.empty((nv,), np.uint8)
        eng._call("sylow_hip_g1_generator_mul_batch", dk.ptr, g1.ptr, g1i.ptr, npts)
        eng._call("sylow_hip_g2_generator_mul_batch", dk2.ptr, g2.ptr, g2i.ptr, nv)
        first = lambda d, k: eng.to_device(np.ascontiguousarray(d.download()[:, :k])) if k != d.shape[1] else d     # the first k points, SoA of stride k
        q_nv, q_h, q_l = first(g1, nv), first(g1, nh), first(g1, nl)
        one1 = eng.to_device(np.ascontiguousarray(g1.download()[:, :1]))
        one2 = eng.to_device(np.ascontiguousarray(g2.download()[:, :1]))
        # canonical scalars for the stand-alone sums (a shorter sum reads them at its own stride: other words of the same array)
        dzc = eng.empty((4, nv))
        eng._call("sylow_hip_fr_add_batch", dz.ptr, dz.ptr, dzc.ptr, nv)
        dsp, dabc, dh, dh2 = eng.empty((m, 4, n)), eng.to_device(u64(3 * m, 4, n)), eng.empty((m, 4, n)), eng.empty((m, 4, n))
        da, db, dc = dabc.ptr, dabc.ptr + 32 * m * n, dabc.ptr + 64 * m * n
        t1, t2 = eng.empty((3 * m, 4, n)), eng.empty((3 * m, 4, n))
        dshift = eng.to_device(np.array([5, 0, 0, 0], dtype=np.uint64))
        dzi = eng.to_device(np.ascontiguousarray(np.repeat(limbs([ZINV(lg)]).T, n, axis=1)))      # the constant as an array [4][n]
        pt1, pt2 = (eng.empty((8, 1)), eng.empty((1,), np.uint8)), (eng.empty((16, 1)), eng.empty((1,), np.uint8))
        pa, pai, pb, pbi, pc, pci = eng.empty((8, m)), eng.empty((m,), np.uint8), eng.empty((16, m)), eng.empty((m,), np.uint8), eng.empty((8, m)), eng.empty((m,), np.uint8)

        def spmv(lanes=-1, dst=dsp):
            eng._call("sylow_hip_fr_spmv_batch_tuned", drp.ptr, dcol.ptr, dval.ptr, n, nnz, dz.ptr, nv, m, n, lanes, dst.ptr)

        def quotient():
            eng._call("sylow_hip_groth16_quotient_batch", da, db, dc, lg, m, dh.ptr)

        def composed():
            for k, src in enumerate((da, db, dc)):                                               # three inverses, three shifted forwards
                eng._call("sylow_hip_fr_ntt_batch", src, lg, m, 1, None, t1.ptr + 32 * m * n * k)
            for k in range(3):
                eng._call("sylow_hip_fr_ntt_batch", t1.ptr + 32 * m * n * k, lg, m, 0, dshift.ptr, t2.ptr + 32 * m * n * k)
            for j in range(m):                                                                   # fr_mul, fr_sub, the constant: an array at a time
                a, b, c, o = (t2.ptr + 32 * n * (k * m + j) for k in (0, 1, 2, 0))
                eng._call("sylow_hip_fr_mul_batch", a, b, o, n)
                eng._call("sylow_hip_fr_sub_batch", o, c, o, n)
                eng._call("sylow_hip_fr_mul_batch", o, dzi.ptr, o, n)
            eng._call("sylow_hip_fr_ntt_batch", t2.ptr, lg, m, 1, dshift.ptr, dh2.ptr)

        def prove():
            eng._call("sylow_hip_groth16_prove_batch", drp.ptr, dcol.ptr, dval.ptr, nnz, drp.ptr, dcol.ptr, dval.ptr, nnz, drp.ptr, dcol.ptr, dval.ptr, nnz, n, nv, l, lg,
                      one1.ptr, one1.ptr, one1.ptr, one2.ptr, one2.ptr, q_nv.ptr, None, q_nv.ptr, None, g2.ptr, None, q_h.ptr, None, q_l.ptr, None,
                      dz.ptr, dr.ptr, ds.ptr, m, pa.ptr, pai.ptr, pb.ptr, pbi.ptr, pc.ptr, pci.ptr)

        msm1 = lambda q, k: (lambda: eng._call("sylow_hip_g1_msm", q.ptr, None, dzc.ptr, k, pt1[0].ptr, pt1[1].ptr))
        fns = (("spmv", lambda: spmv()), ("spmv_lanes_1", lambda: spmv(0)), ("spmv_lanes_4", lambda: spmv(2)), ("spmv_lanes_64", lambda: spmv(6)),
               ("quotient", quotient), ("quotient_composed", composed),
               ("msm_a_query", msm1(q_nv, nv)), ("msm_b_g1_query", msm1(q_nv, nv)), ("msm_h_query", msm1(q_h, nh)), ("msm_l_query", msm1(q_l, nl)),
               ("msm_b_g2_query", lambda: eng._call("sylow_hip_g2_msm", g2.ptr, None, dzc.ptr, nv, pt2[0].ptr, pt2[1].ptr)),
               ("prove", prove))
        for _ in range(args.warmup):
            for _, fn in fns:
                fn()
        eng.sync()
        res = {name: [] for name, _ in fns}
        for _ in range(args.reps):                                       # the candidates alternate inside every repetition
            for name, fn in fns:
                res[name].append(timer.time_ms(fn))
        row = {"m": m, "log_n": lg, "n_vars": nv, "nnz_per_matrix": nnz}
        for name, v in res.items():
            v = sorted(v)
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_ms_min"], row[name + "_ms_max"] = round(v[0], 4), round(v[-1], 4)
        entries, byts = m * nnz, nnz * 40 + n * 8 + m * (nnz * 32 + n * 32)
        row["spmv_entries_per_s"] = round(entries / row["spmv_ms"] * 1e3)
        row["spmv_bytes_per_s"] = round(byts / row["spmv_ms"] * 1e3)
        row["spmv_share_of_hbm_peak"] = round(byts / row["spmv_ms"] * 1e3 / HBM_PEAK, 4)
        spread = max(row[k + "_ms_max"] - row[k + "_ms_min"] for k in ("quotient", "quotient_composed"))
        row["quotient_spread_ms"] = round(spread, 4)
        row["quotient_vs_composed"] = round(row["quotient_ms"] / row["quotient_composed_ms"], 3)
        row["quotient_no_slower_within_the_spread"] = bool(row["quotient_ms"] <= row["quotient_composed_ms"] + spread)
        parts = {"spmv_x3": 3 * row["spmv_ms"], "quotient": row["quotient_ms"]}
        parts.update({k: m * row[k + "_ms"] for k in ("msm_a_query", "msm_b_g1_query", "msm_b_g2_query", "msm_h_query", "msm_l_query")})
        row["share_of_prove"] = {k: round(v / row["prove_ms"], 4) for k, v in parts.items()}
        row["share_of_prove"]["the_rest"] = round(1 - sum(parts.values()) / row["prove_ms"], 4)
        row["proofs_per_s"] = round(m / row["prove_ms"] * 1e3, 2)
        # the same words from the library's call and from the composition, and on every lane pin
        quotient(); composed()
        row["quotient_equals_composition"] = bool(np.array_equal(dh.download(), dh2.download()))
        spmv()
        want, same = dsp.download(), True
        for lanes in (0, 2, 6):
            spmv(lanes, dh2)
            same = same and np.array_equal(dh2.download(), want)
        row["same_words_on_every_lane_pin"] = bool(same)
        out["rows"].append(row)
        for d in (drp, dcol, dval, dz, dr, ds, dk, dk2, g1, g1i, g2, g2i, q_nv, q_h, q_l, dzc, dsp, dabc, dh, dh2, t1, t2, dzi):
            d.free()
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
