"""Timing of PLONK's quotient polynomial -- sylow_plonk_quotient_batch and sylow_plonk_quotient_evals_batch (plonk_quotient.hip, DESIGN.md
§4.20) -- on device-resident arrays, beside the composition a caller of the library had before, on the same box in the same run.  A shape is
m x log_n (W = 3 wire columns, E = 4, blinded lengths len_w = n + 2 and len_z = n + 3, no public inputs):
  (F)  sylow_plonk_quotient_batch: pad, one transform onto K, the fused kernel, one transform back, the status;
  (K)  sylow_plonk_quotient_evals_batch alone, over the values on K the composition's transform left;
  (N)  the transforms of (F) alone: sylow_hip_fr_ntt_batch forward over (W + 1) m arrays and inverse over m;
  (C)  the composition: the coefficients of z(w_n X) by one product, ONE forward transform over (W + 2) m padded arrays, then per instance
       9 W + 12 element-wise sylow_hip_fr_{mul,add,sub}_batch launches over arrays of N elements, then ONE inverse transform.  In its favour
       and outside its window: the inputs lie zero-padded already, and the arrays it needs beside the table (k_j x_i, (X^n - 1)^-1 at every
       point, w_n^k, 1, and beta, gamma, alpha, alpha^2 repeated N times) are made beforehand.
Before anything is timed (C) must give the words of (F), bit for bit, and (K) between the two transforms too.  Device events around each
call, warm-up calls first; the candidates ALTERNATE inside every repetition in one process, the median of --reps is reported with its
minimum and maximum.  Bytes per point of (K) are from the shapes: 32 (3 W + 6) read (W wires, W sigma, W + 2 selectors, L_1, z twice, the
root) and 32 written.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_plonk_quotient.py [--shapes 1x16,8x16,1x20,8x20] [--warmup 2] [--reps 7] [--out profiles/plonk_quotient/bench_plonk_quotient.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_plonk_quotient.py --shapes 1x20 --warmup 0 --reps 10 --only-full"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_g1_ntt import random_scalars  # noqa: E402
from bench_kzg_evals import measure  # noqa: E402
from bench_msm import Timer  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
WIRES, LOG_E, SHIFT = 3, 2, 5
ROOT28 = pow(5, (R - 1) >> 28, R)
HBM_PEAK_GB_S = 8000.0


def to_words(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64)


def soa_of(vals):
    """[4][count] words of a list of ints"""
    return np.ascontiguousarray(to_words(vals).T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x16,8x16,1x20,8x20")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scratch-gb", type=int, default=64, help="sylow_hip_set_scratch_limit for the run: 2^20 rows do not fit the default of 1 GB")
    ap.add_argument("--only-full", action="store_true", help="run (F) alone, warmup + reps times, and time nothing: for a kernel-trace run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    eng.set_scratch_limit(args.scratch_gb << 30)
    timer = Timer(eng.stream)
    W, E = WIRES, 1 << LOG_E
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "wires": W, "log_e": LOG_E, "rows": []}
    for m, log_n in [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",") if p]:
        n, lb = 1 << log_n, log_n + LOG_E
        big, len_w, len_z, row_b = n << LOG_E, n + 2, n + 3, 32 * (n << LOG_E)
        rng = np.random.default_rng(2003 * m + log_n)
        base = random_scalars(rng, n + 3)
        soa = lambda count, length, k: np.ascontiguousarray(np.stack([np.roll(base, 7 * (k + i), axis=0)[:length].T for i in range(count)]))
        table = eng.plonk_quotient_prepare(np.stack([np.roll(base, 3 * i, axis=0)[:n] for i in range(W + 2)]),
                                           np.stack([np.roll(base, 5 * i + 1, axis=0)[:n] for i in range(W)]), LOG_E)
        shifts = [1, 5, 7]
        dsh, dbeta, dgamma, dalpha = (eng.to_device_soa(x, 4) for x in (to_words(shifts), random_scalars(rng, m), random_scalars(rng, m), random_scalars(rng, m)))
        dwires, dz = eng.to_device(soa(m * W, len_w, 0).reshape(m, W, 4, len_w)), eng.to_device(soa(m, len_z, 100))
        dt, dst = eng.empty((m, 4, big)), eng.empty((m,), np.uint8)
        ntt = lambda src, count, inverse, shift, dst: eng._call("sylow_hip_fr_ntt_batch", src, lb, count, inverse, shift, dst)
        op = lambda name, a, b, o: eng._call("sylow_hip_fr_%s_batch" % name, a, b, o, big)

        def fused_full():
            eng._call("sylow_plonk_quotient_batch", table.ptr, dwires.ptr, len_w, dz.ptr, len_z, None, dsh.ptr, dbeta.ptr, dgamma.ptr, dalpha.ptr, log_n, LOG_E, W, m,
                      dt.ptr, dst.ptr)

        if args.only_full:
            for _ in range(args.warmup + args.reps):
                fused_full()
            eng.sync()
            continue
        # ---- what the composition needs beside the table, made beforehand: instance s holds W + 2 padded columns (wires, z, z(w_n X))
        cols = W + 2
        pad = np.zeros((m, cols, 4, big), dtype=np.uint64)
        pad[:, :W, :, :len_w] = dwires.download()
        pad[:, W, :, :len_z] = dz.download()
        dpad, dext, dcomp = eng.to_device(pad), eng.empty((m, cols, 4, big)), eng.empty((m, 4, big))
        # (K) and (N) work on arrays laid out as the entry takes them: wires_ext [m][W][4][N], then z_ext [m][4][N]
        dpad2 = eng.to_device(np.ascontiguousarray(np.concatenate([pad[:, :W].reshape(m * W, 4, big), pad[:, W]])))
        del pad
        dfive = eng.to_device(np.array([SHIFT, 0, 0, 0], dtype=np.uint64))
        w_big = pow(ROOT28, 1 << (28 - lb), R)
        zi = [pow((pow(SHIFT, n, R) * pow(w_big, n * k, R) - 1) % R, R - 2, R) for k in range(E)]
        ident = eng.plonk_identity(to_words([SHIFT * k for k in shifts]), lb)          # k_j x_i = 5 k_j w_N^i, [W, N, 4]
        did = [eng.to_device(np.ascontiguousarray(ident[j].T)) for j in range(W)]
        del ident
        dzinv = eng.to_device(np.ascontiguousarray(np.tile(soa_of(zi), (1, n))))
        powers = np.ascontiguousarray(eng.plonk_identity(to_words([1]), log_n)[0].T)    # w_n^k for k < n; w_n^(n + k) = w_n^k
        wk = np.zeros((4, big), dtype=np.uint64)
        wk[:, :n], wk[:, n:len_z] = powers, powers[:, :len_z - n]
        ones = np.zeros((4, big), dtype=np.uint64)
        ones[0] = 1
        dwk, done = eng.to_device(wk), eng.to_device(ones)
        rep = lambda d, s: eng.to_device(np.ascontiguousarray(np.repeat(d.download()[:, s:s + 1], big, axis=1)))
        dB, dG, dA = ([rep(d, s) for s in range(m)] for d in (dbeta, dgamma, dalpha))
        dA2 = [eng.empty((4, big)) for _ in range(m)]
        for s in range(m):
            op("mul", dA[s].ptr, dA[s].ptr, dA2[s].ptr)
        tmp = [eng.empty((4, big)) for _ in range(4 + W)]
        trow = lambda r: table.ptr + r * row_b

        def composition():
            for s in range(m):                                       # the coefficients of z(w_n X): z_k w_n^k
                op("mul", dpad.ptr + (s * cols + W) * row_b, dwk.ptr, dpad.ptr + (s * cols + W + 1) * row_b)
            ntt(dpad.ptr, m * cols, 0, dfive.ptr, dext.ptr)
            for s in range(m):
                col = lambda c: dext.ptr + (s * cols + c) * row_b
                g, a, b, u = (t.ptr for t in tmp[:4])
                wg = [t.ptr for t in tmp[4:]]
                op("mul", col(0), col(1), g)                          # the gate: 2 W + 3 launches
                op("mul", trow(W), g, g)
                for j in range(W):
                    op("mul", trow(j), col(j), u)
                    op("add", g, u, g)
                op("add", g, trow(W + 1), g)
                for j in range(W):                                   # the two products: 7 W launches
                    op("add", col(j), dG[s].ptr, wg[j])
                    op("mul", dB[s].ptr, did[j].ptr, u)
                    op("add", u, wg[j], u)
                    op("mul", a if j else col(W), u, a)
                    op("mul", dB[s].ptr, trow(W + 2 + j), u)
                    op("add", u, wg[j], u)
                    op("mul", b if j else col(W + 1), u, b)
                op("sub", a, b, a)                                    # alpha perm, alpha^2 L_1 (z - 1), the division: 9 launches
                op("mul", a, dA[s].ptr, a)
                op("add", g, a, g)
                op("sub", col(W), done.ptr, u)
                op("mul", u, trow(2 * W + 2), u)
                op("mul", u, dA2[s].ptr, u)
                op("add", g, u, g)
                op("mul", g, dzinv.ptr, dcomp.ptr + s * row_b)
            ntt(dcomp.ptr, m, 1, dfive.ptr, dt2.ptr)

        dt2 = eng.empty((m, 4, big))
        dzx, dtx = eng.empty((m, 4, big)), eng.empty((m, 4, big))
        dext2 = eng.empty((m * (W + 1), 4, big))

        def kernel():
            eng._call("sylow_plonk_quotient_evals_batch", table.ptr, dext2.ptr, dext2.ptr + m * W * row_b, None, dsh.ptr, dbeta.ptr, dgamma.ptr, dalpha.ptr, log_n, LOG_E, W, m,
                      dtx.ptr)

        def transforms():
            ntt(dpad2.ptr, m * (W + 1), 0, dfive.ptr, dext2.ptr)
            ntt(dtx.ptr, m, 1, dfive.ptr, dzx.ptr)

        row = {"m": m, "log_n": log_n, "launches_of_the_composition": m * (9 * W + 12) + 2}
        fused_full()
        composition()
        ntt(dpad2.ptr, m * (W + 1), 0, dfive.ptr, dext2.ptr)
        kernel()
        ntt(dtx.ptr, m, 1, dfive.ptr, dzx.ptr)
        eng.sync()
        want = dt.download()
        row["composition_gives_the_same_words"] = bool(np.array_equal(want, dt2.download()))
        row["kernel_between_transforms_gives_the_same_words"] = bool(np.array_equal(want, dzx.download()))
        row["status"] = [int(v) for v in dst.download()]
        row.update(measure(timer, eng, [("full", fused_full), ("kernel", kernel), ("transforms", transforms), ("composition", composition)], args.warmup, args.reps))
        row["composition_over_full"] = round(row["composition_ms"] / row["full_ms"], 3)
        row["kernel_share_of_full"] = round(row["kernel_ms"] / row["full_ms"], 3)
        row["kernel_bytes_per_point"] = 32 * (3 * W + 7)
        row["kernel_gb_per_s"] = round(32 * (3 * W + 7) * m * big / row["kernel_ms"] / 1e6, 1)
        row["kernel_share_of_hbm_peak"] = round(row["kernel_gb_per_s"] / HBM_PEAK_GB_S, 4)
        row["kernel_ns_per_point"] = round(row["kernel_ms"] * 1e6 / (m * big), 4)
        out["rows"].append(row)
        for d in [table, dsh, dbeta, dgamma, dalpha, dwires, dz, dt, dst, dpad, dext, dcomp, dfive, dzinv, dwk, done, dt2, dzx, dtx, dpad2, dext2] + did + dB + dG + dA + dA2 + tmp:
            d.free()
        eng.trim(0)
    if args.only_full:
        return
    out["conditions_met"] = bool(all(r["composition_gives_the_same_words"] and r["kernel_between_transforms_gives_the_same_words"] for r in out["rows"]))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
