"""Timing of PLONK's closing rounds -- sylow_popen_evaluate_batch, sylow_popen_linearise_batch and sylow_popen_open_batch (plonk_open.hip,
DESIGN.md §4.21) -- on device-resident arrays, beside the composition a caller of the library had before, on the same box in the same run.
A shape is m x log_n (W = 3 wire columns, E = 4, blinded lengths len_w = n + 2 and len_z = n + 3, no public inputs, rows of L = n + 3):
  (E)  sylow_popen_evaluate_batch: the 2 W + 1 evaluations of every instance, sigma read from the shared table;
  (L)  sylow_popen_linearise_batch: the scalars and weights on the device, the fused kernel writing r and F, r(zeta) and the status;
  (C)  the composition from existing calls: sylow_hip_kzg_quotient_batch with q_out = NULL over 2 W rows per instance, replicated and
       padded to L, one point per row; then sylow_hip_fr_lincomb_batch over two groups per instance, r's rows and F's rows, each padded to
       L, the E chunks of t copied out of t, the constant term as a unit row.  In its favour and outside its window: its packing (the
       shared selector and sigma rows copied once per instance, and r's rows twice, since a group is a run of consecutive rows) and its
       weights, which a caller forms on the HOST from the evaluations between the two device phases, are handed to it for nothing.
  (O)  sylow_popen_open_batch: the full route, with its two multi-scalar multiplications of L coefficients per instance.  The SRS of the
       timing is L arbitrary points of G1: the work does not depend on their logarithms.
Before anything is timed (C) must give the words of (E) and (L), bit for bit.  Device events around each call, warm-up calls first; the
candidates ALTERNATE inside every repetition in one process, the median of --reps is reported with its minimum and maximum.  Bytes per
column of the fused kernel are from the shapes: 32 (3 W + 3 + E) read (2 W + 2 table rows, z, W wires, E chunks of t) and 64 written.
Prints ONE JSON object and, with --out, writes it.

    python tools/bench_plonk_open.py [--shapes 1x16,8x16,1x20,8x20] [--warmup 2] [--reps 7] [--out profiles/plonk_open/bench_plonk_open.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_plonk_open.py --shapes 1x20 --warmup 0 --reps 1 --only-open"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_g1_ntt import points, random_scalars  # noqa: E402
from bench_kzg_evals import measure  # noqa: E402
from bench_msm import Timer, words_to_ints  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
WIRES, LOG_E = 3, 2
ROOT28 = pow(5, (R - 1) >> 28, R)
HBM_PEAK_GB_S = 8000.0


def to_words(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64)


def host_weights(ev, shifts, beta, gamma, alpha, zeta, v, log_n):
    """what a caller of the composition computes on the host between its two device phases: (the weights of r's rows in the order the
    table has them, then z, then the E chunks, then the constant term; the weights of the rows F adds: the wires, then sigma_0 .. sigma_(W-2))"""
    W, n, E = WIRES, 1 << log_n, 1 << LOG_E
    a, sg, zw, p = ev[:W], ev[W:2 * W - 1], ev[2 * W - 1], ev[2 * W]
    zn = pow(zeta, n, R)
    zh = (zn - 1) % R
    l1 = zh * pow(n * (zeta - 1) % R, R - 2, R) % R
    A = B = 1
    for j in range(W):
        A = A * (a[j] + beta * shifts[j] * zeta + gamma) % R
    for j in range(W - 1):
        B = B * (a[j] + beta * sg[j] + gamma) % R
    abz = alpha * B * zw % R
    r = a + [a[0] * a[1] % R, 1] + [0] * (W - 1) + [(-abz * beta) % R, (alpha * A + alpha * alpha * l1) % R] + [(-zh * pow(zn, e, R)) % R for e in range(E)]
    r.append((p - abz * (a[W - 1] + gamma) - alpha * alpha * l1) % R)
    return r, [pow(v, 1 + j, R) for j in range(W)] + [pow(v, W + 1 + j, R) for j in range(W - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x16,8x16,1x20,8x20")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scratch-gb", type=int, default=8, help="sylow_hip_set_scratch_limit for the run")
    ap.add_argument("--only-open", action="store_true", help="run (O) alone, warmup + reps times, and time nothing: for a kernel-trace run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    eng.set_scratch_limit(args.scratch_gb << 30)
    timer = Timer(eng.stream)
    W, E = WIRES, 1 << LOG_E
    shapes = [tuple(int(x) for x in p.split("x")) for p in args.shapes.split(",") if p]
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "wires": W, "log_e": LOG_E, "rows": []}
    srs = points(eng, random_scalars(np.random.default_rng(7), (1 << max(lg for _, lg in shapes)) + 3))
    for m, log_n in shapes:
        n = 1 << log_n
        big, len_w, len_z, L = n << LOG_E, n + 2, n + 3, n + 3
        rng = np.random.default_rng(2005 * m + log_n)
        base = random_scalars(rng, 4 * n + 3)
        row = lambda k, length: np.ascontiguousarray(np.roll(base, 7 * k, axis=0)[:length].T)          # [4][length], below r
        ctable = eng.to_device(np.stack([row(1000 + i, n) for i in range(2 * W + 2)]))
        shifts = [1, 5, 7]
        ch = {k: random_scalars(rng, m) for k in ("beta", "gamma", "alpha", "zeta", "v")}
        dch = {k: eng.to_device_soa(x, 4) for k, x in ch.items()}
        dsh = eng.to_device_soa(to_words(shifts), 4)
        wires = np.stack([row(s * W + j, len_w) for s in range(m) for j in range(W)]).reshape(m, W, 4, len_w)
        zc, tc = np.stack([row(100 + s, len_z) for s in range(m)]), np.stack([row(200 + s, big) for s in range(m)])
        dwires, dz, dt = eng.to_device(wires), eng.to_device(zc), eng.to_device(tc)
        dev, dr, df, dst = eng.empty((4, (2 * W + 1) * m)), eng.empty((m, 4, L)), eng.empty((m, 4, L)), eng.empty((m,), np.uint8)
        dsrs = eng.to_device_soa(srs[:L], 8)
        dev2, dp1, dp2, di1, di2, dst2 = eng.empty((4, (2 * W + 1) * m)), eng.empty((8, m)), eng.empty((8, m)), eng.empty((m,), np.uint8), eng.empty((m,), np.uint8), eng.empty((m,), np.uint8)

        def evaluate():
            eng._call("sylow_popen_evaluate_batch", ctable.ptr, dwires.ptr, len_w, dz.ptr, len_z, None, dch["zeta"].ptr, log_n, W, m, dev.ptr)

        def linearise():
            eng._call("sylow_popen_linearise_batch", ctable.ptr, dwires.ptr, len_w, dz.ptr, len_z, dt.ptr, dev.ptr, dsh.ptr, dch["beta"].ptr, dch["gamma"].ptr,
                      dch["alpha"].ptr, dch["zeta"].ptr, dch["v"].ptr, log_n, LOG_E, W, m, L, dr.ptr, df.ptr, dst.ptr)

        def full_open():
            eng._call("sylow_popen_open_batch", dsrs.ptr, ctable.ptr, dwires.ptr, len_w, dz.ptr, len_z, None, dt.ptr, dsh.ptr, dch["beta"].ptr, dch["gamma"].ptr,
                      dch["alpha"].ptr, dch["zeta"].ptr, dch["v"].ptr, log_n, LOG_E, W, m, L, dev2.ptr, dp1.ptr, di1.ptr, dp2.ptr, di2.ptr, dst2.ptr)

        if args.only_open:
            for _ in range(args.warmup + args.reps):
                full_open()
            eng.sync()
            continue
        evaluate()
        linearise()
        eng.sync()
        ev_words = eng.from_device_soa(dev)
        ev = [words_to_ints(ev_words[s * (2 * W + 1):(s + 1) * (2 * W + 1)]) for s in range(m)]
        # ---- what the composition is handed: the rows of its evaluation, [m][2 W][4][L], a point per row; the rows of its linear combination,
        # per instance r's R rows and then F's R + 2 W - 1 rows, each [4][L]; the weights, from the host
        ints = {k: words_to_ints(x) for k, x in ch.items()}
        w_n = pow(ROOT28, 1 << (28 - log_n), R)
        ct = ctable.download()
        pad = lambda a: np.concatenate([a, np.zeros((4, L - a.shape[1]), dtype=np.uint64)], axis=1)
        unit = np.zeros((4, L), dtype=np.uint64)
        unit[0, 0] = 1
        n_r, n_f = 2 * W + 2 + 1 + E + 1, 2 * W - 1
        per = 2 * n_r + n_f
        dlin, dpack = eng.empty((m * per, 4, L)), eng.empty((m * 2 * W, 4, L))
        weights, pts = [], []
        for s in range(m):
            r_rows = [pad(ct[i]) for i in range(2 * W + 2)] + [pad(zc[s])] + [pad(tc[s][:, e * n:(e + 1) * n]) for e in range(E)] + [unit]
            f_rows = [pad(wires[s, j]) for j in range(W)] + [pad(ct[W + 2 + j]) for j in range(W - 1)]
            block = np.ascontiguousarray(np.stack(r_rows + r_rows + f_rows))
            eng.lib.sylow_hip_memcpy_h2d(dlin.ptr + s * per * 32 * L, block.ctypes.data, block.nbytes, eng.stream)
            eng.sync()
            e_rows = np.ascontiguousarray(np.stack([pad(wires[s, j]) for j in range(W)] + [pad(ct[W + 2 + j]) for j in range(W - 1)] + [pad(zc[s])]))
            eng.lib.sylow_hip_memcpy_h2d(dpack.ptr + s * 2 * W * 32 * L, e_rows.ctypes.data, e_rows.nbytes, eng.stream)
            eng.sync()
            wr, wf = host_weights(ev[s], shifts, ints["beta"][s], ints["gamma"][s], ints["alpha"][s], ints["zeta"][s], ints["v"][s], log_n)
            weights += wr + wr + wf
            pts += [ints["zeta"][s]] * (2 * W - 1) + [ints["zeta"][s] * w_n % R]
        dweights, dpts = eng.to_device_soa(to_words(weights), 4), eng.to_device_soa(to_words(pts), 4)
        gs = np.array(sorted([s * per for s in range(m)] + [s * per + n_r for s in range(m)]) + [m * per], dtype=np.uint64)
        dy, dcomb = eng.empty((4, 2 * W * m)), eng.empty((2 * m, 4, L))

        def composition():
            eng._call("sylow_hip_kzg_quotient_batch", dpack.ptr, L, 2 * W * m, dpts.ptr, None, dy.ptr)
            eng._call("sylow_hip_fr_lincomb_batch", dlin.ptr, L, m * per, dweights.ptr, gs.ctypes.data, 2 * m, dcomb.ptr)

        def fused():
            evaluate()
            linearise()

        composition()
        full_open()
        eng.sync()
        comb, y = dcomb.download(), eng.from_device_soa(dy).reshape(m, 2 * W, 4)
        row_out = {"m": m, "log_n": log_n, "rows_of_length": L}
        row_out["composition_gives_the_same_words"] = bool(np.array_equal(comb[0::2], dr.download()) and np.array_equal(comb[1::2], df.download()) and
                                                           np.array_equal(y, ev_words.reshape(m, 2 * W + 1, 4)[:, :2 * W]))
        row_out["open_gives_the_same_evaluations"] = bool(np.array_equal(dev2.download(), dev.download()))
        row_out["status"] = [int(x) for x in dst.download()]
        row_out["composition_bytes_packed"] = int(dlin.nbytes + dpack.nbytes)
        row_out["fused_bytes_read_in_place"] = int(ctable.nbytes + dwires.nbytes + dz.nbytes + dt.nbytes)
        row_out.update(measure(timer, eng, [("evaluate", evaluate), ("linearise", linearise), ("fused", fused), ("composition", composition), ("open", full_open)],
                               args.warmup, args.reps))
        row_out["composition_over_fused"] = round(row_out["composition_ms"] / row_out["fused_ms"], 3)
        row_out["fused_share_of_open"] = round(row_out["fused_ms"] / row_out["open_ms"], 4)
        cols = m * L
        row_out["fold_bytes_per_column"] = 32 * (3 * W + 3 + E) + 64
        row_out["linearise_gb_per_s_lower_bound"] = round((32 * (3 * W + 3 + E) + 64) * cols / row_out["linearise_ms"] / 1e6, 1)
        row_out["linearise_share_of_hbm_peak_lower_bound"] = round(row_out["linearise_gb_per_s_lower_bound"] / HBM_PEAK_GB_S, 4)
        row_out["linearise_ns_per_column"] = round(row_out["linearise_ms"] * 1e6 / cols, 4)
        out["rows"].append(row_out)
        for d in [ctable, dsh, dwires, dz, dt, dev, dr, df, dst, dsrs, dev2, dp1, dp2, di1, di2, dst2, dlin, dpack, dweights, dpts, dy, dcomb] + list(dch.values()):
            d.free()
        eng.trim(0)
    if args.only_open:
        return
    out["conditions_met"] = bool(all(r["composition_gives_the_same_words"] and r["open_gives_the_same_evaluations"] for r in out["rows"]))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
