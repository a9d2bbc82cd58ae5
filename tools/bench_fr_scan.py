"""Timing of the ratio scan and of PLONK's permutation grand product -- sylow_hip_fr_ratio_scan_batch and sylow_hip_plonk_permutation_batch
(fr_scan.hip) -- on device-resident arrays, beside two baselines on the same box in the same run.  A shape is m x log_n
(W = 3 wire columns for the permutation entry):
  (S)  sylow_hip_fr_ratio_scan_batch, product, with numerators;
  (P)  sylow_hip_plonk_permutation_batch;
  (a)  the device ingredients of the same arithmetic alone, as the library had them before: sylow_hip_fr_batch_inv of the denominators and
       sylow_hip_fr_mul_batch with the numerators over the same m n elements.  NO SCAN: a lower composition, not a competitor;
  (b)  the route a caller had: (a), a download of the ratios, the prefix product in host integers, and an upload.  Wall clock, once per
       shape; above --host-max elements the host loop runs over the first --host-max of them and is scaled linearly (`host_scaled`).
Before anything is timed the scan must satisfy out[k + 1] = out[k] t[k] word for word against the ratios of (a), through
sylow_hip_fr_mul_batch (shapes up to --host-max elements).  Device events around each call, warm-up calls first; the candidates ALTERNATE
inside every repetition in one process, the median of --reps is reported with its minimum and maximum.  Bytes per second are against the
ALGORITHMIC traffic: 96 bytes per element for (S) (num and den in, out out), 32 (W m + W + m) n for (P).  Prints ONE JSON object and, with
--out, writes it.

    python tools/bench_fr_scan.py [--warmup 2] [--reps 7] [--out profiles/fr_scan/bench_fr_scan.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_g1_ntt import random_scalars  # noqa: E402
from bench_kzg_evals import measure  # noqa: E402
from bench_msm import Timer, words_to_ints  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
WIRES = 3


def host_prefix(t):
    """the exclusive prefix product of [count, 4] words in host integers, back as words"""
    vals = words_to_ints(t)
    out, run = np.empty((len(vals), 4), dtype=np.uint64), 1
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (run >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        run = run * v % R
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x16,1x20,1x24,64x16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-max", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "wires": WIRES, "rows": []}
    for m, log_n in [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",") if p]:
        n = 1 << log_n
        total = m * n
        rng = np.random.default_rng(1009 * m + log_n)
        soa = lambda rows: np.ascontiguousarray(random_scalars(rng, rows * n).reshape(rows, n, 4).transpose(0, 2, 1))
        dnum, dden, dwires, dsigma = eng.to_device(soa(m)), eng.to_device(soa(m)), eng.to_device(soa(m * WIRES)), eng.to_device(soa(WIRES))
        dsh, dbeta, dgamma = eng.to_device_soa(random_scalars(rng, WIRES), 4), eng.to_device_soa(random_scalars(rng, m), 4), eng.to_device_soa(random_scalars(rng, m), 4)
        dout, dz, dtot, dst = eng.empty((m, 4, n)), eng.empty((m, 4, n)), eng.empty((4, m)), eng.empty((m,), np.uint8)
        dinv, dt = eng.empty((m, 4, n)), eng.empty((m, 4, n))

        def scan():
            eng._call("sylow_hip_fr_ratio_scan_batch", dnum.ptr, dden.ptr, n, m, 1, dout.ptr, dtot.ptr, dst.ptr)

        def permutation():
            eng._call("sylow_hip_plonk_permutation_batch", dwires.ptr, dsigma.ptr, dsh.ptr, dbeta.ptr, dgamma.ptr, log_n, WIRES, m, dz.ptr, dtot.ptr, dst.ptr)

        def ingredients():
            for j in range(m):                                      # the two calls take one [4][count] array: row by row
                off = j * 32 * n
                eng._call("sylow_hip_fr_batch_inv", dden.ptr + off, dinv.ptr + off, n)
                eng._call("sylow_hip_fr_mul_batch", dnum.ptr + off, dinv.ptr + off, dt.ptr + off, n)

        row = {"m": m, "log_n": log_n}
        if total <= args.host_max:                                  # out[k + 1] = out[k] t[k], through sylow_hip_fr_mul_batch
            scan()
            ingredients()
            eng.sync()
            o, t = dout.download(), dt.download()
            ok = True
            for j in range(m):
                oj, tj = np.ascontiguousarray(o[j].T), np.ascontiguousarray(t[j].T)
                ok = ok and np.array_equal(eng.fr_mul(oj[:-1], tj[:-1]), oj[1:]) and oj[0].tolist() == [1, 0, 0, 0]
            row["scan_is_the_prefix_of_the_ratios"] = bool(ok and not dst.download().any())
        row.update(measure(timer, eng, [("scan", scan), ("permutation", permutation), ("ingredients", ingredients)], args.warmup, args.reps))
        # (b): wall clock, once
        count = min(total, args.host_max)
        t0 = time.perf_counter()
        ingredients()
        eng.sync()
        t = dt.download()
        t1 = time.perf_counter()
        flat = np.ascontiguousarray(t.transpose(0, 2, 1)).reshape(total, 4)[:count]
        h0 = time.perf_counter()
        pre = host_prefix(flat)
        host_s = (time.perf_counter() - h0) * (total / count)
        t2 = time.perf_counter()
        dz.upload(np.ascontiguousarray(np.resize(pre, (total, 4)).reshape(m, n, 4).transpose(0, 2, 1)))
        eng.sync()
        up_s = time.perf_counter() - t2
        row["host_route_ms"] = round(((t1 - t0) + host_s + up_s) * 1e3, 1)
        row["host_route_parts_ms"] = {"ingredients_and_download": round((t1 - t0) * 1e3, 1), "host_prefix": round(host_s * 1e3, 1), "upload": round(up_s * 1e3, 1)}
        row["host_scaled"] = bool(count < total)
        row["scan_over_ingredients"] = round(row["scan_ms"] / row["ingredients_ms"], 3)
        row["permutation_over_ingredients"] = round(row["permutation_ms"] / row["ingredients_ms"], 3)
        row["host_route_over_scan"] = round(row["host_route_ms"] / row["scan_ms"], 1)
        row["scan_gb_per_s"] = round(96 * total / row["scan_ms"] / 1e6, 1)
        row["permutation_gb_per_s"] = round(32 * (WIRES * m + WIRES + m) * n / row["permutation_ms"] / 1e6, 1)
        row["scan_beats_host_route"] = bool(row["scan_ms"] < row["host_route_ms"])
        out["rows"].append(row)
        for d in (dnum, dden, dwires, dsigma, dsh, dbeta, dgamma, dout, dz, dtot, dst, dinv, dt):
            d.free()
    out["conditions_met"] = bool(all(r.get("scan_is_the_prefix_of_the_ratios", True) for r in out["rows"]))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
