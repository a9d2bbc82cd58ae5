"""Timing of the KZG calls -- sylow_hip_kzg_fold_batch, sylow_hip_kzg_verify_batch, sylow_hip_kzg_batch_verify_weighted -- against the
COMPOSED routes a host had before them, built from older entry points only:
  (a) the fold against sylow_hip_g1_generator_mul_batch(y) + sylow_hip_g1_scalar_mul_batch(pi, z) + sylow_hip_g1_add_batch + sylow_hip_g1_sub_batch;
  (b) kzg_verify_batch against that composition followed by sylow_hip_bls_verify_hashed_batch with tau_g2 replicated n times;
  (c) the weighted one-boolean call (no counterpart).
n = 2^12, 2^16, 2^20 (or --sizes).  Openings are valid: a pool of 256 made in Fr (generator multiples through
sylow_hip_g1_generator_mul_batch), tiled to n.  Device events around each call, warm-up calls first; the routes ALTERNATE inside every
repetition in one process, the median of --reps is reported.  Every row checks that the fold routes agree bit for bit and that all routes
accept every opening.  Prints ONE JSON object.

    python tools/bench_kzg.py [--sizes 12,16,20] [--warmup 2] [--reps 5]"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_groth16 import R, limbs  # noqa: E402
from bench_msm import Timer  # noqa: E402

POOL = 256


def make_pool(eng, seed):
    """POOL valid openings under one SRS: (tau_g2 [1, 16], c [POOL, 8], z, y [POOL, 4], pi [POOL, 8])"""
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)
    tau = fr()
    c, z, y = ([fr() for _ in range(POOL)] for _ in range(3))
    pi = [(c[i] - y[i]) * pow(tau - z[i], R - 2, R) % R for i in range(POOL)]
    g1 = lambda ks: eng.g1_generator_mul(limbs(ks))[0]
    return eng.g2_generator_mul(limbs([tau]))[0], g1(c), limbs(z), limbs(y), g1(pi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "rows": []}
    tau, pc, pz, py, ppi = make_pool(eng, 20261018)
    d_tau = eng.to_device_soa(tau, 16)
    for lg in [int(v) for v in args.sizes.split(",")]:
        n = 1 << lg
        idx = np.arange(n) % POOL
        dc, dz, dy, dpi = eng.to_device_soa(pc[idx], 8), eng.to_device_soa(pz[idx], 4), eng.to_device_soa(py[idx], 4), eng.to_device_soa(ppi[idx], 8)
        d_taus = eng.to_device_soa(np.repeat(tau, n, 0), 16)
        rng = np.random.default_rng(lg)
        w = np.zeros((n, 4), dtype=np.uint64)
        w[:, 0] = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
        dw = eng.to_device_soa(w, 4)
        pt = lambda: (eng.empty((8, n)), eng.empty((n,), np.uint8))
        (f, fi), (yg, ygi), (zp, zpi), (s, si), (fc, fci) = pt(), pt(), pt(), pt(), pt()
        ok_new, ok_old = eng.empty((n,), np.uint8), eng.empty((n,), np.uint8)
        gt, one = eng.empty((48, 1)), eng.empty((1,), np.uint8)

        def fold():
            eng._call("sylow_hip_kzg_fold_batch", dc.ptr, None, dz.ptr, dy.ptr, dpi.ptr, None, f.ptr, fi.ptr, n)

        def fold_composed():
            eng._call("sylow_hip_g1_generator_mul_batch", dy.ptr, yg.ptr, ygi.ptr, n)
            eng._call("sylow_hip_g1_scalar_mul_batch", dpi.ptr, None, dz.ptr, zp.ptr, zpi.ptr, n)
            eng._call("sylow_hip_g1_add_batch", dc.ptr, None, zp.ptr, zpi.ptr, s.ptr, si.ptr, n)
            eng._call("sylow_hip_g1_sub_batch", s.ptr, si.ptr, yg.ptr, ygi.ptr, fc.ptr, fci.ptr, n)

        def verify():
            eng._call("sylow_hip_kzg_verify_batch", d_tau.ptr, dc.ptr, None, dz.ptr, dy.ptr, dpi.ptr, None, ok_new.ptr, n)

        def verify_composed():
            fold_composed()
            eng._call("sylow_hip_bls_verify_hashed_batch", d_taus.ptr, None, dpi.ptr, None, fc.ptr, fci.ptr, ok_old.ptr, n)

        def weighted():
            eng._call("sylow_hip_kzg_batch_verify_weighted", d_tau.ptr, dc.ptr, None, dz.ptr, dy.ptr, dpi.ptr, None, dw.ptr, n, gt.ptr, one.ptr)

        fns = (("fold", fold), ("fold_composed", fold_composed), ("verify", verify), ("verify_composed", verify_composed), ("weighted", weighted))
        for _ in range(args.warmup):
            for _, fn in fns:
                fn()
        eng.sync()
        res = {name: [] for name, _ in fns}
        for _ in range(args.reps):                                   # the routes alternate inside every repetition
            for name, fn in fns:
                res[name].append(timer.time_ms(fn))
        row = {"n": n}
        for name, v in res.items():
            v = sorted(v)
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_ms_min"], row[name + "_ms_max"] = round(v[0], 4), round(v[-1], 4)
        row["fold_speedup"] = round(row["fold_composed_ms"] / row["fold_ms"], 2)
        row["verify_speedup"] = round(row["verify_composed_ms"] / row["verify_ms"], 2)
        row["weighted_vs_n_openings"] = round(row["verify_ms"] / row["weighted_ms"], 2)
        row["openings_per_s"] = {k: round(n / row[k + "_ms"] * 1e3) for k in ("fold", "verify", "verify_composed", "weighted")}
        row["same_fold"] = bool(np.array_equal(f.download(), fc.download()) and np.array_equal(fi.download(), fci.download()))
        row["all_ok"] = [bool(ok_new.download().all()), bool(ok_old.download().all()), bool(one.download()[0])]
        out["rows"].append(row)
        for d in (dc, dz, dy, dpi, d_taus, dw, f, fi, yg, ygi, zp, zpi, s, si, fc, fci, ok_new, ok_old, gt, one):
            d.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
