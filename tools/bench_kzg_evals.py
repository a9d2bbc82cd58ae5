"""Timing of the evaluation-form KZG unit -- sylow_hip_fr_batch_inv, sylow_hip_kzg_quotient_evals_batch, sylow_hip_kzg_open_evals_batch --
beside the calls the library had for the same words (the two conditions of DESIGN.md §4.11; both against the spread of this same
alternating run):
  (a) fr_batch_inv against sylow_hip_fr_inv_batch at n = 2^12, 2^16, 2^20 (or --inv-sizes): must be no slower; the ratio is recorded, and
      sylow_hip_fr_mul_batch over as many elements beside them (products and bytes per element);
  (b) kzg_quotient_evals_batch against the composition fr_ntt_batch(inverse), kzg_quotient_batch, fr_ntt_batch(forward) on device arrays at
      (m, log_n) = (1, 20), (64, 14) -- must be no slower -- and (4096, 8), recorded, not gated (or --shapes; --gated names the gated ones);
  (c) open_evals against fr_ntt_batch(inverse) + kzg_open_batch -- recorded, not gated: both are dominated by the same multi-scalar
      multiplication.  The monomial SRS is tau^k G1gen through the fixed-base call; the Lagrange SRS is made on the device from it:
      L_i(tau) = (tau^n - 1) n^-1 w^i / (tau - w^i), the w^i as the transform of X, the inverses through fr_batch_inv itself.
Values and points z are random 256-bit words; every row checks that the candidates agree bit for bit.  Device events around each call,
warm-up calls first; the candidates ALTERNATE inside every repetition in one process, the median of --reps is reported with its minimum and
maximum.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_kzg_evals.py [--warmup 1] [--reps 5] [--out profiles/kzg_evals/bench_kzg_evals.json]"""
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

TAU = 0x2F1E0D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978 % R


def words(v):
    return np.frombuffer((v % R).to_bytes(32, "little"), dtype=np.uint64).reshape(1, 4)


def lagrange_srs(eng, log_n):
    """L_i(tau) G1gen, i < n, as affine words [n, 8]: scalars on the device, then g1_scalar_mul_batch on copies of the generator"""
    n = 1 << log_n
    x = np.zeros((n, 4), dtype=np.uint64)
    x[1 % n, 0] = 1
    w = eng.fr_ntt(x) if log_n else np.array([[1, 0, 0, 0]], dtype=np.uint64)
    c = (pow(TAU, n, R) - 1) * pow(n, R - 2, R) % R
    lag = eng.fr_mul(eng.fr_mul(np.tile(words(c), (n, 1)), w), eng.fr_batch_inv(eng.fr_sub(np.tile(words(TAU), (n, 1)), w)))
    gen = np.tile(np.array([1, 0, 0, 0, 2, 0, 0, 0], dtype=np.uint64), (n, 1))
    step, parts = 1 << 16, []                                       # in pieces: every lane of the call leases a 1 KB window table
    for i in range(0, n, step):
        xy, inf = eng.g1_scalar_mul(gen[i:i + step], lag[i:i + step])
        assert not inf.any()
        parts.append(xy)
    return np.concatenate(parts)


def measure(timer, eng, fns, warmup, reps):
    for _ in range(warmup):
        for _, fn in fns:
            fn()
    eng.sync()
    res = {name: [] for name, _ in fns}
    for _ in range(reps):                                           # the candidates alternate inside every repetition
        for name, fn in fns:
            res[name].append(timer.time_ms(fn))
    row = {}
    for name, v in res.items():
        v = sorted(v)
        row[name + "_ms"] = round(v[len(v) // 2], 4)
        row[name + "_ms_min"], row[name + "_ms_max"] = round(v[0], 4), round(v[-1], 4)
    return row


def gate(row, new, old):
    spread = max(row[new + "_ms_max"] - row[new + "_ms_min"], row[old + "_ms_max"] - row[old + "_ms_min"])
    row["spread_ms"] = round(spread, 4)
    row[old + "_over_" + new] = round(row[old + "_ms"] / row[new + "_ms"], 3)
    row[new + "_no_slower"] = bool(row[new + "_ms"] <= row[old + "_ms"] + spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inv-sizes", default="12,16,20")
    ap.add_argument("--shapes", default="1x20,64x14,4096x8")
    ap.add_argument("--gated", default="1x20,64x14")
    ap.add_argument("--open-shapes", default="1x20,64x14,4096x8")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "batch_inv": [], "quotient_evals": [], "open_evals": []}
    pairs = lambda s: [tuple(int(v) for v in p.split("x")) for p in s.split(",") if p]

    # ---- (a) the inversion ----------------------------------------------------------------------------------------------------------
    for lg in [int(v) for v in args.inv_sizes.split(",") if v]:
        n = 1 << lg
        rng = np.random.default_rng(lg)
        da = eng.to_device(rng.integers(0, 1 << 64, size=(4, n), dtype=np.uint64, endpoint=False))
        d_new, d_old, d_mul = eng.empty((4, n)), eng.empty((4, n)), eng.empty((4, n))
        fns = (("batch_inv", lambda: eng._call("sylow_hip_fr_batch_inv", da.ptr, d_new.ptr, n)),
               ("inv_batch", lambda: eng._call("sylow_hip_fr_inv_batch", da.ptr, d_old.ptr, n)),
               ("fr_mul", lambda: eng._call("sylow_hip_fr_mul_batch", da.ptr, da.ptr, d_mul.ptr, n)))
        row = {"n": n, **measure(timer, eng, fns, args.warmup, args.reps)}
        gate(row, "batch_inv", "inv_batch")
        row["batch_inv_vs_fr_mul"] = round(row["batch_inv_ms"] / row["fr_mul_ms"], 2)
        row["ns_per_element"] = {k: round(row[k + "_ms"] * 1e6 / n, 3) for k in ("batch_inv", "inv_batch", "fr_mul")}
        row["same_words"] = bool(np.array_equal(d_new.download(), d_old.download()))
        out["batch_inv"].append(row)
        for d in (da, d_new, d_old, d_mul):
            d.free()

    # ---- (b) the quotient -----------------------------------------------------------------------------------------------------------
    gated = set(pairs(args.gated))
    for m, lg in pairs(args.shapes):
        n = 1 << lg
        rng = np.random.default_rng(m + lg)
        de = eng.to_device(rng.integers(0, 1 << 64, size=(m, 4, n), dtype=np.uint64, endpoint=False))      # [m][4][n], any words
        dz = eng.to_device_soa(rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64, endpoint=False), 4)
        dq, dy = eng.empty((m, 4, n)), eng.empty((4, m))
        t1, t2, rq, ry = eng.empty((m, 4, n)), eng.empty((m, 4, n)), eng.empty((m, 4, n)), eng.empty((4, m))
        dm = eng.empty((4, m * n))

        def evals_route():
            eng._call("sylow_hip_kzg_quotient_evals_batch", de.ptr, lg, m, dz.ptr, dq.ptr, dy.ptr)

        def evaluate_only():
            eng._call("sylow_hip_kzg_quotient_evals_batch", de.ptr, lg, m, dz.ptr, None, dy.ptr)

        def composition():
            eng._call("sylow_hip_fr_ntt_batch", de.ptr, lg, m, 1, None, t1.ptr)
            eng._call("sylow_hip_kzg_quotient_batch", t1.ptr, n, m, dz.ptr, t2.ptr, ry.ptr)
            eng._call("sylow_hip_fr_ntt_batch", t2.ptr, lg, m, 0, None, rq.ptr)

        def fr_mul():
            eng._call("sylow_hip_fr_mul_batch", de.ptr, de.ptr, dm.ptr, m * n)

        fns = (("quotient_evals", evals_route), ("composition", composition), ("evaluate_only", evaluate_only), ("fr_mul", fr_mul))
        row = {"m": m, "log_n": lg, **measure(timer, eng, fns, args.warmup, args.reps)}
        gate(row, "quotient_evals", "composition")
        row["gated"] = (m, lg) in gated
        row["quotient_evals_vs_fr_mul"] = round(row["quotient_evals_ms"] / row["fr_mul_ms"], 2)
        row["ns_per_element"] = {k: round(row[k + "_ms"] * 1e6 / (m * n), 3) for k in ("quotient_evals", "composition", "evaluate_only", "fr_mul")}
        evals_route()
        composition()
        row["same_words"] = bool(np.array_equal(dq.download(), rq.download()) and np.array_equal(dy.download(), ry.download()))
        out["quotient_evals"].append(row)
        for d in (de, dz, dq, dy, t1, t2, rq, ry, dm):
            d.free()

    # ---- (c) the opening ------------------------------------------------------------------------------------------------------------
    shapes = pairs(args.open_shapes)
    if shapes:
        top = max(lg for _, lg in shapes)
        mono_all = srs_points(eng, 1 << top, TAU)
    for m, lg in shapes:
        n = 1 << lg
        rng = np.random.default_rng(3 * m + lg)
        de = eng.to_device(rng.integers(0, 1 << 64, size=(m, 4, n), dtype=np.uint64, endpoint=False))
        dz = eng.to_device_soa(rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64, endpoint=False), 4)
        d_lag, d_mono = eng.to_device_soa(lagrange_srs(eng, lg), 8), eng.to_device_soa(mono_all[:n], 8)
        t1 = eng.empty((m, 4, n))
        ya, yb = eng.empty((4, m)), eng.empty((4, m))
        pa, pai, pb, pbi = eng.empty((8, m)), eng.empty((m,), np.uint8), eng.empty((8, m)), eng.empty((m,), np.uint8)

        def open_evals():
            eng._call("sylow_hip_kzg_open_evals_batch", d_lag.ptr, de.ptr, lg, m, dz.ptr, ya.ptr, pa.ptr, pai.ptr)

        def intt_open():
            eng._call("sylow_hip_fr_ntt_batch", de.ptr, lg, m, 1, None, t1.ptr)
            eng._call("sylow_hip_kzg_open_batch", d_mono.ptr, t1.ptr, n, m, dz.ptr, yb.ptr, pb.ptr, pbi.ptr)

        fns = (("open_evals", open_evals), ("intt_open", intt_open))
        row = {"m": m, "log_n": lg, **measure(timer, eng, fns, args.warmup, args.reps)}
        gate(row, "open_evals", "intt_open")
        row["gated"] = False
        row["same_points"] = bool(np.array_equal(pa.download(), pb.download()) and np.array_equal(pai.download(), pbi.download())
                                  and np.array_equal(ya.download(), yb.download()))
        out["open_evals"].append(row)
        for d in (de, dz, d_lag, d_mono, t1, ya, yb, pa, pai, pb, pbi):
            d.free()

    out["conditions_met"] = bool(all(r["batch_inv_no_slower"] for r in out["batch_inv"])
                                 and all(r["quotient_evals_no_slower"] for r in out["quotient_evals"] if r["gated"]))
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
