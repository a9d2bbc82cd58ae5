"""Timing of the transform over Fr -- sylow_hip_fr_ntt_batch(_tuned) -- and of sylow_hip_kzg_commit_evals_batch at
(m, log_n) = (1, 20), (64, 14), (4096, 8) (or --shapes).  Recorded, not gated: there is no reference or parent number for the transform.
  (a) the forward transform on the default plan beside the same with the stages of a pass pinned to 1, to T / 2 and to the largest, 10; and,
      after the alternating repetitions, every pin 1 .. 10 once more (`sweep_ms`, medians of --reps, recorded for the next change of the default);
  (b) the shares of the table kernel and of the element-wise kernel, from call times alone: the inverse is the forward's launches plus the
      element-wise one, so scale = inverse - forward; the table does not depend on m, so two batch sizes give table = 2 t(m) - t(2 m);
  (c) sylow_hip_fr_mul_batch over m (n / 2) log_n elements -- the same number of Barrett products, streamed -- and products per second for both;
  (d) commit_evals beside commit at the same shapes (the SRS is tau^k G1gen through sylow_hip_g1_generator_mul_batch).
Values are random 256-bit words.  Device events around each call, warm-up calls first; the candidates ALTERNATE inside every repetition in one
process, the median of --reps is reported with its minimum and maximum.  Every row checks that the pinned plans give the default plan's words
and that commit_evals gives the points of commit over the inverse transform.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_ntt.py [--shapes 1x20,64x14,4096x8] [--warmup 1] [--reps 5] [--out profiles/ntt/bench_ntt.json]"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_groth16 import R  # noqa: E402
from bench_kzg_prove import srs_points  # noqa: E402
from bench_msm import Timer  # noqa: E402


def default_stages():
    src = open(os.path.join(ROOT, "sylow_amd", "csrc", "ntt_plan.hpp")).read()
    return int(re.search(r"constexpr int NTT_STAGES_DEFAULT = (\d+);", src).group(1))


S_MAX = 10                                                              # NTT_STAGES_MAX: the deepest pass a tile admits


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
    T = default_stages()
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "default_stages": T, "rows": []}
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    srs = srs_points(eng, 1 << max(lg for _, lg in shapes), 0x2F1E0D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978 % R)
    for m, lg in shapes:
        n = 1 << lg
        rng = np.random.default_rng(m + lg)
        din = eng.to_device(rng.integers(0, 1 << 64, size=(2 * m, 4, n), dtype=np.uint64, endpoint=False))      # [2 m][4][n], any words
        dout, dpin = eng.empty((2 * m, 4, n)), eng.empty((m, 4, n))
        products = m * (n // 2) * lg
        da, db = eng.empty((4, max(products, 1))), eng.empty((4, max(products, 1)))
        ds = eng.to_device_soa(srs[:n], 8)
        pt = lambda: (eng.empty((8, m)), eng.empty((m,), np.uint8))
        (c, ci), (ce, cei) = pt(), pt()

        def ntt(inverse=0, stages=-1, batch=m, dst=dout):
            if stages < 0:
                eng._call("sylow_hip_fr_ntt_batch", din.ptr, lg, batch, inverse, None, dst.ptr)
            else:
                eng._call("sylow_hip_fr_ntt_batch_tuned", din.ptr, lg, batch, inverse, None, stages, dst.ptr)

        fns = (("forward", lambda: ntt()), ("forward_stages_1", lambda: ntt(stages=1)), (f"forward_stages_{T // 2}", lambda: ntt(stages=T // 2)),
               (f"forward_stages_{S_MAX}", lambda: ntt(stages=S_MAX)),
               ("inverse", lambda: ntt(inverse=1)), ("forward_2m", lambda: ntt(batch=2 * m)),
               ("fr_mul", lambda: eng._call("sylow_hip_fr_mul_batch", da.ptr, da.ptr, db.ptr, products)),
               ("commit", lambda: eng._call("sylow_hip_kzg_commit_batch", ds.ptr, din.ptr, n, m, c.ptr, ci.ptr)),
               ("commit_evals", lambda: eng._call("sylow_hip_kzg_commit_evals_batch", ds.ptr, din.ptr, lg, m, ce.ptr, cei.ptr)))
        for _ in range(args.warmup):
            for _, fn in fns:
                fn()
        eng.sync()
        res = {name: [] for name, _ in fns}
        for _ in range(args.reps):                                       # the candidates alternate inside every repetition
            for name, fn in fns:
                res[name].append(timer.time_ms(fn))
        row = {"m": m, "log_n": lg, "passes_default": -(-lg // T)}
        for name, v in res.items():
            v = sorted(v)
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_ms_min"], row[name + "_ms_max"] = round(v[0], 4), round(v[-1], 4)
        names = [name for name, _ in fns[:4]]
        row["spread_ms"] = round(max(row[k + "_ms_max"] - row[k + "_ms_min"] for k in names), 4)
        best = min(names, key=lambda k: row[k + "_ms"])
        row["fastest_plan"] = best
        row["a_pin_beats_the_default_outside_the_spread"] = bool(row[best + "_ms"] + row["spread_ms"] < row["forward_ms"])
        # shares from call times: scale = inverse - forward; table = 2 t(m) - t(2 m)
        row["scale_share_of_inverse"] = round(max(row["inverse_ms"] - row["forward_ms"], 0.0) / row["inverse_ms"], 4)
        row["table_share_of_forward"] = round(max(2 * row["forward_ms"] - row["forward_2m_ms"], 0.0) / row["forward_ms"], 4)
        row["butterfly_products"] = products
        row["products_per_s"] = {"forward": round(products / row["forward_ms"] * 1e3), "fr_mul": round(products / row["fr_mul_ms"] * 1e3)}
        row["forward_vs_fr_mul"] = round(row["forward_ms"] / row["fr_mul_ms"], 3)
        row["bytes_per_pass"] = 64 * m * n
        row["pass_bytes_per_s"] = round(row["passes_default"] * 64 * m * n / row["forward_ms"] * 1e3)
        row["commit_evals_vs_commit"] = round(row["commit_evals_ms"] / row["commit_ms"], 3)
        row["sweep_ms"] = {}
        for stages in range(1, S_MAX + 1):
            v = sorted(timer.time_ms(lambda: ntt(stages=stages)) for _ in range(args.reps))
            row["sweep_ms"][str(stages)] = round(v[len(v) // 2], 4)
        # the same words on every plan; the same points from values and from coefficients
        ntt()
        same = True
        for stages in (1, T // 2, S_MAX):
            ntt(stages=stages, dst=dpin)
            same = same and np.array_equal(dpin.download(), dout.download()[:m])
        row["same_words_on_every_plan"] = bool(same)
        ntt(inverse=1, dst=dpin)
        eng._call("sylow_hip_kzg_commit_batch", ds.ptr, dpin.ptr, n, m, c.ptr, ci.ptr)
        eng._call("sylow_hip_kzg_commit_evals_batch", ds.ptr, din.ptr, lg, m, ce.ptr, cei.ptr)
        row["same_points"] = bool(np.array_equal(c.download(), ce.download()) and np.array_equal(ci.download(), cei.download()))
        out["rows"].append(row)
        for d in (din, dout, dpin, da, db, ds, c, ci, ce, cei):
            d.free()
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
