"""Timing of the recovery of a KZG polynomial from half of its cells -- sylow_hip_kzg_recover_batch (kzg_recover.hip) -- beside the floor of
its own transforms and the composition a caller had before it existed, on device-resident arrays.  A shape is
m x log_c x log_l: m blobs of c = 2^log_c cells of l = 2^log_l values, each with its own random half of the cells missing.
  (A) kzg_recover_batch with y_out = NULL, and (A') with y_out;
  (F) the floor: the sylow_hip_fr_ntt_batch calls the route makes, on buffers of the same size and nothing else -- inverse, forward with
      shift 5, inverse with shift 5 (three; a fourth, forward, for A');
  (B) the composed public route: per row the c values of Z on the domain and on the coset from Python integers ON THE HOST, tiled to n
      and uploaded; sylow_hip_fr_mul_batch per row; the inverse and the shifted forward transform of the batch; sylow_hip_fr_batch_inv of
      the n coset values and sylow_hip_fr_mul_batch per row; the shifted inverse transform.  The host work and the uploads are inside the
      timed region: they repeat for every set of missing cells.
(B)'s words are compared with (A)'s before anything is timed.  Device events around each call, warm-up calls first; the candidates
ALTERNATE inside every repetition in one process, the median of --reps is reported with its minimum and maximum.  Prints ONE JSON object
and, with --out, writes it.

    python tools/bench_kzg_recover.py [--warmup 2] [--reps 7] [--out profiles/kzg_recover/bench_kzg_recover.json]"""
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
S = 5


def omega(log_n):
    return pow(pow(5, (R - 1) >> 28, R), 1 << (28 - log_n), R)


def words(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for k in range(4):
        out[:, k] = np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)
    return out


def host_vanish(present, log_c, log_l):
    """what a caller computes per row without the library: the c values of Z on the domain and on the coset, Python integers"""
    c = 1 << log_c
    v, sl = pow(omega(log_c + log_l), 1 << log_l, R), pow(S, 1 << log_l, R)
    vp = [1] * c
    for k in range(1, c):
        vp[k] = vp[k - 1] * v % R
    miss = [vp[i] for i in range(c) if not present[i]]
    zd, zc = [], []
    for k in range(c):
        a, b, pd, pc = vp[k], sl * vp[k] % R, 1, 1
        for x in miss:
            pd, pc = pd * (a - x) % R, pc * (b - x) % R
        zd.append(pd)
        zc.append(pc)
    return zd, zc


class Composed:
    """route (B) on the engine's own arrays"""

    def __init__(self, eng, dy, present, log_c, log_l):
        self.eng, self.dy, self.present, self.log_c, self.log_l = eng, dy, present, log_c, log_l
        m, n = present.shape[0], 1 << (log_c + log_l)
        self.m, self.n = m, n
        self.t, self.p, self.zci = eng.empty((m, 4, n)), eng.empty((m, 4, n)), eng.empty((m, 4, n))
        self.shift = eng.to_device(np.array([S, 0, 0, 0], dtype=np.uint64))

    def run(self):
        eng, m, n, L = self.eng, self.m, self.n, self.log_c + self.log_l
        l = 1 << self.log_l
        zd, zc = np.empty((m, 4, n), dtype=np.uint64), np.empty((m, 4, n), dtype=np.uint64)
        for j in range(m):
            d, c = host_vanish(self.present[j], self.log_c, self.log_l)
            zd[j], zc[j] = np.tile(words(d).T, (1, l)), np.tile(words(c).T, (1, l))          # element i + c t holds value i
        dzd, dzc = eng.to_device(zd), eng.to_device(zc)
        row = 32 * n
        for j in range(m):
            eng._call("sylow_hip_fr_mul_batch", self.dy.ptr + j * row, dzd.ptr + j * row, self.t.ptr + j * row, n)
            eng._call("sylow_hip_fr_batch_inv", dzc.ptr + j * row, self.zci.ptr + j * row, n)
        eng._call("sylow_hip_fr_ntt_batch", self.t.ptr, L, m, 1, None, self.p.ptr)
        eng._call("sylow_hip_fr_ntt_batch", self.p.ptr, L, m, 0, self.shift.ptr, self.t.ptr)
        for j in range(m):
            eng._call("sylow_hip_fr_mul_batch", self.t.ptr + j * row, self.zci.ptr + j * row, self.p.ptr + j * row, n)
        eng._call("sylow_hip_fr_ntt_batch", self.p.ptr, L, m, 1, self.shift.ptr, self.t.ptr)
        self.keep = (dzd, dzc)                                                              # alive until the stream has used them

    def result(self):
        return self.t.download()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x7x6,64x7x6,1x10x10")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "rows": []}
    for m, lc, ll in [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",") if p]:
        n, c, L = 1 << (lc + ll), 1 << lc, lc + ll
        rng = np.random.default_rng(13 * m + 101 * lc + ll)
        coeffs = random_scalars(rng, m * n).reshape(m, n, 4)
        coeffs[:, n // 2:] = 0                                                              # blobs: degree below n / 2
        y = np.ascontiguousarray(eng.fr_ntt(coeffs).transpose(0, 2, 1))                     # [m][4][n]
        present = np.ones((m, c), dtype=np.uint8)
        for j in range(m):
            present[j, rng.permutation(c)[:c // 2]] = 0
        dy, dp = eng.to_device(y), eng.to_device(present)
        dc, dyo, ds = eng.empty((m, 4, n)), eng.empty((m, 4, n)), eng.empty((m,), np.uint8)
        fa, fb = eng.empty((m, 4, n)), eng.empty((m, 4, n))
        shift = eng.to_device(np.array([S, 0, 0, 0], dtype=np.uint64))
        comp = Composed(eng, dy, present, lc, ll)

        def recover():
            eng._call("sylow_hip_kzg_recover_batch", dy.ptr, dp.ptr, lc, ll, m, dc.ptr, None, ds.ptr)

        def recover_y():
            eng._call("sylow_hip_kzg_recover_batch", dy.ptr, dp.ptr, lc, ll, m, dc.ptr, dyo.ptr, ds.ptr)

        def floor():
            eng._call("sylow_hip_fr_ntt_batch", dy.ptr, L, m, 1, None, fa.ptr)
            eng._call("sylow_hip_fr_ntt_batch", fa.ptr, L, m, 0, shift.ptr, fb.ptr)
            eng._call("sylow_hip_fr_ntt_batch", fb.ptr, L, m, 1, shift.ptr, fa.ptr)

        def floor_y():
            floor()
            eng._call("sylow_hip_fr_ntt_batch", fa.ptr, L, m, 0, None, fb.ptr)

        recover_y()
        comp.run()
        eng.sync()
        got, status, back = dc.download(), ds.download(), dyo.download()
        same = {"blob": bool(np.array_equal(got.transpose(0, 2, 1), coeffs) and not status.any() and np.array_equal(back, y)),
                "composed": bool(np.array_equal(got, comp.result()))}
        row = {"m": m, "log_c": lc, "log_l": ll, "missing_per_row": c // 2, "same_words": same}
        if all(same.values()):                                      # nothing is timed before every candidate has returned the same words
            fns = [("recover", recover), ("floor", floor), ("recover_y", recover_y), ("floor_y", floor_y), ("composed", comp.run)]
            row.update(measure(timer, eng, fns, args.warmup, args.reps))
            row["recover_over_floor"] = round(row["recover_ms"] / row["floor_ms"], 3)
            row["recover_y_over_floor_y"] = round(row["recover_y_ms"] / row["floor_y_ms"], 3)
            row["composed_over_recover"] = round(row["composed_ms"] / row["recover_ms"], 3)
            row["vanish_products"] = 2 * c * (c // 2) * m
        out["rows"].append(row)
        for d in (dy, dp, dc, dyo, ds, fa, fb, shift, comp.t, comp.p, comp.zci, comp.shift):
            d.free()
        del comp
    out["conditions_met"] = bool(all(all(r["same_words"].values()) for r in out["rows"]))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
