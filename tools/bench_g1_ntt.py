"""Timing of the G1 transform -- sylow_hip_g1_ntt_batch (g1_ntt.hip) -- beside what a caller could compose before it existed and beside the
scalar-multiplication kernel it is built on:
  (a) g1_ntt_batch, forward and inverse, at (m, log_n) = (1, 12), (1, 16), (1, 20), (16, 12) (or --shapes);
  (b) the composed route on device-resident arrays, forward: per stage sylow_hip_g1_scalar_mul_batch of the second halves by the stage's
      twiddles (ones included: a batch call cannot skip them), then sylow_hip_g1_add_batch and sylow_hip_g1_sub_batch, then the stage's
      index permutation as a gather on the device.  Twiddle arrays and permutations are prepared outside the timed region.  Both routes
      must return the same words before anything is timed.  (a) must be faster than (b) at the --gated shapes, outside the spread;
  (c) ONE sylow_hip_g1_scalar_mul_batch over m n points with random scalars as the issue-rate yardstick: its time per point beside (a)'s
      time per scalar multiplication ((n / 2)(log_n - 2) + 1 per array, and n more for the inverse's scale).
Points are s_k G1gen for random s_k (the fixed-base call).  Device events around each call, warm-up calls first; the candidates ALTERNATE
inside every repetition in one process, the median of --reps is reported with its minimum and maximum.  Prints ONE JSON object and, with
--out, writes it.

    python tools/bench_g1_ntt.py [--warmup 1] [--reps 5] [--out profiles/g1_ntt/bench_g1_ntt.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_kzg_evals import measure  # noqa: E402
from bench_msm import Timer  # noqa: E402


def multiplications(log_n):
    half = (1 << log_n) >> 1
    return sum(half - (half >> p) for p in range(1, log_n))


def random_scalars(rng, n):
    s = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64, endpoint=False)
    s[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)                      # below r
    return s


def points(eng, s, step=1 << 16):
    parts = []
    for i in range(0, len(s), step):
        xy, inf = eng.g1_generator_mul(s[i:i + step])
        assert not inf.any()
        parts.append(xy)
    return np.concatenate(parts)


class Composed:
    """the route of (b): tensors on the device, the library's calls on their pointers, the gathers through torch on the same stream"""

    def __init__(self, eng, timer, pts, log_n):
        import torch
        self.torch, self.eng, self.stream = torch, eng, timer.stream
        m, n = pts.shape[0], 1 << log_n
        half = n // 2
        self.m, self.n, self.half, self.log_n = m, n, half, log_n
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
        soa = lambda a: dev(np.ascontiguousarray(a.reshape(-1, a.shape[-1]).T))
        self.a0, self.b0 = soa(pts[:, :half]), soa(pts[:, half:])                      # [8][m half]: point (array, j) at column array * half + j
        x = np.zeros((n, 4), dtype=np.uint64)
        x[1 % n, 0] = 1
        w = eng.fr_ntt(x)                                                               # w^i, i < n
        j = np.arange(half)
        self.tw, self.perm_a, self.perm_b = [], [], []
        for p in range(log_n):
            ns = 1 << p
            self.tw.append(soa(np.tile(w[(j % ns) * (n // (2 * ns))], (m, 1))))
            # [S | D] as columns (array, j) and m half + (array, j)  ->  natural order of the stage's output, split into halves again
            src = np.empty((m, n), dtype=np.int64)
            o = (j // ns) * 2 * ns + j % ns
            for a in range(m):
                src[a, o], src[a, o + ns] = a * half + j, m * half + a * half + j
            self.perm_a.append(dev(src[:, :half].reshape(-1)))
            self.perm_b.append(dev(src[:, half:].reshape(-1)))
        k = m * half
        mk = lambda rows: torch.empty((rows, k), dtype=torch.int64, device="cuda")
        self.v, self.sd = mk(8), torch.empty((8, 2 * k), dtype=torch.int64, device="cuda")
        self.s, self.d = mk(8), mk(8)
        flag = lambda: torch.zeros((k,), dtype=torch.uint8, device="cuda")
        self.vi, self.si, self.di = flag(), flag(), flag()
        self.sdi = torch.zeros((2 * k,), dtype=torch.uint8, device="cuda")
        self.out = None

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {rc} {self.eng.lib.sylow_hip_last_error()}")

    def run(self):
        torch, lib, st, k = self.torch, self.eng.lib, self.eng.stream, self.m * self.half
        a, b, ai, bi = self.a0, self.b0, None, None
        with torch.cuda.stream(self.stream):
            for p in range(self.log_n):
                pa, pb = (None if ai is None else ai.data_ptr()), (None if bi is None else bi.data_ptr())
                self._chk(lib.sylow_hip_g1_scalar_mul_batch(b.data_ptr(), pb, self.tw[p].data_ptr(), self.v.data_ptr(), self.vi.data_ptr(), k, st), "scalar_mul")
                self._chk(lib.sylow_hip_g1_add_batch(a.data_ptr(), pa, self.v.data_ptr(), self.vi.data_ptr(), self.s.data_ptr(), self.si.data_ptr(), k, st), "add")
                self._chk(lib.sylow_hip_g1_sub_batch(a.data_ptr(), pa, self.v.data_ptr(), self.vi.data_ptr(), self.d.data_ptr(), self.di.data_ptr(), k, st), "sub")
                torch.cat([self.s, self.d], dim=1, out=self.sd)
                torch.cat([self.si, self.di], out=self.sdi)
                a, b = self.sd.index_select(1, self.perm_a[p]), self.sd.index_select(1, self.perm_b[p])
                ai, bi = self.sdi.index_select(0, self.perm_a[p]), self.sdi.index_select(0, self.perm_b[p])
            self.out = (a, b, ai, bi)

    def result(self):
        """([m, n, 8] words, [m, n] flags) of the last run"""
        a, b, ai, bi = [t.cpu().numpy() for t in self.out]
        m, half = self.m, self.half
        xy = np.concatenate([a.view(np.uint64).T.reshape(m, half, 8), b.view(np.uint64).T.reshape(m, half, 8)], axis=1)
        return xy, np.concatenate([ai.reshape(m, half), bi.reshape(m, half)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x12,1x16,1x20,16x12")
    ap.add_argument("--gated", default="1x16,1x20")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    pairs = lambda s: [tuple(int(v) for v in p.split("x")) for p in s.split(",") if p]
    gated = set(pairs(args.gated))
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "rows": []}
    for m, lg in pairs(args.shapes):
        n = 1 << lg
        rng = np.random.default_rng(7 * m + lg)
        pts = points(eng, random_scalars(rng, m * n)).reshape(m, n, 8)
        din = eng.to_device(np.ascontiguousarray(pts.transpose(0, 2, 1)))              # [m][8][n]
        do, doi = eng.empty((m, 8, n)), eng.empty((m, n), np.uint8)
        dk = eng.to_device_soa(random_scalars(rng, m * n), 4)
        dp = eng.to_device_soa(pts.reshape(-1, 8), 8)
        dmo, dmi = eng.empty((8, m * n)), eng.empty((m * n,), np.uint8)
        comp = Composed(eng, timer, pts, lg)

        def forward():
            eng._call("sylow_hip_g1_ntt_batch", din.ptr, None, lg, m, 0, do.ptr, doi.ptr)

        def inverse():
            eng._call("sylow_hip_g1_ntt_batch", din.ptr, None, lg, m, 1, do.ptr, doi.ptr)

        def scalar_mul():
            eng._call("sylow_hip_g1_scalar_mul_batch", dp.ptr, None, dk.ptr, dmo.ptr, dmi.ptr, m * n)

        # the same words first
        forward()
        comp.run()
        eng.sync()
        cxy, cinf = comp.result()
        same = bool(np.array_equal(np.ascontiguousarray(do.download().transpose(0, 2, 1)), cxy) and np.array_equal(doi.download(), cinf))
        fns = (("g1_ntt_forward", forward), ("composed_forward", comp.run), ("g1_ntt_inverse", inverse), ("scalar_mul", scalar_mul))
        row = {"m": m, "log_n": lg, "same_words": same, **measure(timer, eng, fns, args.warmup, args.reps)}
        spread = max(row[k + "_ms_max"] - row[k + "_ms_min"] for k in ("g1_ntt_forward", "composed_forward"))
        row["spread_ms"] = round(spread, 4)
        row["composed_over_g1_ntt"] = round(row["composed_forward_ms"] / row["g1_ntt_forward_ms"], 3)
        row["gated"] = (m, lg) in gated
        row["g1_ntt_faster"] = bool(row["g1_ntt_forward_ms"] + spread < row["composed_forward_ms"])
        mults = m * multiplications(lg)
        row["multiplications"] = {"forward": mults, "inverse": mults + m * n, "composed": m * (n // 2) * lg, "scalar_mul": m * n}
        row["us_per_multiplication"] = {"g1_ntt_forward": round(row["g1_ntt_forward_ms"] * 1e3 / max(mults, 1), 4),
                                        "g1_ntt_inverse": round(row["g1_ntt_inverse_ms"] * 1e3 / (mults + m * n), 4),
                                        "composed_forward": round(row["composed_forward_ms"] * 1e3 / (m * (n // 2) * lg), 4),
                                        "scalar_mul": round(row["scalar_mul_ms"] * 1e3 / (m * n), 4)}
        out["rows"].append(row)
        for d in (din, do, doi, dk, dp, dmo, dmi):
            d.free()
        del comp
    out["conditions_met"] = bool(all(r["same_words"] for r in out["rows"]) and all(r["g1_ntt_faster"] for r in out["rows"] if r["gated"]))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
