"""Timing of the KZG proofs at every point of the domain -- sylow_hip_kzg_open_all_batch (kzg_open_all.hip) -- beside the two routes a caller
had before it existed, on device-resident arrays:
  (A) kzg_open_all_batch with the table of kzg_open_all_prepare, y_out = NULL;
  (B) the composed public route over the same table: sylow_hip_fr_ntt_batch of the zero-padded coefficients, sylow_hip_g1_scalar_mul_batch
      of the table by them, sylow_hip_g1_ntt_batch inverse over 2n points, the first n points of each array, sylow_hip_g1_ntt_batch forward.
      The padding and the table tiled m times are prepared outside the timed region; the transposes between the calls' layouts and the
      slice run through torch on the same stream, inside it;
  (C) sylow_hip_kzg_open_batch with the polynomial repeated n times at z_i = w^i, at the --c-shapes only (n^2 coefficients).
Every route's words are compared with (A)'s before anything is timed.  The table is built outside the timed region.  (A) must be faster
than (B) at the --gated shapes and than (C) at the --c-gated shapes by more than the two routes' combined spread.
The "SRS" is s_k G1gen for random s_k (the fixed-base call): all three routes are linear in the SRS points, so any points serve.
Device events around each call, warm-up calls first; the candidates ALTERNATE inside every repetition in one process, the median of --reps
is reported with its minimum and maximum.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_kzg_open_all.py [--warmup 1] [--reps 5] [--out profiles/kzg_open_all/bench_kzg_open_all.json]"""
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
from bench_msm import Timer  # noqa: E402


def multiplications(log_n):
    """per polynomial: 2n products, the stages p >= 1 of the inverse of 2n points and of the forward of n points"""
    n = 1 << log_n
    return 2 * n + (n * (log_n - 1) + 1) + ((n // 2) * (log_n - 2) + 1)


class Composed:
    """route (B): tensors on the device, the library's calls on their pointers, the layout changes through torch on the same stream"""

    def __init__(self, eng, timer, table, coeffs, log_n):
        import torch
        self.torch, self.eng, self.stream = torch, eng, timer.stream
        m, n = coeffs.shape[0], 1 << log_n
        self.m, self.n, self.log_n = m, n, log_n
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).cuda()
        txy, tinf = table
        self.t = dev(np.tile(txy, (1, m)))                                              # [8][m 2n]: entry i of array a at column a 2n + i
        self.ti = dev(np.tile(tinf, m))
        padded = np.zeros((m, 4, 2 * n), dtype=np.uint64)
        padded[:, :, :n] = coeffs
        self.padded = dev(padded)
        mk = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
        fl = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
        self.f, self.v, self.vi = mk(m, 4, 2 * n), mk(8, m * 2 * n), fl(m * 2 * n)
        self.h, self.hi = mk(m, 8, 2 * n), fl(m, 2 * n)
        self.o, self.oi = mk(m, 8, n), fl(m, n)

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {rc} {self.eng.lib.sylow_hip_last_error()}")

    def run(self):
        torch, lib, st, m, n, lg = self.torch, self.eng.lib, self.eng.stream, self.m, self.n, self.log_n
        with torch.cuda.stream(self.stream):
            self._chk(lib.sylow_hip_fr_ntt_batch(self.padded.data_ptr(), lg + 1, m, 0, None, self.f.data_ptr(), st), "fr_ntt")
            k = self.f if m == 1 else self.f.permute(1, 0, 2).contiguous()              # [4][m 2n]
            self._chk(lib.sylow_hip_g1_scalar_mul_batch(self.t.data_ptr(), self.ti.data_ptr(), k.data_ptr(), self.v.data_ptr(), self.vi.data_ptr(), m * 2 * n, st), "scalar_mul")
            vp = self.v if m == 1 else self.v.view(8, m, 2 * n).permute(1, 0, 2).contiguous()      # [m][8][2n]
            self._chk(lib.sylow_hip_g1_ntt_batch(vp.data_ptr(), self.vi.data_ptr(), lg + 1, m, 1, self.h.data_ptr(), self.hi.data_ptr(), st), "g1_ntt inverse")
            hs, his = self.h[:, :, :n].contiguous(), self.hi[:, :n].contiguous()
            self._chk(lib.sylow_hip_g1_ntt_batch(hs.data_ptr(), his.data_ptr(), lg, m, 0, self.o.data_ptr(), self.oi.data_ptr(), st), "g1_ntt forward")
            self.keep = (k, vp, hs, his)                                                # alive until the stream has used them

    def result(self):
        return self.o.cpu().numpy().view(np.uint64), self.oi.cpu().numpy()


class Repeated:
    """route (C): the polynomial n times, one opening per point of the domain; one polynomial (m = 1)"""

    def __init__(self, eng, srs, coeffs, log_n):
        n = 1 << log_n
        self.eng, self.n = eng, n
        x = np.zeros((n, 4), dtype=np.uint64)
        x[1 % n, 0] = 1
        self.dz = eng.to_device_soa(eng.fr_ntt(x), 4)                                   # w^i
        self.ds = eng.to_device_soa(srs, 8)
        self.dc = eng.to_device(np.ascontiguousarray(np.broadcast_to(coeffs[0], (n, 4, n))))
        self.dy, self.dp, self.dpi = eng.empty((4, n)), eng.empty((8, n)), eng.empty((n,), np.uint8)

    def run(self):
        self.eng._call("sylow_hip_kzg_open_batch", self.ds.ptr, self.dc.ptr, self.n, self.n, self.dz.ptr, self.dy.ptr, self.dp.ptr, self.dpi.ptr)

    def result(self):
        return self.dp.download()[None], self.dpi.download()[None]

    def free(self):
        for d in (self.dz, self.ds, self.dc, self.dy, self.dp, self.dpi):
            d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x10,1x12,1x16,16x12,1x20")
    ap.add_argument("--gated", default="1x16,16x12")
    ap.add_argument("--c-shapes", default="1x10,1x12")
    ap.add_argument("--c-gated", default="1x12")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    pairs = lambda s: [tuple(int(v) for v in p.split("x")) for p in s.split(",") if p]
    gated, c_shapes, c_gated = set(pairs(args.gated)), set(pairs(args.c_shapes)), set(pairs(args.c_gated))
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "rows": []}
    for m, lg in pairs(args.shapes):
        n = 1 << lg
        rng = np.random.default_rng(11 * m + lg)
        srs = points(eng, random_scalars(rng, n))
        coeffs = np.ascontiguousarray(random_scalars(rng, m * n).reshape(m, n, 4).transpose(0, 2, 1))      # [m][4][n]
        dt, dti = eng.kzg_open_all_prepare(srs)
        table = (dt.download(), dti.download())
        dc = eng.to_device(coeffs)
        dp, dpi = eng.empty((m, 8, n)), eng.empty((m, n), np.uint8)
        comp = Composed(eng, timer, table, coeffs, lg)
        rep = Repeated(eng, srs, coeffs, lg) if (m, lg) in c_shapes else None

        def open_all():
            eng._call("sylow_hip_kzg_open_all_batch", dt.ptr, dti.ptr, dc.ptr, lg, m, None, dp.ptr, dpi.ptr)

        # the same words first
        open_all()
        comp.run()
        eng.sync()
        axy, ainf = dp.download(), dpi.download()
        bxy, binf = comp.result()
        same = {"composed": bool(np.array_equal(axy, bxy) and np.array_equal(ainf, binf))}
        fns = [("open_all", open_all), ("composed", comp.run)]
        if rep:
            rep.run()
            eng.sync()
            cxy, cinf = rep.result()
            same["repeated"] = bool(np.array_equal(axy, cxy) and np.array_equal(ainf, cinf))
            fns.append(("repeated", rep.run))
        row = {"m": m, "log_n": lg, "same_words": same, **measure(timer, eng, fns, args.warmup, args.reps)}
        spread = lambda k: row[k + "_ms_max"] - row[k + "_ms_min"]
        for other, is_gated in (("composed", (m, lg) in gated),) + ((("repeated", (m, lg) in c_gated),) if rep else ()):
            both = spread("open_all") + spread(other)
            row[other + "_spread_ms"] = round(both, 4)
            row[other + "_over_open_all"] = round(row[other + "_ms"] / row["open_all_ms"], 3)
            row["faster_than_" + other] = bool(row["open_all_ms"] + both < row[other + "_ms"])
            row["gated_against_" + other] = is_gated
        mults = m * multiplications(lg)
        composed_mults = m * (2 * n + (n * (lg - 1) + 1) + 2 * n + ((n // 2) * (lg - 2) + 1))       # and the inverse's scale: one per point of 2n
        row["multiplications"] = {"open_all": mults, "composed": composed_mults, "repeated_terms": n * n if rep else None}
        row["us_per_multiplication"] = {"open_all": round(row["open_all_ms"] * 1e3 / mults, 4), "composed": round(row["composed_ms"] * 1e3 / composed_mults, 4)}
        out["rows"].append(row)
        for d in (dt, dti, dc, dp, dpi):
            d.free()
        if rep:
            rep.free()
        del comp
    ok = all(all(r["same_words"].values()) for r in out["rows"])
    for r in out["rows"]:
        for other in ("composed", "repeated"):
            if r.get("gated_against_" + other):
                ok = ok and r["faster_than_" + other]
    out["conditions_met"] = bool(ok)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
