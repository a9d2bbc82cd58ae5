"""Timing of the KZG proofs on every coset of the domain -- sylow_hip_kzg_open_cosets_batch (kzg_cosets.hip) -- beside the two routes a caller
had before it existed, on device-resident arrays.  A shape is m x log_c x log_l: m polynomials, c = 2^log_c cosets of
l = 2^log_l points.
  (A) kzg_open_cosets_batch with the table of kzg_open_cosets_prepare, y_out = NULL;
  (B) the composed public route over the same table: the split into l residue arrays padded to 2c, sylow_hip_fr_ntt_batch of the m l
      arrays, sylow_hip_g1_lincomb_batch with 2c m jobs of l terms (table entry times transformed coefficient, summed over the residues),
      sylow_hip_g1_ntt_batch inverse over 2c points, the first c points of each array, sylow_hip_g1_ntt_batch forward.  The table laid out
      term-major and tiled m times is prepared outside the timed region; the split, the transposes between the calls' layouts and the slice
      run through torch on the same stream, inside it;
  (C) sylow_hip_kzg_open_points_batch with the polynomial repeated c times, z = the points of each coset, at the --c-shapes only (m = 1,
      l <= 64: c n coefficients).
Every route's words are compared with (A)'s before anything is timed.  The table is built outside the timed region.  (A) must be faster
than (C) at the --c-gated shapes by more than the two routes' combined min - max spreads; (A) against (B) is recorded, not gated.
The "SRS" is s_k G1gen for random s_k (the fixed-base call): all three routes are linear in the SRS points, so any points serve.
Device events around each call, warm-up calls first; the candidates ALTERNATE inside every repetition in one process, the median of --reps
is reported with its minimum and maximum.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_kzg_cosets.py [--warmup 1] [--reps 5] [--out profiles/kzg_cosets/bench_kzg_cosets.json]"""
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


def stage_multiplications(log_n):
    """the stages p >= 1 of a transform of 2^log_n points: sum of (n / 2)(1 - 2^-p)"""
    half = (1 << log_n) >> 1
    return sum(half - (half >> p) for p in range(1, log_n))


def multiplications(log_c, log_l):
    """per polynomial: 2n products, the stages p >= 1 of the inverse of 2c points and of the forward of c points"""
    return (2 << (log_c + log_l)) + stage_multiplications(log_c + 1) + stage_multiplications(log_c)


def default_planes_log(log_c, log_l, m, resident=512 * 256):
    p = 0
    while p < log_l and ((m << log_c) << p) < resident:
        p += 1
    return p


class Composed:
    """route (B): tensors on the device, the library's calls on their pointers, the layout changes through torch on the same stream"""

    def __init__(self, eng, timer, table, coeffs, log_c, log_l):
        import torch
        self.torch, self.eng, self.stream = torch, eng, timer.stream
        m, c, l = coeffs.shape[0], 1 << log_c, 1 << log_l
        self.m, self.c, self.l, self.log_c = m, c, l, log_c
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).cuda()
        txy, tinf = table                                                               # [l][8][2c], [l][2c]
        # term-major for the linear combinations: (job A 2c + k, term a) at index a (2c m) + A 2c + k
        self.t = dev(np.ascontiguousarray(np.broadcast_to(txy.transpose(1, 0, 2)[:, :, None, :], (8, l, m, 2 * c))).reshape(8, -1))
        self.ti = dev(np.ascontiguousarray(np.broadcast_to(tinf[:, None, :], (l, m, 2 * c))).reshape(-1))
        self.coeffs = dev(coeffs)                                                       # [m][4][n]
        mk = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")
        fl = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")
        self.f = mk(m * l, 4, 2 * c)
        self.v, self.vi = mk(8, m * 2 * c), fl(m * 2 * c)
        self.h, self.hi = mk(m, 8, 2 * c), fl(m, 2 * c)
        self.o, self.oi = mk(m, 8, c), fl(m, c)

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {rc} {self.eng.lib.sylow_hip_last_error()}")

    def run(self):
        torch, lib, st, m, c, l, lg = self.torch, self.eng.lib, self.eng.stream, self.m, self.c, self.l, self.log_c
        with torch.cuda.stream(self.stream):
            padded = torch.zeros((m * l, 4, 2 * c), dtype=torch.int64, device="cuda")
            padded[:, :, :c] = self.coeffs.view(m, 4, c, l).permute(0, 3, 1, 2).reshape(m * l, 4, c)      # row A l + a holds f_(a + l j), j < c
            self._chk(lib.sylow_hip_fr_ntt_batch(padded.data_ptr(), lg + 1, m * l, 0, None, self.f.data_ptr(), st), "fr_ntt")
            k = self.f.view(m, l, 4, 2 * c).permute(2, 1, 0, 3).contiguous()            # [4][l][m][2c]: term-major
            self._chk(lib.sylow_hip_g1_lincomb_batch(self.t.data_ptr(), self.ti.data_ptr(), k.data_ptr(), self.v.data_ptr(), self.vi.data_ptr(), m * 2 * c, l, st), "lincomb")
            vp = self.v if m == 1 else self.v.view(8, m, 2 * c).permute(1, 0, 2).contiguous()              # [m][8][2c]
            self._chk(lib.sylow_hip_g1_ntt_batch(vp.data_ptr(), self.vi.data_ptr(), lg + 1, m, 1, self.h.data_ptr(), self.hi.data_ptr(), st), "g1_ntt inverse")
            hs, his = self.h[:, :, :c].contiguous(), self.hi[:, :c].contiguous()
            if c > 1:                                                                   # h_(c-1) is the identity by construction; the transform reads it as it is
                self._chk(lib.sylow_hip_g1_ntt_batch(hs.data_ptr(), his.data_ptr(), lg, m, 0, self.o.data_ptr(), self.oi.data_ptr(), st), "g1_ntt forward")
            self.keep = (padded, k, vp, hs, his)                                        # alive until the stream has used them

    def result(self):
        return self.o.cpu().numpy().view(np.uint64), self.oi.cpu().numpy()


class Repeated:
    """route (C): the polynomial c times, one several-point opening per coset; one polynomial (m = 1), l <= 64"""

    def __init__(self, eng, srs, coeffs, log_c, log_l):
        c, l, n = 1 << log_c, 1 << log_l, 1 << (log_c + log_l)
        self.eng, self.c, self.l, self.n = eng, c, l, n
        x = np.zeros((n, 4), dtype=np.uint64)
        x[1 % n, 0] = 1
        w = eng.fr_ntt(x)                                                               # w^i
        idx = (np.arange(c)[:, None] + c * np.arange(l)[None, :]).reshape(-1)           # (coset i, point j) at i l + j: w^(i + c j)
        self.dz = eng.to_device_soa(w[idx], 4)
        self.ds = eng.to_device_soa(srs, 8)
        self.dc = eng.to_device(np.ascontiguousarray(np.broadcast_to(coeffs[0], (c, 4, n))))
        self.dy, self.dp, self.dpi = eng.empty((4, c * l)), eng.empty((8, c)), eng.empty((c,), np.uint8)

    def run(self):
        self.eng._call("sylow_hip_kzg_open_points_batch", self.ds.ptr, self.dc.ptr, self.n, self.c, self.dz.ptr, self.l, self.dy.ptr, self.dp.ptr, self.dpi.ptr)

    def result(self):
        return self.dp.download()[None], self.dpi.download()[None]

    def free(self):
        for d in (self.dz, self.ds, self.dc, self.dy, self.dp, self.dpi):
            d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x10x4,1x8x4,1x12x4,16x8x4,1x12x6,1x6x4")
    ap.add_argument("--c-shapes", default="1x10x4,1x6x4")
    ap.add_argument("--c-gated", default="1x10x4")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    triples = lambda s: [tuple(int(v) for v in p.split("x")) for p in s.split(",") if p]
    c_shapes, c_gated = set(triples(args.c_shapes)), set(triples(args.c_gated))
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "rows": []}
    for m, lc, ll in triples(args.shapes):
        n, c, l = 1 << (lc + ll), 1 << lc, 1 << ll
        rng = np.random.default_rng(11 * m + 101 * lc + ll)
        srs = points(eng, random_scalars(rng, n))
        coeffs = np.ascontiguousarray(random_scalars(rng, m * n).reshape(m, n, 4).transpose(0, 2, 1))      # [m][4][n]
        dt, dti = eng.kzg_open_cosets_prepare(srs, ll)
        table = (dt.download(), dti.download())
        dc = eng.to_device(coeffs)
        dp, dpi = eng.empty((m, 8, c)), eng.empty((m, c), np.uint8)
        comp = Composed(eng, timer, table, coeffs, lc, ll)
        rep = Repeated(eng, srs, coeffs, lc, ll) if (m, lc, ll) in c_shapes else None

        def open_cosets():
            eng._call("sylow_hip_kzg_open_cosets_batch", dt.ptr, dti.ptr, dc.ptr, lc, ll, m, None, dp.ptr, dpi.ptr)

        # the same words first
        open_cosets()
        comp.run()
        eng.sync()
        axy, ainf = dp.download(), dpi.download()
        bxy, binf = comp.result()
        same = {"composed": bool(np.array_equal(axy, bxy) and np.array_equal(ainf, binf))}
        fns = [("open_cosets", open_cosets), ("composed", comp.run)]
        if rep:
            rep.run()
            eng.sync()
            cxy, cinf = rep.result()
            same["repeated"] = bool(np.array_equal(axy, cxy) and np.array_equal(ainf, cinf))
            fns.append(("repeated", rep.run))
        row = {"m": m, "log_c": lc, "log_l": ll, "planes_log": default_planes_log(lc, ll, m), "same_words": same}
        if all(same.values()):                                      # nothing is timed before every candidate has returned (A)'s words
            row.update(measure(timer, eng, fns, args.warmup, args.reps))
            spread = lambda k: row[k + "_ms_max"] - row[k + "_ms_min"]
            for other, is_gated in (("composed", False),) + ((("repeated", (m, lc, ll) in c_gated),) if rep else ()):
                both = spread("open_cosets") + spread(other)
                row[other + "_spread_ms"] = round(both, 4)
                row[other + "_over_open_cosets"] = round(row[other + "_ms"] / row["open_cosets_ms"], 3)
                row["faster_than_" + other] = bool(row["open_cosets_ms"] + both < row[other + "_ms"])
                row["gated_against_" + other] = is_gated
            mults = m * multiplications(lc, ll)
            composed_mults = mults + m * 2 * c                       # and the inverse's scale: one per point of 2c
            row["multiplications"] = {"open_cosets": mults, "composed": composed_mults, "repeated_terms": c * n if rep else None}
            row["us_per_multiplication"] = {"open_cosets": round(row["open_cosets_ms"] * 1e3 / mults, 4), "composed": round(row["composed_ms"] * 1e3 / composed_mults, 4)}
        out["rows"].append(row)
        for d in (dt, dti, dc, dp, dpi):
            d.free()
        if rep:
            rep.free()
        del comp
    ok = all(all(r["same_words"].values()) for r in out["rows"])
    for r in out["rows"]:
        if r.get("gated_against_repeated"):
            ok = ok and r["faster_than_repeated"]
    out["conditions_met"] = bool(ok)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
