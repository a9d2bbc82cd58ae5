"""Timing of the three Groth16 calls -- sylow_hip_groth16_vk_x_batch, sylow_hip_groth16_verify_batch, sylow_hip_groth16_batch_verify_weighted --
against the COMPOSED route a host had before them, built from older entry points only: sylow_hip_g1_lincomb_batch on the IC bases replicated
n times (scalar 1 for IC_0) and sylow_hip_multi_pairing_batch on the 4 n literal pairs (-A_i, B_i), (alpha, beta), (vk_x_i, gamma), (C_i, delta)
with beta, gamma, delta replicated.  n = 2^10, 2^14, 2^16 and l = 2, 16 public inputs (or --sizes / --inputs).  Proofs are valid: a pool of
256 made in Fr (generator multiples through sylow_hip_g1/g2_generator_mul_batch), tiled to n.  Device events around each call, warm-up
calls first; the routes ALTERNATE inside every repetition (new, composed, new, ...) in one process, the median of --reps is reported.  The
composed route's pair arrays are prepared outside the timed region, vk_x column included, so its figure is lincomb + multi_pairing and
nothing else.  Every row checks that all routes accept every proof.  Prints ONE JSON object.

    python tools/bench_groth16.py [--sizes 10,14,16] [--inputs 2,16] [--warmup 2] [--reps 5]"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_msm import Timer  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
POOL = 256


def limbs(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


def ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(r[k]) << (64 * k) for k in range(4)) for r in a]


def make_pool(eng, l, seed):
    """POOL valid proofs with l inputs under one key: (vk arrays, a, b, c, inputs [POOL, l] ints)"""
    rng = random.Random(seed)
    fr = lambda: rng.randrange(1, R)
    alpha, beta, gamma, delta = fr(), fr(), fr(), fr()
    ic = [fr() for _ in range(l + 1)]
    a, b = [fr() for _ in range(POOL)], [fr() for _ in range(POOL)]
    x = [[fr() for _ in range(l)] for _ in range(POOL)]
    inv_delta = pow(delta, R - 2, R)
    c = [(a[i] * b[i] - alpha * beta - (ic[0] + sum(v * w for v, w in zip(x[i], ic[1:]))) * gamma) * inv_delta % R for i in range(POOL)]
    g1 = lambda ks: eng.g1_generator_mul(limbs(ks))[0]
    g2 = lambda ks: eng.g2_generator_mul(limbs(ks))[0]
    return (g1([alpha]), g2([beta]), g2([gamma]), g2([delta]), g1(ic)), g1(a), g2(b), g1(c), x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,16")
    ap.add_argument("--inputs", default="2,16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "rows": []}
    for l in [int(v) for v in args.inputs.split(",")]:
        vk, pa, pb, pc, px = make_pool(eng, l, 20261018 + l)
        d_vk = [eng.to_device_soa(v, v.shape[1]) for v in vk]
        for lg in [int(v) for v in args.sizes.split(",")]:
            n = 1 << lg
            idx = np.arange(n) % POOL
            a, b, c = pa[idx], pb[idx], pc[idx]
            xw = limbs([v for row in px for v in row]).reshape(POOL, l, 4)[idx]                      # [n, l, 4]
            da, db, dc = eng.to_device_soa(a, 8), eng.to_device_soa(b, 16), eng.to_device_soa(c, 8)
            dx = eng.to_device_soa(np.ascontiguousarray(xw.transpose(1, 0, 2)).reshape(l * n, 4), 4)
            rng = np.random.default_rng(lg)
            w = np.zeros((n, 4), dtype=np.uint64)
            w[:, 0] = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
            dw = eng.to_device_soa(w, 4)
            vkx, vkxi = eng.empty((8, n)), eng.empty((n,), np.uint8)
            ok_new, ok_old = eng.empty((n,), np.uint8), eng.empty((n,), np.uint8)
            gt, one = eng.empty((48, 1)), eng.empty((1,), np.uint8)
            # the composed route's operands: replicated bases + scalars (term-major), replicated pairs (job-major)
            d_bases = eng.to_device_soa(np.repeat(vk[4], n, 0), 8)
            d_k = eng.to_device_soa(np.concatenate([limbs([1] * n), np.ascontiguousarray(xw.transpose(1, 0, 2)).reshape(l * n, 4)]), 4)
            lc, lci = eng.empty((8, n)), eng.empty((n,), np.uint8)

            def vk_x():
                eng._call("sylow_hip_groth16_vk_x_batch", d_vk[4].ptr, l, dx.ptr, n, vkx.ptr, vkxi.ptr)

            def lincomb():
                eng._call("sylow_hip_g1_lincomb_batch", d_bases.ptr, None, d_k.ptr, lc.ptr, lci.ptr, n, l + 1)

            vk_x()
            lincomb()
            vx = eng.from_device_soa(vkx)
            same_vk_x = bool(np.array_equal(vx, eng.from_device_soa(lc)))
            na = a.copy()
            na[:, 4:8] = limbs([(P - v) % P for v in ints(a[:, 4:8])])
            pp = np.zeros((n, 4, 8), dtype=np.uint64)
            qq = np.zeros((n, 4, 16), dtype=np.uint64)
            pp[:, 0], pp[:, 1], pp[:, 2], pp[:, 3] = na, vk[0][0], vx, c
            qq[:, 0], qq[:, 1], qq[:, 2], qq[:, 3] = b, vk[1][0], vk[2][0], vk[3][0]
            d_pp, d_qq = eng.to_device_soa(pp.reshape(4 * n, 8), 8), eng.to_device_soa(qq.reshape(4 * n, 16), 16)
            d_off = eng.to_device(np.arange(n + 1, dtype=np.uint64) * np.uint64(4))

            def pairs_old():
                eng._call("sylow_hip_multi_pairing_batch", d_pp.ptr, None, d_qq.ptr, None, d_off.ptr, n, 4 * n, 1, None, ok_old.ptr)

            def composed():
                lincomb()
                pairs_old()

            def verify():
                eng._call("sylow_hip_groth16_verify_batch", d_vk[0].ptr, d_vk[1].ptr, d_vk[2].ptr, d_vk[3].ptr, d_vk[4].ptr, l, da.ptr, None, db.ptr, None,
                          dc.ptr, None, dx.ptr, n, ok_new.ptr)

            def weighted():
                eng._call("sylow_hip_groth16_batch_verify_weighted", d_vk[0].ptr, d_vk[1].ptr, d_vk[2].ptr, d_vk[3].ptr, d_vk[4].ptr, l, da.ptr, None, db.ptr,
                          None, dc.ptr, None, dx.ptr, dw.ptr, n, gt.ptr, one.ptr)

            fns = (("vk_x", vk_x), ("lincomb", lincomb), ("verify", verify), ("composed", composed), ("weighted", weighted))
            for _ in range(args.warmup):
                for _, fn in fns:
                    fn()
            eng.sync()
            res = {name: [] for name, _ in fns}
            for _ in range(args.reps):                                   # the routes alternate inside every repetition
                for name, fn in fns:
                    res[name].append(timer.time_ms(fn))
            row = {"n": n, "n_inputs": l}
            for name, v in res.items():
                v = sorted(v)
                row[name + "_ms"] = round(v[len(v) // 2], 4)
                row[name + "_ms_min"], row[name + "_ms_max"] = round(v[0], 4), round(v[-1], 4)
            row["vk_x_speedup"] = round(row["lincomb_ms"] / row["vk_x_ms"], 2)
            row["verify_speedup"] = round(row["composed_ms"] / row["verify_ms"], 2)
            row["weighted_vs_n_proofs"] = round(row["verify_ms"] / row["weighted_ms"], 2)
            row["proofs_per_s"] = {"verify": round(n / row["verify_ms"] * 1e3), "composed": round(n / row["composed_ms"] * 1e3),
                                   "weighted": round(n / row["weighted_ms"] * 1e3)}
            row["same_vk_x"] = same_vk_x
            row["all_ok"] = [bool(ok_new.download().all()), bool(ok_old.download().all()), bool(one.download()[0])]
            out["rows"].append(row)
            for d in (da, db, dc, dx, dw, vkx, vkxi, ok_new, ok_old, gt, one, d_bases, d_k, lc, lci, d_pp, d_qq, d_off):
                d.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
