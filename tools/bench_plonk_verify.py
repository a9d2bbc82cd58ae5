"""Timing of the batched PLONK verifier -- sylow_pverify_verify_batch and sylow_pverify_batch_verify_weighted (plonk_verify.hip, DESIGN.md
§4.22) -- on device-resident arrays, beside the same flags composed on the surface the library had before, on the same box in the same run.
A shape is m proofs of one circuit (W = 3 wire columns, E = 4 chunks of t, n_pub = 4 public inputs, log_n = 16; T = 18 terms):
  (S)  sylow_pverify_scalars_batch: the denominators, their shared inversion, the lane-per-proof pass;
  (F)  sylow_pverify_fold_batch: (S), the gather, sylow_hip_g1_lincomb_batch twice, the scatter;
  (V)  sylow_pverify_verify_batch: (F), sylow_hip_kzg_verify_batch over the rows (C, 0, y, pi), the veto;
  (W)  sylow_pverify_batch_verify_weighted: the scalars, the weighted prep and join, two multi-scalar multiplications, the pairing product;
  (L)  the two sylow_hip_g1_lincomb_batch calls alone, over term-major bases packed beforehand;  (K) sylow_hip_kzg_verify_batch alone;
  (C)  the composition (L) + (K): what a caller had before.  In its favour and outside its window: the T m scalars, y and the term-major
       bases with the key replicated m times are handed to it for nothing.  It is a FLOOR the new call cannot beat: (V) runs the same two
       calls after forming their inputs.
The scalars handed to (C) are those of (S), which tests/test_gpu_plonk_verify.py pins word for word to the integer model; the first proofs
are checked against tests/plonk_verify_model.py here as well.  The points are random points of G1, not valid proofs: the work does not
depend on what the flags come out as, and (C) must give the flags of (V), byte for byte, before anything is timed.  Device events around
each call, warm-up calls first; the candidates ALTERNATE inside every repetition in one process, the median of --reps is reported with its
minimum and maximum.  new_kernels_ms = (F) - (L): the scalars, the gather and the scatter.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_plonk_verify.py [--sizes 10,14,16] [--warmup 2] [--reps 7] [--out profiles/plonk_verify/bench_plonk_verify.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_plonk_verify.py --sizes 14 --warmup 0 --reps 1 --only-verify"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_g1_ntt import points, random_scalars  # noqa: E402
from bench_kzg_evals import measure  # noqa: E402
from bench_msm import Timer, words_to_ints  # noqa: E402

WIRES, LOG_E, LOG_N, PUBLIC = 3, 2, 16, 4
POOL = 1 << 12                      # distinct random points; the arrays tile them


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,16", help="log2 of the batch sizes m")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-verify", action="store_true", help="run (V) alone, warmup + reps times, and time nothing: for a kernel-trace run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    W, E = WIRES, 1 << LOG_E
    K, P = 2 * W + 2, W + E + 3
    T = K + P
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "wires": W, "log_e": LOG_E, "log_n": LOG_N, "n_pub": PUBLIC, "terms": T, "rows": []}
    rng = np.random.default_rng(20261020)
    pool = points(eng, random_scalars(rng, POOL))
    tau = eng.to_device_soa(eng.g2_generator_mul(random_scalars(rng, 1))[0], 16)
    vk = pool[:K]
    dvk = eng.to_device_soa(vk, 8)
    shifts = np.zeros((W, 4), dtype=np.uint64)
    shifts[:, 0] = [1, 5, 7]
    dsh = eng.to_device_soa(shifts, 4)
    for lg in [int(x) for x in args.sizes.split(",") if x]:
        m = 1 << lg
        proofs = pool[(np.arange(P * m) * 7 + 11) % POOL]                    # slot-major: slot c of proof i at c m + i
        dpr = eng.to_device_soa(proofs, 8)
        ev, pub = random_scalars(rng, (2 * W + 1) * m), random_scalars(rng, PUBLIC * m)
        dev, dpub = eng.to_device_soa(ev, 4), eng.to_device_soa(pub, 4)
        ch = [random_scalars(rng, m) for _ in range(7)]                      # beta, gamma, alpha, zeta, v, u, weights
        dch = [eng.to_device_soa(x, 4) for x in ch]
        ins = [dev.ptr, dpub.ptr, PUBLIC, dsh.ptr] + [d.ptr for d in dch[:6]]
        pts = [dvk.ptr, None, dpr.ptr, None]
        dims = [LOG_N, LOG_E, W, m]
        dk, dy, dst = eng.empty((4, T * m)), eng.empty((4, m)), eng.empty((m,), np.uint8)
        dc, dci, dpi, dpii, dy2, dst2 = eng.empty((8, m)), eng.empty((m,), np.uint8), eng.empty((8, m)), eng.empty((m,), np.uint8), eng.empty((4, m)), eng.empty((m,), np.uint8)
        dok, dst3, dgt, done, dst4 = eng.empty((m,), np.uint8), eng.empty((m,), np.uint8), eng.empty((48, 1)), eng.empty((1,), np.uint8), eng.empty((m,), np.uint8)

        def scalars():
            eng._call("sylow_pverify_scalars_batch", *ins, *dims, dk.ptr, dy.ptr, dst.ptr)

        def fold():
            eng._call("sylow_pverify_fold_batch", *pts, *ins, *dims, dc.ptr, dci.ptr, dpi.ptr, dpii.ptr, dy2.ptr, dst2.ptr)

        def verify():
            eng._call("sylow_pverify_verify_batch", tau.ptr, *pts, *ins, *dims, dok.ptr, dst3.ptr)

        def weighted():
            eng._call("sylow_pverify_batch_verify_weighted", tau.ptr, *pts, *ins, dch[6].ptr, *dims, dgt.ptr, done.ptr, dst4.ptr)

        if args.only_verify:
            for _ in range(args.warmup + args.reps):
                verify()
            eng.sync()
            continue
        scalars()
        verify()
        eng.sync()
        # ---- what the composition is handed: the scalars and y of (S), the term-major bases with the key replicated, pi's two terms
        import plonk_verify_model as V
        k_words = eng.from_device_soa(dk).reshape(T, m, 4)
        ints = [words_to_ints(x) for x in ch[:6]]
        checked = min(m, 4)
        for i in range(checked):
            want = V.scalars(words_to_ints(ev[i * (2 * W + 1):(i + 1) * (2 * W + 1)]), words_to_ints(pub.reshape(PUBLIC, m, 4)[:, i]), [1, 5, 7],
                             *(c[i] for c in ints), LOG_N, LOG_E)
            assert words_to_ints(k_words[:, i]) == want[0] and words_to_ints(eng.from_device_soa(dy)[i:i + 1]) == [want[1]], i
        bases = np.concatenate([np.repeat(vk, m, axis=0), proofs])
        dbases = eng.to_device_soa(bases, 8)
        pbases = np.concatenate([proofs[(P - 2) * m:(P - 1) * m], proofs[(P - 1) * m:]])
        dpb = eng.to_device_soa(pbases, 8)
        one = np.zeros((m, 4), dtype=np.uint64)
        one[:, 0] = 1
        dpsc = eng.to_device_soa(np.concatenate([one, ch[5]]), 4)
        dzero = eng.to_device_soa(np.zeros((m, 4), dtype=np.uint64), 4)
        dc2, dci2, dpi2, dpii2, dok2 = eng.empty((8, m)), eng.empty((m,), np.uint8), eng.empty((8, m)), eng.empty((m,), np.uint8), eng.empty((m,), np.uint8)

        def lincombs():
            eng._call("sylow_hip_g1_lincomb_batch", dbases.ptr, None, dk.ptr, dc2.ptr, dci2.ptr, m, T)
            eng._call("sylow_hip_g1_lincomb_batch", dpb.ptr, None, dpsc.ptr, dpi2.ptr, dpii2.ptr, m, 2)

        def kzg_verify():
            eng._call("sylow_hip_kzg_verify_batch", tau.ptr, dc2.ptr, dci2.ptr, dzero.ptr, dy.ptr, dpi2.ptr, dpii2.ptr, dok2.ptr, m)

        def composition():
            lincombs()
            kzg_verify()

        composition()
        fold()
        weighted()
        eng.sync()
        row = {"m": m, "model_checked_proofs": checked}
        row["composition_gives_the_same_flags"] = bool(np.array_equal(dok.download(), dok2.download()))
        row["fold_gives_the_composition_s_rows"] = bool(np.array_equal(dc.download(), dc2.download()) and np.array_equal(dpi.download(), dpi2.download()) and
                                                        np.array_equal(dy.download(), dy2.download()))
        row["flags_set"] = int(dok.download().sum())
        row.update(measure(timer, eng, [("scalars", scalars), ("fold", fold), ("verify", verify), ("weighted", weighted), ("lincombs", lincombs),
                                        ("kzg_verify", kzg_verify), ("composition", composition)], args.warmup, args.reps))
        row["verify_over_composition"] = round(row["verify_ms"] / row["composition_ms"], 3)
        row["new_kernels_ms"] = round(row["fold_ms"] - row["lincombs_ms"], 4)
        row["new_kernels_share_of_verify"] = round(row["new_kernels_ms"] / row["verify_ms"], 4)
        row["scalars_share_of_verify"] = round(row["scalars_ms"] / row["verify_ms"], 4)
        row["verify_us_per_proof"] = round(row["verify_ms"] * 1e3 / m, 3)
        row["weighted_us_per_proof"] = round(row["weighted_ms"] * 1e3 / m, 3)
        row["weighted_over_verify"] = round(row["weighted_ms"] / row["verify_ms"], 3)
        out["rows"].append(row)
        for d in [dpr, dev, dpub, dk, dy, dst, dc, dci, dpi, dpii, dy2, dst2, dok, dst3, dgt, done, dst4, dbases, dpb, dpsc, dzero, dc2, dci2, dpi2, dpii2, dok2] + dch:
            d.free()
        eng.trim(0)
    if args.only_verify:
        return
    out["conditions_met"] = bool(all(r["composition_gives_the_same_flags"] and r["fold_gives_the_composition_s_rows"] for r in out["rows"]))
    at14 = [r for r in out["rows"] if r["m"] == 1 << 14]
    out["new_kernels_are_a_minority_of_verify_at_2_14"] = bool(at14 and at14[0]["new_kernels_share_of_verify"] < 0.5) if at14 else None
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
