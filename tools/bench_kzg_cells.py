"""Timing of the check of many cells of many KZG blobs as one boolean -- sylow_hip_kzg_cells_verify_weighted (kzg_cells.hip) -- beside the
route a caller had before it existed, on device-resident arrays.  A shape is rows x n_com x log_c x log_l: `rows` cells
drawn from n_com blobs of c = 2^log_c cells of l = 2^log_l values, every cell once while there are enough, with their real commitments
and proofs (sylow_hip_kzg_commit_batch, sylow_hip_kzg_open_cosets_batch) and weights of 128 bits.
  (A)  sylow_hip_kzg_cells_verify_weighted: one call;
  (Af) its Fr half alone, sylow_hip_kzg_cells_fold_batch;
  (B)  the existing route: sylow_hip_kzg_cosets_reduce_batch over the rows with each commitment gathered per row, then
       sylow_hip_kzg_batch_verify_weighted with y = 0.  THE GATHER IS DONE ONCE, OUTSIDE THE TIMED REGION: (B) is charged less than a
       caller pays.
Before anything is timed both candidates must return the same Gt words twice: on the valid rows (the identity, is_one set) and with one
value of one cell altered (another element of Gt, is_one clear).  Device events around each call, warm-up calls first; the candidates
ALTERNATE inside every repetition in one process, the median of --reps is reported with its minimum and maximum.  The gate of a shape: (A)
faster than (B) by more than the two spreads combined.  Prints ONE JSON object and, with --out, writes it.

    python tools/bench_kzg_cells.py [--warmup 2] [--reps 7] [--out profiles/kzg_cells/bench_kzg_cells.json]"""
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
TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
G2 = [0x1800DEEF121F1E76426A00665E5C4479674322D4F75EDADD46DEBD5CD992F6ED, 0x198E9393920D483A7260BFB731FB5D25F1AA493335A9E71297E485B7AEF312C2,
      0x12C85EA5DB8C6DEB4AAB71808DCB408FE3D1E7690C43D37B4CE6CC0166FA7DAA, 0x090689D0585FF075EC9E99AD690C3395BC4B313370B38EF355ACDADCD122975B]


def words(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for k in range(4):
        out[:, k] = np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)
    return out


def blobs(eng, n_com, log_c, log_l, rng, chunk=64):
    """(SRS prefix [l, 8], tau^l G2gen [1, 16], commitments [n_com, 8], cells [n_com, c, l, 4], proofs [n_com, c, 8]) of random blobs"""
    n, c, l = 1 << (log_c + log_l), 1 << log_c, 1 << log_l
    powers, t = [], 1
    for _ in range(n):
        powers.append(t)
        t = t * TAU % R
    srs, _ = eng.g1_generator_mul(words(powers))
    tau_l, _ = eng.g2_scalar_mul(words(G2).reshape(1, 16), words([pow(TAU, l, R)]))
    table = eng.kzg_open_cosets_prepare(srs, log_l)
    coms, cells, pis = [], [], []
    for j in range(0, n_com, chunk):
        m = min(chunk, n_com - j)
        polys = random_scalars(rng, m * n).reshape(m, n, 4)
        y, pxy, pinf = eng.kzg_open_cosets(table, polys, log_l)
        assert not pinf.any()
        coms.append(eng.kzg_commit(srs, polys)[0])
        cells.append(y.reshape(m, l, c, 4).transpose(0, 2, 1, 3))                           # value t of cell i at y[i + c t]
        pis.append(pxy)
    for d in table:
        d.free()
    return srs[:l], tau_l, np.concatenate(coms), np.concatenate(cells), np.concatenate(pis)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x64x7x6,128x1x7x6,16x4x7x6,65536x512x7x6")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import sylow_amd
    eng = sylow_amd.Engine(0)
    timer = Timer(eng.stream)
    out = {"device": "cuda:0", "warmup": args.warmup, "reps": args.reps, "gather_timed": False, "rows": []}
    for rows, n_com, lc, ll in [tuple(int(v) for v in p.split("x")) for p in args.shapes.split(",") if p]:
        c, l = 1 << lc, 1 << ll
        rng = np.random.default_rng(17 * rows + 101 * n_com + 7 * lc + ll)
        srs, tau_l, coms, cells, pis = blobs(eng, n_com, lc, ll, rng)
        pick = rng.permutation(n_com * c)[:rows] if rows <= n_com * c else rng.integers(0, n_com * c, size=rows)
        com, idx = (pick // c).astype(np.uint64), (pick % c).astype(np.uint64)
        vals = np.ascontiguousarray(cells[com.astype(np.int64), idx.astype(np.int64)].transpose(0, 2, 1))       # [rows][4][l]
        weights = random_scalars(rng, rows)
        weights[:, 2:] = 0                                                                   # 128 bits
        ds, dtau, dc = eng.to_device_soa(srs, 8), eng.to_device_soa(tau_l, 16), eng.to_device_soa(coms, 8)
        dgath = eng.to_device_soa(coms[com.astype(np.int64)], 8)                             # (B)'s commitment per row: gathered once, untimed
        di, dci, dv, dw = eng.to_device(idx), eng.to_device(com), eng.to_device(vals), eng.to_device_soa(weights, 4)
        dp = eng.to_device_soa(pis[com.astype(np.int64), idx.astype(np.int64)], 8)
        dgt_a, dgt_b, dis_a, dis_b = eng.empty((48, 1)), eng.empty((48, 1)), eng.empty((1,), np.uint8), eng.empty((1,), np.uint8)
        dcred, dcinf, dz, dy0 = eng.empty((8, rows)), eng.empty((rows,), np.uint8), eng.empty((4, rows)), eng.to_device(np.zeros((4, rows), dtype=np.uint64))
        dwo, dao, dr, drz, dg = eng.empty((4, n_com)), eng.empty((4, l)), eng.empty((4, rows)), eng.empty((4, rows)), eng.empty((1,), np.uint8)

        def cells_call():
            eng._call("sylow_hip_kzg_cells_verify_weighted", ds.ptr, dtau.ptr, dc.ptr, None, di.ptr, dci.ptr, dv.ptr, dp.ptr, None, dw.ptr, lc, ll, rows, n_com,
                      dgt_a.ptr, dis_a.ptr, None)

        def fold_call():
            eng._call("sylow_hip_kzg_cells_fold_batch", di.ptr, dci.ptr, dv.ptr, dw.ptr, lc, ll, rows, n_com, dwo.ptr, dao.ptr, dr.ptr, drz.ptr, dg.ptr)

        def per_row():
            eng._call("sylow_hip_kzg_cosets_reduce_batch", ds.ptr, dgath.ptr, None, di.ptr, dv.ptr, lc, ll, rows, dcred.ptr, dcinf.ptr, dz.ptr, None)
            eng._call("sylow_hip_kzg_batch_verify_weighted", dtau.ptr, dcred.ptr, dcinf.ptr, dz.ptr, dy0.ptr, dp.ptr, None, dw.ptr, rows, dgt_b.ptr, dis_b.ptr)

        def both():
            cells_call()
            per_row()
            eng.sync()
            return dgt_a.download(), dgt_b.download(), int(dis_a.download()[0]), int(dis_b.download()[0])

        ga, gb, ia, ib = both()
        same = {"valid": bool(np.array_equal(ga, gb) and ia == 1 and ib == 1)}
        bad = vals.copy()
        bad[rows // 2, 0, 0] ^= np.uint64(1)
        dv.upload(bad)
        ga, gb, ia, ib = both()
        same["one_value_altered"] = bool(np.array_equal(ga, gb) and ia == 0 and ib == 0 and ga.any())
        dv.upload(vals)
        row = {"rows": rows, "n_com": n_com, "log_c": lc, "log_l": ll, "same_gt_words": same}
        if all(same.values()):                                      # nothing is timed before every candidate has returned the same words
            row.update(measure(timer, eng, [("cells", cells_call), ("per_row", per_row), ("cells_fold", fold_call)], args.warmup, args.reps))
            spread = (row["cells_ms_max"] - row["cells_ms_min"]) + (row["per_row_ms_max"] - row["per_row_ms_min"])
            row["spreads_combined_ms"] = round(spread, 4)
            row["per_row_over_cells"] = round(row["per_row_ms"] / row["cells_ms"], 3)
            row["cells_faster_beyond_spreads"] = bool(row["per_row_ms"] - row["cells_ms"] > spread)
            row["cells_rest_ms"] = round(row["cells_ms"] - row["cells_fold_ms"], 4)             # the curve half and the pairing
        out["rows"].append(row)
        for d in (ds, dtau, dc, dgath, di, dci, dv, dw, dp, dgt_a, dgt_b, dis_a, dis_b, dcred, dcinf, dz, dy0, dwo, dao, dr, drz, dg):
            d.free()
    out["conditions_met"] = bool(all(all(r["same_gt_words"].values()) for r in out["rows"]))
    first = out["rows"][0] if out["rows"] else {}
    out["gate"] = bool(first.get("cells_faster_beyond_spreads", False))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
