"""The input and memory contract for the entry points of include/sylow_hip_kzg_cells.h (kzg_cells.hip).  They are declared in a header of
their own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror include/sylow_hip.h.

  * Coordinate words of the SRS prefix, the commitments and the proofs as x and as x + p, and scalars (cell values, weights) as v and as
    v + j r: the same bytes out of every entry point.
  * A NULL flag array reads as all zeros.
  * Every entry point runs between guard bands under two fill bytes (tests/guarded_engine.py, with the prototypes of the new header added
    to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte left unwritten -- the bytes
    of every output are the same under both fills and equal the plain engine's."""
import re

import numpy as np
import pytest

import test_gpu_input_contract as T
import test_gpu_kzg_cells as G
from groth16_model import ints, limbs
from guarded_engine import FILLS, GuardedEngine
from test_kzg_cells_header import HEADER

R = G.R
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
LOG_C, LOG_L = 2, 2
TOP = (1 << 256) - 1
FP_ARGS = {"sylow_hip_kzg_cells_fold_batch": set(), "sylow_hip_kzg_cells_fold_batch_tuned": set(),
           "sylow_hip_kzg_cells_reduce_batch": {"srs_g1_xy", "c_xy", "pi_xy"}, "sylow_hip_kzg_cells_verify_weighted": {"srs_g1_xy", "c_xy", "pi_xy"}}
FLAG_ARGS = {"c_inf", "pi_inf"}


def prototypes():
    """{entry point: [(is a pointer, const, name)]} of the new header"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [("*" in p, "const" in p.split(), p.replace("*", " ").split()[-1]) for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_rows_name_real_parameters():
    protos = prototypes()
    assert set(FP_ARGS) == set(protos)
    for name, params in protos.items():
        names = {p[2] for p in params}
        assert FP_ARGS[name] <= names and {p[2] for p in params if p[0] and p[1] and p[2].endswith("_xy")} - {"tau_l_g2_xy"} == FP_ARGS[name], name
        assert {p[2] for p in params if p[2].endswith("_inf") and p[1]} == (FLAG_ARGS if FP_ARGS[name] else set()), name
        assert all(p[1] == (not p[2].endswith(("_out", "f_xy", "f_inf", "p_xy", "p_inf", "is_one"))) for p in params if p[0] and p[2] != "stream"), name
    assert not set(protos) & set(T.CONTRACT), "include/sylow_hip.h does not declare them"


def batch(engine):
    """every cell of three blobs at (2, 2), one row repeated, one masked and one out of range with the weight 0"""
    b = G.blobs(engine, LOG_C, LOG_L)
    picks = [(j, i) for j in range(3) for i in range(1 << LOG_C)] + [(1, 2)]
    rows, _, pxy, pinf = G.sample(b, LOG_C, picks, T.SEED + 0x71)
    rows[4] = rows[4][:3] + (0,)
    rows.append((1 << LOG_C, 0, rows[0][2], R))
    return b, rows, np.concatenate([pxy, pxy[:1]]), np.concatenate([pinf, pinf[:1]])


def lift_fp(xy, largest):
    """x + j p for every coordinate: another word for the same element of Fp"""
    vals = ints(np.asarray(xy).reshape(-1, 4))
    return limbs([v + ((TOP - v) // P if largest else 1) * P for v in vals]).reshape(np.asarray(xy).shape)


def lift_fr(vals, largest):
    return [v + ((TOP - v) // R if largest else 1 + i % ((TOP - v) // R)) * R for i, v in enumerate(vals)]


def drive(eng, b, rows, pxy, pinf, srs=None, cxy=None, cinf="zero", pflags="given"):
    """every entry point once (the fold on the default form and on the tuned one): the list of every output"""
    idx, com, cells, weights = G.arrays(rows, LOG_L)
    srs = b["srs_l"] if srs is None else srs
    cxy = b["coms"][0] if cxy is None else cxy
    ci = None if cinf == "null" else np.zeros(3, dtype=np.uint8)
    pf = {"given": pinf, "null": None, "zero": np.zeros(len(rows), dtype=np.uint8)}[pflags]
    out = []
    for route in (-1, 1, 0):
        W, A, r, rz, flag = eng.kzg_cells_fold(idx, com, cells, weights, LOG_C, LOG_L, 3, route=route)
        out += [W, A, r, rz, np.array([flag])]
    f, fi, p, pi, flag = eng.kzg_cells_reduce(srs, cxy, idx, com, cells, pxy, weights, LOG_C, LOG_L, c_inf=ci, pi_inf=pf)
    out += [f, fi, p, pi, np.array([flag])]
    gt, ok, flag = eng.kzg_cells_verify_weighted(srs, b["tau_l"], cxy, idx, com, cells, pxy, weights, LOG_C, LOG_L, c_inf=ci, pi_inf=pf)
    return [np.asarray(o) for o in out + [gt, np.array([ok, flag])]]


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_representatives_give_the_same_bytes(engine, largest):
    b, rows, pxy, pinf = batch(engine)
    base = drive(engine, b, rows, pxy, pinf)
    assert base[-1].all(), "the batch is valid and in range"
    T._same(drive(engine, b, rows, lift_fp(pxy, largest), pinf, srs=lift_fp(b["srs_l"], largest), cxy=lift_fp(b["coms"][0], largest)), base, "x + j p")
    lifted = [(i, cb, lift_fr(v, largest), lift_fr([w], largest)[0]) for i, cb, v, w in rows]
    assert all(w >= R and min(v) >= R for _, _, v, w in lifted)
    T._same(drive(engine, b, lifted, pxy, pinf), base, "v + j r")


@pytest.mark.gpu
def test_null_flag_arrays_read_as_zeros(engine):
    b, rows, pxy, pinf = batch(engine)
    assert not pinf.any() and not b["coms"][1].any()
    base = drive(engine, b, rows, pxy, pinf, cinf="zero", pflags="zero")
    T._same(drive(engine, b, rows, pxy, pinf, cinf="null", pflags="null"), base, "NULL flags against all-zero flags")
    T._same(drive(engine, b, rows, pxy, pinf, cinf="null", pflags="zero"), base, "NULL c_inf alone")


class GuardedCells(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


@pytest.mark.gpu
def test_every_entry_point_stays_inside_its_buffers_and_writes_its_outputs(engine):
    b, rows, pxy, pinf = batch(engine)
    guarded = GuardedCells(engine.device, engine.stream)
    outs, raw = [], []
    for fill in FILLS:
        guarded.fill = fill
        del guarded.written[:]
        outs.append(drive(guarded, b, rows, pxy, pinf))            # every call audited inside: guard bands, const inputs, @shape extents
        raw.append([(n, p, x) for n, p, x in guarded.written if n in guarded._const and "kzg_cells" in n])
    names = {n for n, _ in guarded.audited}
    assert set(prototypes()) <= names, set(prototypes()) - names
    for name, params in prototypes().items():
        pointers = {p for ptr, _, p in params if ptr and p != "stream"}
        assert pointers == {p for n, p in guarded.audited if n == name}, (name, pointers)
    T._same(outs[0], outs[1], "the outputs under the two fills: a byte nobody wrote keeps the fill")
    assert [(n, p) for n, p, _ in raw[0]] == [(n, p) for n, p, _ in raw[1]] and raw[0]
    for (n, p, x), (_, _, y) in zip(*raw):
        assert np.array_equal(x, y), f"{n}: the bytes of {p} differ between the fills"
    T._same(outs[0], drive(engine, b, rows, pxy, pinf), "the guarded engine against the plain engine")
