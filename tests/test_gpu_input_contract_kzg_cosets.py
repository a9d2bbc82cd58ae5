"""The input and memory contract for the entry points of include/sylow_hip_kzg_cosets.h (kzg_cosets.hip).  They are declared in a header of
their own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror include/sylow_hip.h.

  * Scalars (coefficients, cell values) are taken mod r: the same words out for v and v + j r, the model's words.
  * Coordinate words of points (the SRS, the table, tau^l G2gen, C, pi) are reduced like Fp::new: the same flags and points out for x and
    x + j p.
  * NULL flag arrays read as all-zero flags.
  * Every entry point runs between guard bands under two fill bytes (tests/guarded_engine.py, with the prototypes of the new header added
    to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte left unwritten -- the bytes
    of every output are the same under both fills and equal the plain engine's."""
import re

import numpy as np
import pytest

import groth16_model as G
import kzg_cosets_model as M
import kzg_prove_model as KP
import test_gpu_input_contract as T
from guarded_engine import FILLS, GuardedEngine
from test_kzg_cosets_header import HEADER

R = M.R
TAU = 0xC0FFEE0DDBA11
LOG_C, LOG_L, POLYS = 2, 2, 2
TOP = (1 << 256) - 1
ROWS = {
    "sylow_hip_kzg_open_cosets_prepare": T.Row({"srs_g1_xy": T.G1A}),
    "sylow_hip_kzg_open_cosets_batch": T.Row({"table_xy": T.G1A}, ["table_inf"]),
    "sylow_hip_kzg_open_cosets_batch_tuned": T.Row({"table_xy": T.G1A}, ["table_inf"]),
    "sylow_hip_kzg_cosets_reduce_batch": T.Row({"srs_g1_xy": T.G1A, "c_xy": T.G1A}, ["c_inf"]),
    "sylow_hip_kzg_verify_cosets_batch": T.Row({"srs_g1_xy": T.G1A, "tau_l_g2_xy": T.G2A, "c_xy": T.G1A, "pi_xy": T.G1A}, ["c_inf", "pi_inf"]),
}
FR_ONLY = ["sylow_hip_kzg_coset_interp_batch"]
_DATA = []


def data():
    """one valid instance from the model and the oracle: two polynomials of 16 coefficients on four cosets of four points; the second has a
    degree below l, so its proofs are flagged.  The rows of the verifier are the eight (polynomial, coset) pairs."""
    if not _DATA:
        rng = T.Xoshiro(T.SEED + 0x60)
        n, l, c = 1 << (LOG_C + LOG_L), 1 << LOG_L, 1 << LOG_C
        polys = [[rng.u256() % R for _ in range(n)], [rng.u256() % R for _ in range(l)] + [0] * (n - l)]
        d = dict(polys=polys, srs=KP.srs_points(TAU, n))
        tables = M.table_logs(TAU, LOG_C, LOG_L)
        d["table"], d["table_inf"] = M.points([v for t in tables for v in t])
        d["y"] = [M.values(f, LOG_C, LOG_L) for f in polys]
        logs = [M.proof_logs(f, TAU, LOG_C, LOG_L) for f in polys]
        d["pi"], d["pi_inf"] = M.points([v for p in logs for v in p])
        cxy, cinf = KP.expected_commit(polys, TAU)
        d["c"], d["c_inf"] = np.repeat(cxy, c, 0), np.repeat(cinf, c)
        d["idx"] = [i for _ in polys for i in range(c)]
        d["cells"] = [M.cells(y, LOG_C, LOG_L)[i] for y in d["y"] for i in range(c)]
        d["r"] = [M.interp_lagrange(v, i, LOG_C, LOG_L) for v, i in zip(d["cells"], d["idx"])]
        d["cred"], d["cred_inf"] = KP.canonical_identity(*G.g1_gen_mul([(M.evaluate(polys[j // c], TAU) - M.evaluate(r, TAU)) % R for j, r in enumerate(d["r"])]))
        d["z"] = [pow(M.roots(LOG_C, LOG_L)[1], i, R) for i in d["idx"]]
        g2, inf = G.g2_gen_mul([pow(TAU, l, R)])
        assert not np.asarray(inf).any() and not d["table_inf"].any() and list(d["pi_inf"]) == [0] * c + [1] * c
        d["g2"] = np.asarray(g2, dtype=np.uint64)
        _DATA.append(d)
    return _DATA[0]


def lift(vals, largest=False):
    """v + j r for every value: another word for the same element of Fr (j = 1, 2, ... in turn, or the largest that fits 256 bits)"""
    return [v + ((TOP - v) // R if largest else 1 + i % ((TOP - v) // R)) * R for i, v in enumerate(vals)]


def _prepare(eng, c):
    dt, dti = eng.kzg_open_cosets_prepare(c.fp("srs_g1_xy", data()["srs"]), LOG_L)
    return [np.ascontiguousarray(dt.download().transpose(0, 2, 1)).reshape(-1, 8), dti.download().reshape(-1)]


def _open(tuned):
    def run(eng, c):
        d = data()
        pins = dict(max_blocks=1, planes_log=1) if tuned else {}
        return list(eng.kzg_open_cosets((c.fp("table_xy", d["table"]), c.flag("table_inf", d["table_inf"])), KP.poly_words(d["polys"]), LOG_L, **pins))
    return run


def _reduce(eng, c):
    d = data()
    flags = np.array([0, 1, 0, 0, 0, 0, 0, 0], dtype=np.uint8)     # commitment 1 is flagged away: cred_1 = -R(tau) G1gen
    return list(eng.kzg_cosets_reduce(c.fp("srs_g1_xy", d["srs"][:1 << LOG_L]), c.fp("c_xy", d["c"]), d["idx"], KP.poly_words(d["cells"]), LOG_C, LOG_L,
                                      c.flag("c_inf", flags)))


def _verify(eng, c):
    d = data()
    flags = np.array([0, 1, 0, 0, 0, 0, 0, 0], dtype=np.uint8)     # its row fails, the others hold
    return [eng.kzg_verify_cosets(c.fp("srs_g1_xy", d["srs"][:1 << LOG_L]), c.fp("tau_l_g2_xy", d["g2"]), c.fp("c_xy", d["c"]), d["idx"], KP.poly_words(d["cells"]),
                                  c.fp("pi_xy", d["pi"]), LOG_C, LOG_L, c.flag("c_inf", flags), c.flag("pi_inf", d["pi_inf"]))]


CASES = {"sylow_hip_kzg_open_cosets_prepare": _prepare, "sylow_hip_kzg_open_cosets_batch": _open(False), "sylow_hip_kzg_open_cosets_batch_tuned": _open(True),
         "sylow_hip_kzg_cosets_reduce_batch": _reduce, "sylow_hip_kzg_verify_cosets_batch": _verify}


def check_row(engine, name):
    """tests/test_gpu_input_contract.py's check_row over this file's rows"""
    row, case = ROWS[name], CASES[name]
    c0 = T.Ctx()
    base = case(engine, c0)
    assert c0.seen_fp == set(row.fp) and c0.seen_flags == set(row.flags), (name, c0.seen_fp, c0.seen_flags)
    for arg in row.fp:
        T._same(case(engine, T.Ctx({arg})), base, f"{name}: {arg} as representatives")
    if len(row.fp) > 1:
        T._same(case(engine, T.Ctx(row.fp)), base, f"{name}: every Fp argument as representatives")
    T._same(case(engine, T.Ctx(row.fp, largest=True)), base, f"{name}: the largest representatives")
    if row.flags:
        T._same(case(engine, T.Ctx(flags="null")), case(engine, T.Ctx(flags="zero")), f"{name}: NULL flags against all-zero flags")
        T._same(case(engine, T.Ctx(row.fp, flags="null")), case(engine, T.Ctx(flags="zero")), f"{name}: NULL flags, representatives")
    return base


def prototypes():
    """{entry point: [(is a pointer, const, name)]} of the new header"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [("*" in p, "const" in p.split(), p.replace("*", " ").split()[-1]) for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_rows_name_real_parameters():
    from sylow_amd import _shapes
    protos, shapes = prototypes(), _shapes.parse(HEADER)
    assert set(ROWS) | set(FR_ONLY) == set(protos) and set(CASES) == set(ROWS)
    for name, row in ROWS.items():
        params = {p[2] for p in protos[name]}
        assert set(row.fp) | set(row.flags) <= params, name
        assert {p for p, sh in shapes[name][1].items() if sh.optional and sh.dtype == "u8" and p.endswith("_inf")} == set(row.flags), name
        assert {p[2] for p in protos[name] if p[0] and p[1] and p[2].endswith("_xy")} == set(row.fp), name      # every const point array
    for name in FR_ONLY:
        assert not any(p[2].endswith(("_xy", "_inf")) for p in protos[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_kzg_cosets_reduces_representatives(engine, name):
    base = check_row(engine, name)
    d = data()
    c = 1 << LOG_C
    if name.endswith("prepare"):
        assert np.array_equal(base[0], d["table"]) and np.array_equal(base[1], d["table_inf"])
    elif "open" in name:
        assert [KP.ints(y) for y in base[0]] == d["y"]
        assert np.array_equal(base[1].reshape(-1, 8), d["pi"]) and np.array_equal(base[2].reshape(-1), d["pi_inf"])
    elif "reduce" in name:
        assert np.array_equal(np.delete(base[0], 1, 0), np.delete(d["cred"], 1, 0)) and np.array_equal(np.delete(base[1], 1), np.delete(d["cred_inf"], 1))
        assert KP.ints(base[2]) == d["z"] and base[3].all()
        assert d["cred_inf"][c:].all()                                 # degree below l: C = R(tau) G1gen
    else:
        assert list(base[0]) == [1, 0, 1, 1, 1, 1, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_scalars_are_taken_mod_r(engine, largest):
    """every Fr-valued argument of the six entry points as v and as v + j r: the same words out, the model's words"""
    d = data()
    lpolys = KP.poly_words([lift(f, largest) for f in d["polys"]])
    lcells = KP.poly_words([lift(v, largest) for v in d["cells"]])
    table = (d["table"], d["table_inf"])
    for pins in ({}, dict(max_blocks=1, planes_log=0)):
        y, pxy, pinf = engine.kzg_open_cosets(table, lpolys, LOG_L, **pins)
        assert [KP.ints(v) for v in y] == d["y"] and np.array_equal(pxy.reshape(-1, 8), d["pi"]) and np.array_equal(pinf.reshape(-1), d["pi_inf"])
    r, ok = engine.kzg_coset_interp(d["idx"], lcells, LOG_C, LOG_L)
    assert [KP.ints(v) for v in r] == d["r"] and ok.all()
    cred, cred_inf, z, ok = engine.kzg_cosets_reduce(d["srs"][:1 << LOG_L], d["c"], d["idx"], lcells, LOG_C, LOG_L, d["c_inf"])
    assert np.array_equal(cred, d["cred"]) and np.array_equal(cred_inf, d["cred_inf"]) and KP.ints(z) == d["z"] and ok.all()
    assert engine.kzg_verify_cosets(d["srs"][:1 << LOG_L], d["g2"], d["c"], d["idx"], lcells, d["pi"], LOG_C, LOG_L, d["c_inf"], d["pi_inf"]).all()


class GuardedCosets(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


def drive(eng):
    """the six entry points once each, on data() -- the opening with and without y_out, with one plane and with four"""
    d = data()
    polys, cells, l = KP.poly_words(d["polys"]), KP.poly_words(d["cells"]), 1 << LOG_L
    dt, dti = eng.kzg_open_cosets_prepare(d["srs"], LOG_L)
    out = [dt.download(), dti.download()]
    out += list(eng.kzg_open_cosets((dt, dti), polys, LOG_L))
    out += list(eng.kzg_open_cosets((dt, None), polys, LOG_L, want_y=False, max_blocks=1, planes_log=0)[1:])
    out += list(eng.kzg_open_cosets((dt, dti), polys, LOG_L, max_blocks=3, planes_log=LOG_L))
    out += list(eng.kzg_coset_interp(d["idx"], cells, LOG_C, LOG_L))
    out += list(eng.kzg_cosets_reduce(d["srs"][:l], d["c"], d["idx"], cells, LOG_C, LOG_L, d["c_inf"]))
    out += [eng.kzg_verify_cosets(d["srs"][:l], d["g2"], d["c"], d["idx"], cells, d["pi"], LOG_C, LOG_L, d["c_inf"], d["pi_inf"])]
    return [np.asarray(o) for o in out]


@pytest.mark.gpu
def test_every_entry_point_stays_inside_its_buffers_and_writes_its_outputs(engine):
    guarded = GuardedCosets(engine.device, engine.stream)
    outs, raw = [], []
    for fill in FILLS:
        guarded.fill = fill
        del guarded.written[:]
        outs.append(drive(guarded))                                # every call audited inside: guard bands, const inputs, @shape extents
        raw.append([(n, p, x) for n, p, x in guarded.written if n in guarded._const and "kzg" in n and "coset" in n])
    names = {n for n, _ in guarded.audited}
    assert set(prototypes()) <= names, set(prototypes()) - names
    for name, params in prototypes().items():
        pointers = {p for ptr, _, p in params if ptr and p != "stream"}
        assert pointers == {p for n, p in guarded.audited if n == name}, (name, pointers)
    T._same(outs[0], outs[1], "the outputs under the two fills: a byte nobody wrote keeps the fill")
    assert [(n, p) for n, p, _ in raw[0]] == [(n, p) for n, p, _ in raw[1]] and raw[0]
    for (n, p, x), (_, _, y) in zip(*raw):
        assert np.array_equal(x, y), f"{n}: the bytes of {p} differ between the fills"
    T._same(outs[0], drive(engine), "the guarded engine against the plain engine")
