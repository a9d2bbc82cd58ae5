"""The input and memory contract for the entry points of include/sylow_hip_kzg_points.h (kzg_points.hip).  They are declared in a header
of their own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror include/sylow_hip.h.

  * Scalars (coefficients, z, y) are taken mod r: the same words out for v and v + j r, the model's words.
  * Coordinate words of points (the SRS on both sides, C, pi) are reduced like Fp::new: the same flags and points out for x and x + j p.
  * NULL flag arrays read as all-zero flags.
  * Every entry point runs between guard bands under two fill bytes (tests/guarded_engine.py, with the prototypes of the new header added
    to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte left unwritten -- the bytes
    of every output are the same under both fills and equal the plain engine's."""
import re

import numpy as np
import pytest

import groth16_model as G
import kzg_points_model as M
import kzg_prove_model as KP
import test_gpu_input_contract as T
from guarded_engine import FILLS, GuardedEngine
from test_kzg_points_header import HEADER

R = M.R
TAU = 0xC0FFEE0DDBA11
N, K, ROWS_N = 21, 3, 4
ROWS = {
    "sylow_hip_kzg_open_points_batch": T.Row({"srs_g1_xy": T.G1A}),
    "sylow_hip_kzg_verify_points_batch": T.Row({"srs_g1_xy": T.G1A, "srs_g2_xy": T.G2A, "c_xy": T.G1A, "pi_xy": T.G1A}, ["c_inf", "pi_inf"]),
}
FR_ONLY = ["sylow_hip_kzg_points_weights_batch", "sylow_hip_kzg_quotient_points_batch", "sylow_hip_kzg_points_polys_batch"]
_DATA = []


def data():
    """one valid instance from the model and the oracle: four polynomials of 21 coefficients at three points each; row 3 has a zero quotient"""
    if not _DATA:
        rng = T.Xoshiro(T.SEED + 0x50)
        polys = [[rng.u256() % R for _ in range(N)] for _ in range(ROWS_N)]
        polys[3] = polys[3][:K] + [0] * (N - K)
        rows = [[rng.u256() % R for _ in range(K)] for _ in range(ROWS_N)]
        d = dict(polys=polys, rows=rows)
        d["y"], d["pi"], d["pi_inf"] = M.expected_open(polys, rows, TAU)
        d["q"] = [M.quotient_points(f, zs)[0] for f, zs in zip(polys, rows)]
        d["srs"] = KP.srs_points(TAU, N)
        d["c"], d["c_inf"] = KP.expected_commit(polys, TAU)
        g2, inf = G.g2_gen_mul(KP.srs_logs(TAU, K + 1))
        assert not np.asarray(inf).any() and list(d["pi_inf"]) == [0, 0, 0, 1]
        d["g2"] = np.asarray(g2, dtype=np.uint64)
        _DATA.append(d)
    return _DATA[0]


def lift(vals, largest=False):
    """v + j r for every value: another word for the same element of Fr (j = 1, 2, ... in turn, or the largest that fits 256 bits)"""
    return [v + ((M.TOP - v) // R if largest else 1 + i % ((M.TOP - v) // R)) * R for i, v in enumerate(vals)]


def _open(eng, c):
    d = data()
    return list(eng.kzg_open_points(c.fp("srs_g1_xy", d["srs"]), KP.poly_words(d["polys"]), M.row_words(d["rows"])))


def _verify(eng, c):
    d = data()
    flags = np.array([0, 1, 0, 0], dtype=np.uint8)                 # commitment 1 is flagged away: its row fails, the others hold
    return [eng.kzg_verify_points(c.fp("srs_g1_xy", d["srs"][:K]), c.fp("srs_g2_xy", d["g2"]), c.fp("c_xy", d["c"]), M.row_words(d["rows"]), M.row_words(d["y"]),
                                  c.fp("pi_xy", d["pi"]), c.flag("c_inf", flags), c.flag("pi_inf", d["pi_inf"]))]


CASES = {"sylow_hip_kzg_open_points_batch": _open, "sylow_hip_kzg_verify_points_batch": _verify}


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
    assert set(ROWS) | set(FR_ONLY) == set(protos)
    for name, row in ROWS.items():
        params = {p[2] for p in protos[name]}
        assert set(row.fp) | set(row.flags) <= params, name
        assert {p for p, sh in shapes[name][1].items() if sh.optional and sh.dtype == "u8" and p.endswith("_inf")} == set(row.flags), name
        assert {p[2] for p in protos[name] if p[0] and p[1] and p[2].endswith("_xy")} == set(row.fp), name      # every const point array
    for name in FR_ONLY:
        assert not any(p[2].endswith(("_xy", "_inf")) for p in protos[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_kzg_points_reduces_representatives(engine, name):
    base = check_row(engine, name)
    d = data()
    if "open" in name:
        assert np.array_equal(base[0], M.row_words(d["y"])) and np.array_equal(base[1], d["pi"]) and np.array_equal(base[2], d["pi_inf"])
    else:
        assert list(base[0]) == [1, 0, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_scalars_are_taken_mod_r(engine, largest):
    """every Fr-valued argument of the five entry points as v and as v + j r: the same words out, the model's words"""
    d = data()
    up = lambda rows: M.row_words([lift(r, largest) for r in rows])
    lpolys = KP.poly_words([lift(f, largest) for f in d["polys"]])
    want_a = M.row_words([M.weights(zs)[0] for zs in d["rows"]])
    a, distinct = engine.kzg_points_weights(up(d["rows"]))
    assert np.array_equal(a, want_a) and distinct.all()
    q, y = engine.kzg_quotient_points(lpolys, up(d["rows"]))
    assert np.array_equal(q, KP.poly_words(d["q"])) and np.array_equal(y, M.row_words(d["y"]))
    y, pi, pi_inf = engine.kzg_open_points(d["srs"], lpolys, up(d["rows"]))
    assert np.array_equal(y, M.row_words(d["y"])) and np.array_equal(pi, d["pi"]) and np.array_equal(pi_inf, d["pi_inf"])
    Z, Rp, distinct = engine.kzg_points_polys(up(d["rows"]), up(d["y"]))
    assert np.array_equal(Z, KP.poly_words([M.vanishing(zs) for zs in d["rows"]])) and distinct.all()
    assert np.array_equal(Rp, KP.poly_words([M.remainder_points(zs, ys) for zs, ys in zip(d["rows"], d["y"])]))
    ok = engine.kzg_verify_points(d["srs"][:K], d["g2"], d["c"], up(d["rows"]), up(d["y"]), d["pi"], d["c_inf"], d["pi_inf"])
    assert ok.all()


class GuardedPoints(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


def drive(eng):
    """the five entry points once each, on data() -- the quotient on both of its routes and with either output alone"""
    d = data()
    polys, rows, ys = KP.poly_words(d["polys"]), M.row_words(d["rows"]), M.row_words(d["y"])
    long_polys = np.concatenate([polys, np.zeros((ROWS_N, 2 * 2048 + 5 - N, 4), dtype=np.uint64)], axis=1)      # three chunks: totals, the carry level
    long_polys[:, -1, 0] = 7
    out = list(eng.kzg_points_weights(rows))
    out += list(eng.kzg_quotient_points(polys, rows))
    out += list(eng.kzg_quotient_points(long_polys, rows))
    out += [eng.kzg_quotient_points(long_polys, rows, want_q=False)[1], eng.kzg_quotient_points(long_polys, rows, want_y=False)[0]]
    out += list(eng.kzg_open_points(d["srs"], polys, rows))
    out += list(eng.kzg_points_polys(rows, ys))
    out += [eng.kzg_verify_points(d["srs"][:K], d["g2"], d["c"], rows, ys, d["pi"], d["c_inf"], d["pi_inf"])]
    return [np.asarray(o) for o in out]


@pytest.mark.gpu
def test_every_entry_point_stays_inside_its_buffers_and_writes_its_outputs(engine):
    guarded = GuardedPoints(engine.device, engine.stream)
    outs, raw = [], []
    for fill in FILLS:
        guarded.fill = fill
        del guarded.written[:]
        outs.append(drive(guarded))                                # every call audited inside: guard bands, const inputs, @shape extents
        raw.append([(n, p, x) for n, p, x in guarded.written if n in guarded._const and "kzg" in n and "points" in n])
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
