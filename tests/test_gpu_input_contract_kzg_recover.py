"""The input and memory contract for the entry points of include/sylow_hip_kzg_recover.h (kzg_recover.hip).  They are declared in a header of
their own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror include/sylow_hip.h.

  * Both entry points take scalars and mask bytes only -- no point array, no flag array -- so there is no coordinate word to reduce like
    Fp::new and no NULL flag array to read as zeros.
  * Scalars (the values of the held cells) are taken mod r: the same words out for v and v + j r, the model's words.
  * The words of cells that are not held are never part of a result: zeros, all-ones and random words give the same bytes.
  * Both entry points run between guard bands under two fill bytes (tests/guarded_engine.py, with the prototypes of the new header added
    to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte left unwritten -- the bytes
    of every output are the same under both fills and equal the plain engine's."""
import re

import numpy as np
import pytest

import kzg_prove_model as KP
import kzg_recover_model as M
import test_gpu_input_contract as T
from guarded_engine import FILLS, GuardedEngine
from test_kzg_recover_header import HEADER

R = M.R
LOG_C, LOG_L = 2, 2
TOP = (1 << 256) - 1
ROWS = {}                                                             # entry points with Fp-valued words or flag arrays: none
FR_ONLY = ["sylow_hip_kzg_recover_vanish_batch", "sylow_hip_kzg_recover_batch"]
_DATA = []


def data():
    """three blobs of 16 values in four cells of four: one cell missing, two missing (exactly half), three missing (refused)"""
    if not _DATA:
        rng = T.Xoshiro(T.SEED + 0x70)
        n, c = 1 << (LOG_C + LOG_L), 1 << LOG_C
        blobs = [[rng.u256() % R for _ in range(n // 2)] + [0] * (n // 2) for _ in range(3)]
        ys = [M.fft(f, LOG_C + LOG_L) for f in blobs]
        present = [[1, 0, 1, 1], [0, 1, 1, 0], [0, 0, 1, 0]]
        held = [[v if p[j % c] else rng.u256() for j, v in enumerate(y)] for y, p in zip(ys, present)]
        want = [M.recover(y, p, LOG_C, LOG_L) for y, p in zip(held, present)]
        assert [w[0] for w in want] == [M.OK, M.OK, M.TOO_FEW] and [w[1] for w in want[:2]] == blobs[:2]
        _DATA.append(dict(blobs=blobs, ys=ys, present=present, held=held, want=want, vanish=[M.vanish(p, LOG_C, LOG_L) for p in present]))
    return _DATA[0]


def lift(vals, present, largest=False):
    """v + j r for every held value: another word for the same element of Fr (j = 1, 2, ... in turn, or the largest that fits 256 bits)"""
    c = len(present)
    return [v + ((TOP - v) // R if largest else 1 + i % ((TOP - v) // R)) * R if present[i % c] else v for i, v in enumerate(vals)]


def prototypes():
    """{entry point: [(is a pointer, const, name)]} of the new header"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [("*" in p, "const" in p.split(), p.replace("*", " ").split()[-1]) for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_rows_name_real_parameters():
    protos = prototypes()
    assert set(ROWS) | set(FR_ONLY) == set(protos) and not ROWS
    for name in FR_ONLY:
        assert not any(p[2].endswith(("_xy", "_inf")) for p in protos[name]), name
        assert {p[2] for p in protos[name] if p[0] and p[1]} == ({"present"} if "vanish" in name else {"y", "present"}), name      # the const inputs
    assert not set(protos) & set(T.CONTRACT), "include/sylow_hip.h does not declare them"


def check(got, d):
    coeffs, y, status = got
    assert [int(s) for s in status] == [w[0] for w in d["want"]]
    assert [KP.ints(v) for v in coeffs] == [w[1] for w in d["want"]]
    if y is not None:
        assert [KP.ints(v) for v in y[:2]] == d["ys"][:2] and not y[2].any()


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_scalars_are_taken_mod_r(engine, largest):
    """the values of the held cells as v and as v + j r: the same words out, the model's words"""
    d = data()
    present = np.array(d["present"], dtype=np.uint8)
    base = engine.kzg_recover(KP.poly_words(d["held"]), present, LOG_C, LOG_L)
    check(base, d)
    lifted = [lift(v, p, largest) for v, p in zip(d["held"], d["present"])]
    assert all(v >= R for row, p in zip(lifted, d["present"]) for j, v in enumerate(row) if p[j % 4])
    got = engine.kzg_recover(KP.poly_words(lifted), present, LOG_C, LOG_L)
    T._same(list(got), list(base), "v + j r")


@pytest.mark.gpu
def test_words_of_cells_that_are_not_held_are_not_read_into_the_result(engine):
    d = data()
    present = np.array(d["present"], dtype=np.uint8)
    base = engine.kzg_recover(KP.poly_words(d["held"]), present, LOG_C, LOG_L)
    for junk in (0, TOP, R, R - 1):
        ys = [[v if p[j % 4] else junk for j, v in enumerate(y)] for y, p in zip(d["ys"], d["present"])]
        T._same(list(engine.kzg_recover(KP.poly_words(ys), present, LOG_C, LOG_L)), list(base), f"missing cells filled with {junk:#x}")
    zd, zc, status = engine.kzg_recover_vanish(present, LOG_C, LOG_L)
    assert [(KP.ints(a), KP.ints(b), int(s)) for a, b, s in zip(zd, zc, status)] == d["vanish"]


class GuardedRecover(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


def drive(eng):
    """both entry points on data() -- the recovery with and without y_out, three rows at once and one row alone"""
    d = data()
    y, present = KP.poly_words(d["held"]), np.array(d["present"], dtype=np.uint8)
    out = list(eng.kzg_recover_vanish(present, LOG_C, LOG_L))
    out += list(eng.kzg_recover(y, present, LOG_C, LOG_L))
    got = eng.kzg_recover(y, present, LOG_C, LOG_L, want_y=False)
    out += [got[0], got[2]]
    out += list(eng.kzg_recover(y[1:2], present[1:2], LOG_C, LOG_L))
    return [np.asarray(o) for o in out]


@pytest.mark.gpu
def test_every_entry_point_stays_inside_its_buffers_and_writes_its_outputs(engine):
    guarded = GuardedRecover(engine.device, engine.stream)
    outs, raw = [], []
    for fill in FILLS:
        guarded.fill = fill
        del guarded.written[:]
        outs.append(drive(guarded))                                # every call audited inside: guard bands, const inputs, @shape extents
        raw.append([(n, p, x) for n, p, x in guarded.written if n in guarded._const and "kzg" in n and "recover" in n])
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
