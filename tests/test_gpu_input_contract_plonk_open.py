"""The input and memory contract for the entry points of include/sylow_popen.h (plonk_open.hip).  They are declared in a header of their
own, under a prefix of their own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror
include/sylow_hip.h.

  * Every scalar (selectors, sigma, wires, z, public inputs, t, evaluations, shifts and the five challenges) as v and as v + j r: the same
    bytes out.
  * Every entry point runs between guard bands under two fill bytes (tests/guarded_engine.py, imported and subclassed: the prototypes of
    the new header are added to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte
    left unwritten, the optional r_out and f_out included -- the bytes of every output are the same under both fills and equal the plain
    engine's.
  * Every SYLOW_HIP_E_ARG case of the header, with nothing written, and the refusal when the scratch limit does not hold one instance."""
import random
import re

import numpy as np
import pytest

import kzg_prove_model as M
import plonk_open_model as O
import test_gpu_input_contract as T
from groth16_model import limbs
from guarded_engine import FILLS, GuardedEngine
from test_popen_header import HEADER

R = O.R
TOP = (1 << 256) - 1
E_HIP, E_ARG = -1, -2
LOG_N, LOG_E, WIRES, INSTANCES = 5, 2, 3, 2
LEN_W, LEN_Z, LEN_OUT, LEN_F = 34, 35, 300, 40            # blinded lengths; len_out: two tiles, zeros from 35 on; the SRS of the full route
SENTINEL = 0x5A5A5A5A5A5A5A5A
OUTPUTS = ("ctable", "evals_out", "r_out", "f_out", "status", "w_zeta_xy", "w_zeta_inf", "w_omega_xy", "w_omega_inf")


def prototypes():
    """{entry point: [(is a pointer, const, name)]} of the new header"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(sylow_popen_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [("*" in p, "const" in p.split(), p.replace("*", " ").split()[-1]) for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_outputs_are_the_non_const_pointers():
    protos = prototypes()
    assert len(protos) == 6 and not set(protos) & set(T.CONTRACT), "include/sylow_hip.h does not declare them"
    for name, params in protos.items():
        pointers = [p for p in params if p[0] and p[2] != "stream"]
        outputs = OUTPUTS if name == "sylow_popen_prepare" else OUTPUTS[1:]      # ctable is the output of prepare and an input everywhere else
        assert all(p[1] == (p[2] not in outputs) for p in pointers) and any(not p[1] for p in pointers), name


def batch():
    """values below r >> 3, so that v + j r has room: random rows of the blinded lengths"""
    rng = random.Random(T.SEED + 0x9108)
    n, big = 1 << LOG_N, 1 << (LOG_N + LOG_E)
    small = lambda *shape: [small(*shape[1:]) for _ in range(shape[0])] if len(shape) > 1 else [rng.randrange(R >> 3) for _ in range(shape[0])]
    b = {"selectors": small(WIRES + 2, n), "sigma": small(WIRES, n), "shifts": small(WIRES), "wires": small(INSTANCES, WIRES, LEN_W), "z": small(INSTANCES, LEN_Z),
         "pi": small(INSTANCES, n), "t": small(INSTANCES, big), "evals": small(INSTANCES, 2 * WIRES + 1)}
    for k in ("beta", "gamma", "alpha", "zeta", "v"):
        b[k] = small(INSTANCES)
    return b


def lift(tree, largest):
    """v + j r for every value of a nested list: another word for the same element of Fr"""
    if isinstance(tree, list):
        return [lift(t, largest) for t in tree]
    return tree + ((TOP - tree) // R if largest else 1 + tree % ((TOP - tree) // R)) * R


def words(rows):
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


@pytest.fixture(scope="module")
def srs():
    return M.srs_points(0xC0FFEE0123456789ABCDEF, LEN_F)


def drive(eng, b, srs):
    """every entry point once, the default form and the tuned one, with and without public inputs, r alone, F alone and both, then the full
    route: the list of every output"""
    ctable = eng.plonk_open_prepare(words(b["selectors"]), words(b["sigma"]))
    out = [eng.plonk_open_ctable_down(ctable)]
    ch = [limbs(b[k]) for k in ("beta", "gamma", "alpha", "zeta", "v")]
    for pins in ({}, {"max_blocks": 1}):
        for with_pi in (True, False):
            out.append(eng.plonk_open_evaluate(ctable, words(b["wires"]), words(b["z"]), words(b["pi"]) if with_pi else None, ch[3], **pins))
        for want_r, want_f in ((True, True), (True, False), (False, True)):
            got = eng.plonk_open_linearise(ctable, words(b["wires"]), words(b["z"]), words(b["t"]), words(b["evals"]), limbs(b["shifts"]), *ch, LOG_E,
                                           len_out=LEN_OUT, want_r=want_r, want_f=want_f, **pins)
            out += [x for x in got if x is not None]
    for with_pi in (True, False):
        ev, (p1, f1), (p2, f2), status = eng.plonk_open(srs, ctable, words(b["wires"]), words(b["z"]), words(b["pi"]) if with_pi else None, words(b["t"]),
                                                        limbs(b["shifts"]), *ch, LOG_E)
        out += [ev, p1, f1, p2, f2, status]
    return [np.asarray(o) for o in out]


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_representatives_give_the_same_bytes(engine, srs, largest):
    b = batch()
    base = drive(engine, b, srs)
    lifted = {k: lift(v, largest) for k, v in b.items()}
    assert min(lifted["v"]) >= R and min(min(r) for r in lifted["selectors"]) >= R and min(min(r) for r in lifted["evals"]) >= R
    T._same(drive(engine, lifted, srs), base, "v + j r")
    ct = O.ctable(b["selectors"], b["sigma"], LOG_N)
    assert np.array_equal(base[0], words(ct))
    want_ev = [O.evaluate(ct, b["wires"][s], b["z"][s], b["pi"][s], b["zeta"][s], LOG_N) for s in range(INSTANCES)]
    assert np.array_equal(base[1], words(want_ev))
    want = [O.linearise(ct, b["wires"][s], b["z"][s], b["t"][s], b["evals"][s], b["shifts"], b["beta"][s], b["gamma"][s], b["alpha"][s], b["zeta"][s], b["v"][s],
                        LOG_N, LOG_E) for s in range(INSTANCES)]
    r, f, status = base[3:6]                                          # after the table and the two evaluations
    assert r.shape == (INSTANCES, LEN_OUT, 4) and not r[:, LEN_Z:].any() and not f[:, LEN_Z:].any()
    assert np.array_equal(r[:, :LEN_Z], words([w[0] for w in want])) and np.array_equal(f[:, :LEN_Z], words([w[1] for w in want])) and list(status) == [w[2] for w in want]


class GuardedOpening(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


@pytest.mark.gpu
def test_every_entry_point_stays_inside_its_buffers_and_writes_its_outputs(engine, srs):
    b = batch()
    guarded = GuardedOpening(engine.device, engine.stream)
    outs, raw = [], []
    for fill in FILLS:
        guarded.fill = fill
        del guarded.written[:]
        outs.append(drive(guarded, b, srs))                         # every call audited inside: guard bands, const inputs, @shape extents
        raw.append([(n, p, x) for n, p, x in guarded.written if n in prototypes()])
    names = {n for n, _ in guarded.audited}
    assert set(prototypes()) <= names, set(prototypes()) - names
    for name, params in prototypes().items():
        pointers = {p for ptr, _, p in params if ptr and p != "stream"}
        assert pointers == {p for n, p in guarded.audited if n == name}, (name, pointers)
    T._same(outs[0], outs[1], "the outputs under the two fills: a byte nobody wrote keeps the fill")
    assert [(n, p) for n, p, _ in raw[0]] == [(n, p) for n, p, _ in raw[1]] and raw[0]
    for (n, p, x), (_, _, y) in zip(*raw):
        assert np.array_equal(x, y), f"{n}: the bytes of {p} differ between the fills"
    T._same(outs[0], drive(engine, b, srs), "the guarded engine against the plain engine")


@pytest.mark.gpu
def test_argument_errors_write_nothing(engine):
    lib, st = engine.lib, engine.stream
    log_n, log_e, W, m = 3, 2, 2, 2
    n, big, len_out = 1 << log_n, 1 << (log_n + log_e), 12
    fill = np.full(4 * big * m + 64, SENTINEL, dtype=np.uint64)       # every array is as large as the largest
    keys = ("srs", "ct", "sel", "sig", "wires", "z", "pi", "t", "ev", "sh", "be", "ga", "al", "ze", "v", "r", "f", "e_out", "p1", "p2")
    arrays = {k: engine.to_device(fill) for k in keys}
    flags = {k: engine.to_device(np.full(8, 0x5A, dtype=np.uint8)) for k in ("status", "i1", "i2")}
    p = {k: d.ptr for k, d in list(arrays.items()) + list(flags.items())}
    bad = lambda rc: rc == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    sub = lambda lst, **kw: [kw.get("i%d" % k, v) for k, v in enumerate(lst)]
    prep = lambda *a: lib.sylow_popen_prepare(*a, st)
    ev = lambda *a: lib.sylow_popen_evaluate_batch(*a, st)
    lin = lambda *a: lib.sylow_popen_linearise_batch(*a, st)
    full = lambda *a: lib.sylow_popen_open_batch(*a, st)
    pr_full = [p["sel"], p["sig"], log_n, W, p["ct"]]
    ev_full = [p["ct"], p["wires"], n + 2, p["z"], n + 3, p["pi"], p["ze"], log_n, W, m, p["e_out"]]
    li_full = [p["ct"], p["wires"], n + 2, p["z"], n + 3, p["t"], p["ev"], p["sh"], p["be"], p["ga"], p["al"], p["ze"], p["v"], log_n, log_e, W, m, len_out, p["r"],
               p["f"], p["status"]]
    op_full = [p["srs"], p["ct"], p["wires"], n + 2, p["z"], n + 3, p["pi"], p["t"], p["sh"], p["be"], p["ga"], p["al"], p["ze"], p["v"], log_n, log_e, W, m, 16,
               p["e_out"], p["p1"], p["i1"], p["p2"], p["i2"], p["status"]]
    ev_t = lambda mb: lib.sylow_popen_evaluate_batch_tuned(*ev_full[:10], mb, ev_full[10], st)
    li_t = lambda mb: lib.sylow_popen_linearise_batch_tuned(*li_full[:18], mb, *li_full[18:], st)
    # NULL where an array is required (pi may be NULL; wires and v only beside f_out; r_out or f_out, not both NULL)
    for i in (0, 1, 4):
        assert bad(prep(*[None if k == i else v for k, v in enumerate(pr_full)])), i
    for i in (0, 1, 3, 6, 10):
        assert bad(ev(*[None if k == i else v for k, v in enumerate(ev_full)])), i
    for i in (0, 1, 3, 5, 6, 7, 8, 9, 10, 11, 12, 20):
        assert bad(lin(*[None if k == i else v for k, v in enumerate(li_full)])), i
    assert bad(lin(*sub(li_full, i18=None, i19=None)))
    for i in (0, 1, 2, 4, 7, 8, 9, 10, 11, 12, 13, 19, 20, 21, 22, 23, 24):
        assert bad(full(*[None if k == i else v for k, v in enumerate(op_full)])), i
    # log_n, log_e and W out of range, whatever m is; the pin
    for lg, w in ((-1, W), (29, W), (log_n, 1), (log_n, 0), (log_n, 33), (log_n, -1)):
        assert bad(prep(*sub(pr_full, i2=lg, i3=w))) and bad(ev(*sub(ev_full, i7=lg, i8=w))) and bad(ev(*sub(ev_full, i7=lg, i8=w, i9=0))), (lg, w)
    for lg, le, w in ((-1, log_e, W), (log_n, -1, W), (27, 2, W), (29, 0, W), (0, 29, W), (log_n, log_e, 1), (log_n, log_e, 33), (log_n, log_e, -1)):
        assert bad(lin(*sub(li_full, i13=lg, i14=le, i15=w))) and bad(full(*sub(op_full, i14=lg, i15=le, i16=w))), (lg, le, w)
        assert bad(lin(*sub(li_full, i13=lg, i14=le, i15=w, i16=0))) and bad(full(*sub(op_full, i14=lg, i15=le, i16=w, i17=0))), "refused whatever m is"
    assert bad(ev_t(0)) and bad(li_t(0))
    # the lengths: outside 1 .. N (1 .. 2^28 where there is no log_e)
    for lw, lz in ((0, n), (n, 0), (big + 1, n), (n, big + 1)):
        assert bad(lin(*sub(li_full, i2=lw, i4=lz))) and bad(full(*sub(op_full, i3=lw, i5=lz))), (lw, lz)
    for lw, lz in ((0, n), (n, 0), ((1 << 28) + 1, n), (n, (1 << 28) + 1)):
        assert bad(ev(*sub(ev_full, i2=lw, i4=lz))), (lw, lz)
    # len_out and len_f below max(n, len_z), and below len_w as well when F is asked for
    assert bad(lin(*sub(li_full, i17=n + 2))) and bad(lin(*sub(li_full, i4=4, i17=n - 1))) and bad(lin(*sub(li_full, i2=20, i17=19)))
    assert bad(full(*sub(op_full, i18=n + 2))) and bad(full(*sub(op_full, i3=20, i18=19))) and bad(full(*sub(op_full, i18=0)))
    # an output that overlaps an input or another output, by byte ranges
    assert bad(prep(*sub(pr_full, i4=p["sel"]))) and bad(prep(*sub(pr_full, i4=p["sig"] + 8))) and bad(prep(*sub(pr_full, i4=p["sel"] - 32 * n * (2 * W + 2) + 8)))
    for k in (0, 1, 3, 5, 6):                                    # evals_out over every input
        assert bad(ev(*sub(ev_full, i10=ev_full[k]))) and bad(ev(*sub(ev_full, i10=ev_full[k] - 32 * (2 * W + 1) * m + 8))), k
    for k in (0, 1, 3, 5, 6, 7, 8, 9, 10, 11, 12):               # r_out, f_out and status over every input
        assert bad(lin(*sub(li_full, i18=li_full[k]))) and bad(lin(*sub(li_full, i19=li_full[k] + 8))) and bad(lin(*sub(li_full, i20=li_full[k] + 3))), k
    assert bad(lin(*sub(li_full, i19=p["r"]))) and bad(lin(*sub(li_full, i19=p["r"] + 32 * len_out * m - 8))) and bad(lin(*sub(li_full, i20=p["f"] + 1)))
    for k in (0, 1, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13):           # every output of the full route over every input
        for o in (19, 20, 21, 22, 23, 24):
            assert bad(full(*sub(op_full, **{"i%d" % o: op_full[k] + 8}))), (k, o)
    assert bad(full(*sub(op_full, i22=p["p1"]))) and bad(full(*sub(op_full, i24=p["i1"] + 1))) and bad(full(*sub(op_full, i21=p["e_out"] + 5)))
    # the scratch limit does not hold one instance of the full route: refused before anything is enqueued
    try:
        engine.set_scratch_limit(64)
        assert full(*op_full) == E_HIP and b"does not hold one instance" in lib.sylow_hip_last_error()
    finally:
        engine.set_scratch_limit(0)
    # m = 0: OK, nothing launched, whatever the pointers
    assert ev(None, None, 1, None, 1, None, None, log_n, W, 0, None) == 0
    assert lin(*([None, None, 1, None, 1] + [None] * 8 + [log_n, log_e, W, 0, n, None, None, None])) == 0
    assert full(*([None, None, None, 1, None, 1] + [None] * 8 + [log_n, log_e, W, 0, n] + [None] * 6)) == 0
    engine.sync()
    for k, d in arrays.items():
        assert np.array_equal(d.download(), fill), f"{k}: nothing written"
    for k, d in flags.items():
        assert (d.download() == 0x5A).all(), k
    # the shortest legal len_out runs, and writes every status byte of the batch and no other
    assert lin(*sub(li_full, i17=n + 3)) == 0
    engine.sync()
    assert (flags["status"].download()[:m] <= 3).all() and (flags["status"].download()[m:] == 0x5A).all()
