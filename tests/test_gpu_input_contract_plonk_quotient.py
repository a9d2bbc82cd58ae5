"""The input and memory contract for the entry points of include/sylow_plonk.h (plonk_quotient.hip).  They are declared in a header of their
own, under a prefix of their own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror
include/sylow_hip.h.

  * Every scalar (selectors, sigma, wires, z, public inputs, shifts, beta, gamma, alpha) as v and as v + j r: the same bytes out.
  * Every entry point runs between guard bands under two fill bytes (tests/guarded_engine.py, with the prototypes of the new header added
    to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte left unwritten -- the bytes
    of every output are the same under both fills and equal the plain engine's.
  * Every SYLOW_HIP_E_ARG case of the header, with nothing written."""
import random
import re

import numpy as np
import pytest

import plonk_quotient_model as Q
import test_gpu_input_contract as T
from groth16_model import limbs
from guarded_engine import FILLS, GuardedEngine
from test_plonk_header import HEADER

R = Q.R
TOP = (1 << 256) - 1
E_ARG = -2
LOG_N, LOG_E, WIRES, M = 7, 2, 3, 2                       # N = 512: two tiles, and a tail of t that crosses one
SENTINEL = 0x5A5A5A5A5A5A5A5A
OUTPUTS = ("t_ext_out", "t_out", "status")                # and the table, for the one call that writes it


def prototypes():
    """{entry point: [(is a pointer, const, name)]} of the new header"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(sylow_plonk_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [("*" in p, "const" in p.split(), p.replace("*", " ").split()[-1]) for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_outputs_are_the_non_const_pointers():
    protos = prototypes()
    assert len(protos) == 5 and not set(protos) & set(T.CONTRACT), "include/sylow_hip.h does not declare them"
    for name, params in protos.items():
        pointers = [p for p in params if p[0] and p[2] != "stream"]
        outputs = ("table",) if name == "sylow_plonk_quotient_prepare" else OUTPUTS
        assert all(p[1] == (p[2] not in outputs) for p in pointers) and any(not p[1] for p in pointers), name


def batch():
    """values below r: a circuit with public inputs and two instances, blinded wires and z (a satisfied one and a broken one), and random
    values on K for the fused kernel"""
    rng = random.Random(T.SEED + 0x9107)
    c = Q.circuit(rng, LOG_N, WIRES, with_pi=True)
    big = 1 << (LOG_N + LOG_E)
    ch = [[rng.randrange(R >> 3) for _ in range(M)] for _ in range(3)]
    polys = [Q.witness_polys(c, ch[0][s], ch[1][s], rng) for s in range(M)]
    polys[1][0][2][5] = (polys[1][0][2][5] + 1) % R
    small = lambda *shape: [small(*shape[1:]) for _ in range(shape[0])] if len(shape) > 1 else [rng.randrange(R >> 3) for _ in range(shape[0])]
    return {"selectors": c["selectors"], "sigma": c["sigma"], "shifts": c["shifts"], "wires": [p[0] for p in polys], "z": [p[1] for p in polys],
            "pi": [p[2] for p in polys], "beta": ch[0], "gamma": ch[1], "alpha": ch[2], "wires_ext": small(M, WIRES, big), "z_ext": small(M, big),
            "pi_ext": small(M, big)}


def lift(tree, largest):
    """v + j r for every value of a nested list: another word for the same element of Fr"""
    if isinstance(tree, list):
        return [lift(t, largest) for t in tree]
    return tree + ((TOP - tree) // R if largest else 1 + tree % ((TOP - tree) // R)) * R


def words(rows):
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


def drive(eng, b):
    """every entry point once, the default form and the tuned one, with and without public inputs: the list of every output"""
    table = eng.plonk_quotient_prepare(words(b["selectors"]), words(b["sigma"]), LOG_E)
    out = list(eng.plonk_quotient_table_down(table, WIRES, LOG_N, LOG_E))
    scalars = (limbs(b["shifts"]), limbs(b["beta"]), limbs(b["gamma"]), limbs(b["alpha"]), LOG_N, LOG_E)
    for pins in ({}, {"max_blocks": 1}):
        for with_pi in (True, False):
            out.append(eng.plonk_quotient_evals(table, words(b["wires_ext"]), words(b["z_ext"]), words(b["pi_ext"]) if with_pi else None, *scalars, **pins))
            out += list(eng.plonk_quotient(table, words(b["wires"]), words(b["z"]), words(b["pi"]) if with_pi else None, *scalars, **pins))
    return [np.asarray(o) for o in out]


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_representatives_give_the_same_bytes(engine, largest):
    b = batch()
    base = drive(engine, b)
    lifted = {k: lift(v, largest) for k, v in b.items()}
    assert min(lifted["alpha"]) >= R and min(min(r) for r in lifted["selectors"]) >= R
    T._same(drive(engine, lifted), base, "v + j r")
    rows, zinv = Q.table(b["selectors"], b["sigma"], LOG_N, LOG_E)
    want = [Q.quotient(rows, zinv, b["wires"][s], b["z"][s], b["pi"][s], b["shifts"], b["beta"][s], b["gamma"][s], b["alpha"][s], LOG_N, LOG_E) for s in range(M)]
    t, status = base[3:5]                                            # after the table's two parts and the first fused call
    assert np.array_equal(t, words([w for w, _ in want])) and list(status) == [s for _, s in want] == [0, 1]


class GuardedQuotient(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


@pytest.mark.gpu
def test_every_entry_point_stays_inside_its_buffers_and_writes_its_outputs(engine):
    b = batch()
    guarded = GuardedQuotient(engine.device, engine.stream)
    outs, raw = [], []
    for fill in FILLS:
        guarded.fill = fill
        del guarded.written[:]
        outs.append(drive(guarded, b))                              # every call audited inside: guard bands, const inputs, @shape extents
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
    T._same(outs[0], drive(engine, b), "the guarded engine against the plain engine")


@pytest.mark.gpu
def test_argument_errors_write_nothing(engine):
    lib, st = engine.lib, engine.stream
    log_n, log_e, W, m = 3, 2, 2, 2
    n, big = 1 << log_n, 1 << (log_n + log_e)
    table_words = 4 * big * (2 * W + 3) + 4 * (1 << log_e)
    fill = np.full(table_words + 64, SENTINEL, dtype=np.uint64)       # every array is as large as the largest
    arrays = {k: engine.to_device(fill) for k in ("table", "sel", "sig", "wires", "z", "pi", "sh", "be", "ga", "al", "out")}
    status = engine.to_device(np.full(8, 0x5A, dtype=np.uint8))
    p = {k: d.ptr for k, d in arrays.items()}
    bad = lambda rc: rc == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    prep = lambda sel, sig, lg, le, w, tab: lib.sylow_plonk_quotient_prepare(sel, sig, lg, le, w, tab, st)
    evals = lambda *a: lib.sylow_plonk_quotient_evals_batch(*a, st)
    evals_t = lambda mb: lib.sylow_plonk_quotient_evals_batch_tuned(*ev_full[:12], mb, ev_full[12], st)
    full = lambda *a: lib.sylow_plonk_quotient_batch(*a, st)
    full_t = lambda mb: lib.sylow_plonk_quotient_batch_tuned(*fu_full[:14], mb, *fu_full[14:], st)
    ev_full = [p["table"], p["wires"], p["z"], p["pi"], p["sh"], p["be"], p["ga"], p["al"], log_n, log_e, W, m, p["out"]]
    fu_full = [p["table"], p["wires"], n, p["z"], n, p["pi"], p["sh"], p["be"], p["ga"], p["al"], log_n, log_e, W, m, p["out"], status.ptr]
    sub = lambda lst, **kw: [kw.get("i%d" % k, v) for k, v in enumerate(lst)]
    # NULL where an array is required (pi and pi_ext may be NULL)
    assert bad(prep(None, p["sig"], log_n, log_e, W, p["table"])) and bad(prep(p["sel"], None, log_n, log_e, W, p["table"])) and bad(prep(p["sel"], p["sig"], log_n, log_e, W, None))
    for i in (0, 1, 2, 4, 5, 6, 7, 12):
        assert bad(evals(*[None if k == i else v for k, v in enumerate(ev_full)])), i
    for i in (0, 1, 3, 6, 7, 8, 9, 14, 15):
        assert bad(full(*[None if k == i else v for k, v in enumerate(fu_full)])), i
    # log_n, log_e and W out of range; the pin
    dims = ((-1, log_e, W), (log_n, -1, W), (27, 2, W), (29, 0, W), (0, 29, W), (log_n, log_e, 1), (log_n, log_e, 0), (log_n, log_e, 33), (log_n, log_e, -1))
    for lg, le, w in dims:
        assert bad(prep(p["sel"], p["sig"], lg, le, w, p["table"])), (lg, le, w)
        assert bad(evals(*sub(ev_full, i8=lg, i9=le, i10=w))) and bad(full(*sub(fu_full, i10=lg, i11=le, i12=w))), (lg, le, w)
        assert bad(evals(*sub(ev_full, i8=lg, i9=le, i10=w, i11=0))) and bad(full(*sub(fu_full, i10=lg, i11=le, i12=w, i13=0))), "refused whatever m is"
    assert bad(evals_t(0)) and bad(full_t(0))
    # the lengths: outside 1 .. N, and D - n >= N (W = 2, n = 8, N = 32: len_z - 1 + 2 (len_w - 1) - 8 >= 32 from len_z = 27 on at len_w = 8)
    for lw, lz in ((0, n), (n, 0), (big + 1, n), (n, big + 1), (n, 27), (big, n), (20, 20)):
        assert bad(full(*sub(fu_full, i2=lw, i4=lz))), (lw, lz)
    assert Q.args_ok(log_n, log_e, W, n, 26) and not Q.args_ok(log_n, log_e, W, n, 27) and not Q.args_ok(log_n, log_e, W, 20, 20)
    # an output that overlaps an input or another output, by byte ranges
    t_bytes = 32 * big * m
    assert bad(prep(p["sel"], p["sig"], log_n, log_e, W, p["sel"])) and bad(prep(p["sel"], p["sig"], log_n, log_e, W, p["sig"] + 8))
    assert bad(prep(p["sel"], p["sig"], log_n, log_e, W, p["sel"] - 8 * table_words + 8))
    for k in range(8):                                           # t_ext_out over every input
        assert bad(evals(*sub(ev_full, i12=ev_full[k]))) and bad(evals(*sub(ev_full, i12=ev_full[k] - t_bytes + 8))), k
    for k in (0, 1, 3, 5, 6, 7, 8, 9):                           # t_out and status over every input; status inside t_out
        assert bad(full(*sub(fu_full, i14=fu_full[k]))) and bad(full(*sub(fu_full, i15=fu_full[k] + 3))), k
    assert bad(full(*sub(fu_full, i15=p["out"]))) and bad(full(*sub(fu_full, i15=p["out"] + t_bytes - 1)))
    # m = 0: OK, nothing launched, whatever the pointers
    assert evals(*([None] * 8), log_n, log_e, W, 0, None) == 0 and full(None, None, n, None, n, None, None, None, None, None, log_n, log_e, W, 0, None, None) == 0
    engine.sync()
    for k, d in arrays.items():
        assert np.array_equal(d.download(), fill), f"{k}: nothing written"
    assert (status.download() == 0x5A).all()
    # the largest legal len_z runs, and writes every status byte of the batch and no other
    assert full(*sub(fu_full, i4=26)) == 0
    engine.sync()
    assert (status.download()[:m] <= 1).all() and (status.download()[m:] == 0x5A).all()
