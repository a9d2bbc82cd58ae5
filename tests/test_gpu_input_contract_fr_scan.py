"""The input and memory contract for the entry points of include/sylow_hip_fr_scan.h (fr_scan.hip).  They are declared in a header of their
own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror include/sylow_hip.h.

  * Every scalar (elements, numerators, denominators, wires, sigma, shifts, beta, gamma) as v and as v + j r: the same bytes out.
  * Every entry point runs between guard bands under two fill bytes (tests/guarded_engine.py, with the prototypes of the new header added
    to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte left unwritten -- the bytes
    of every output are the same under both fills and equal the plain engine's.
  * Every SYLOW_HIP_E_ARG case of the header, with nothing written."""
import random
import re

import numpy as np
import pytest

import fr_scan_model as M
import test_gpu_input_contract as T
from groth16_model import ints, limbs
from guarded_engine import FILLS, GuardedEngine
from test_fr_scan_header import HEADER

R = M.R
TOP = (1 << 256) - 1
E_ARG = -2
CH = M.plan_constants()["SCAN_CHUNK"]
LEN, ROWS, LOG_N, WIRES = CH + 9, 2, 3, 3                 # two chunks: the three phases and the scratch; one chunk through the permutation
SENTINEL = 0x5A5A5A5A5A5A5A5A


def prototypes():
    """{entry point: [(is a pointer, const, name)]} of the new header"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [("*" in p, "const" in p.split(), p.replace("*", " ").split()[-1]) for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_outputs_are_the_non_const_pointers():
    protos = prototypes()
    assert len(protos) == 7 and not set(protos) & set(T.CONTRACT), "include/sylow_hip.h does not declare them"
    for name, params in protos.items():
        assert all(p[1] == (p[2] not in ("out", "total_out", "status", "z_out")) for p in params if p[0] and p[2] != "stream"), name


def batch():
    """values below r: rows of the scans, and one PLONK instance pair over a random permutation"""
    rng = random.Random(T.SEED + 0x5CA)
    rows = lambda: [[rng.randrange(1, R >> 3) for _ in range(LEN)] for _ in range(ROWS)]
    n = 1 << LOG_N
    mapping = list(range(WIRES * n))
    rng.shuffle(mapping)
    shifts = [1, 5, 7]
    return {"a": rows(), "num": rows(), "den": rows(), "shifts": shifts, "sigma": M.sigma_from_mapping(shifts, LOG_N, mapping),
            "wires": [M.satisfying_wires(mapping, WIRES, LOG_N, rng), [[rng.randrange(R >> 3) for _ in range(n)] for _ in range(WIRES)]],
            "beta": [rng.randrange(R >> 3) for _ in range(2)], "gamma": [rng.randrange(R >> 3) for _ in range(2)]}


def lift(tree, largest):
    """v + j r for every value of a nested list: another word for the same element of Fr"""
    if isinstance(tree, list):
        return [lift(t, largest) for t in tree]
    return tree + ((TOP - tree) // R if largest else 1 + tree % ((TOP - tree) // R)) * R


def words(rows):
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


def drive(eng, b):
    """every entry point once, the default form and the tuned one: the list of every output"""
    out = []
    for pins in ({}, {"max_blocks": 1, "totals_tile": 1}):
        for op in (M.SUM, M.PRODUCT):
            out += list(eng.fr_scan(words(b["a"]), op, op == M.SUM, **pins))
            out += list(eng.fr_ratio_scan(words(b["num"]), words(b["den"]), op, **pins))
        out += list(eng.plonk_permutation(words(b["wires"]), words(b["sigma"]), limbs(b["shifts"]), limbs(b["beta"]), limbs(b["gamma"]), **pins))
    out += list(eng.fr_ratio_scan(None, words(b["den"]), M.PRODUCT))
    out.append(eng.plonk_identity(limbs(b["shifts"]), LOG_N))
    return [np.asarray(o) for o in out]


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_representatives_give_the_same_bytes(engine, largest):
    b = batch()
    base = drive(engine, b)
    lifted = {k: lift(v, largest) for k, v in b.items()}
    assert min(lifted["beta"]) >= R and min(min(r) for r in lifted["den"]) >= R
    T._same(drive(engine, lifted), base, "v + j r")
    want = M.permutation(b["wires"][0], b["sigma"], b["shifts"], b["beta"][0], b["gamma"][0], LOG_N)
    z, total, status = base[10:13]                                   # after the two scans and the two ratio scans of the default form
    assert np.array_equal(z[0], limbs(want[0])) and list(status) == [0, 2] and ints(total[:1]) == [1]


class GuardedScan(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


@pytest.mark.gpu
def test_every_entry_point_stays_inside_its_buffers_and_writes_its_outputs(engine):
    b = batch()
    guarded = GuardedScan(engine.device, engine.stream)
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
    n, m, log_n, W = 8, 2, 3, 2
    fill = np.full((m * W, 4, n), SENTINEL, dtype=np.uint64)
    arrays = {k: engine.to_device(fill) for k in ("a", "b", "out", "tot", "sig", "sh", "be", "ga")}
    status = engine.to_device(np.full(8, 0x5A, dtype=np.uint8))
    p = {k: d.ptr for k, d in arrays.items()}
    bad = lambda rc: rc == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    scan = lambda a, ln, mm, op, ex, out, tot: lib.sylow_hip_fr_scan_batch(a, ln, mm, op, ex, out, tot, st)
    scan_t = lambda mb, tile: lib.sylow_hip_fr_scan_batch_tuned(p["a"], n, m, 1, 0, mb, tile, p["out"], p["tot"], st)
    ratio = lambda num, den, ln, mm, op, out, tot, s: lib.sylow_hip_fr_ratio_scan_batch(num, den, ln, mm, op, out, tot, s, st)
    ratio_t = lambda mb, tile: lib.sylow_hip_fr_ratio_scan_batch_tuned(p["a"], p["b"], n, m, 1, mb, tile, p["out"], p["tot"], status.ptr, st)
    ident = lambda sh, lg, w, out: lib.sylow_hip_plonk_identity_batch(sh, lg, w, out, st)
    perm = lambda wi, sg, sh, be, ga, lg, w, mm, z, tot, s: lib.sylow_hip_plonk_permutation_batch(wi, sg, sh, be, ga, lg, w, mm, z, tot, s, st)
    perm_t = lambda mb, tile: lib.sylow_hip_plonk_permutation_batch_tuned(p["a"], p["sig"], p["sh"], p["be"], p["ga"], log_n, W, m, mb, tile, p["out"], p["tot"],
                                                                        status.ptr, st)
    size = 32 * n * m
    # NULL where an array is required; len = 0; op and exclusive out of range; the pins
    assert bad(scan(None, n, m, 1, 0, p["out"], p["tot"])) and bad(scan(p["a"], n, m, 1, 0, None, p["tot"])) and bad(scan(p["a"], 0, m, 1, 0, p["out"], p["tot"]))
    assert bad(scan(p["a"], 0, 0, 1, 0, p["out"], None)), "len = 0 is refused whatever m is"
    assert all(bad(scan(p["a"], n, m, op, ex, p["out"], p["tot"])) for op, ex in ((2, 0), (-1, 0), (0, 2), (1, -1)))
    assert bad(scan_t(0, -1)) and bad(scan_t(-1, 0)) and bad(scan_t(-1, 257)) and bad(ratio_t(0, -1)) and bad(ratio_t(-1, 0)) and bad(ratio_t(1, 257))
    assert bad(ratio(p["a"], None, n, m, 1, p["out"], p["tot"], status.ptr)) and bad(ratio(p["a"], p["b"], n, m, 1, None, p["tot"], status.ptr))
    assert bad(ratio(p["a"], p["b"], n, m, 1, p["out"], p["tot"], None)) and bad(ratio(p["a"], p["b"], 0, m, 1, p["out"], p["tot"], status.ptr))
    assert bad(ratio(p["a"], p["b"], n, m, 2, p["out"], p["tot"], status.ptr)) and bad(ratio(p["a"], p["b"], n, m, -1, p["out"], p["tot"], status.ptr))
    assert bad(ident(None, log_n, W, p["out"])) and bad(ident(p["sh"], log_n, W, None))
    assert all(bad(ident(p["sh"], lg, w, p["out"])) for lg, w in ((-1, W), (29, W), (log_n, 0), (log_n, 33), (log_n, -1)))
    full = [p["a"], p["sig"], p["sh"], p["be"], p["ga"], log_n, W, m, p["out"], p["tot"], status.ptr]
    for i in (0, 1, 2, 3, 4, 8, 10):                             # every required array of the permutation entry
        assert bad(perm(*[None if k == i else v for k, v in enumerate(full)])), i
    for lg, w in ((-1, W), (29, W), (log_n, 0), (log_n, 33)):
        assert bad(perm(*(full[:5] + [lg, w] + full[7:]))), (lg, w)
    assert bad(perm_t(0, -1)) and bad(perm_t(-1, 0)) and bad(perm_t(-1, 257))
    # an output that overlaps an input or another output, by byte ranges
    for off in (0, 32, size - 8, -(size - 8)):
        base = p["a"] + size if off < 0 else p["a"]
        assert bad(scan(base, n, m, 1, 0, base + off, p["tot"])), off
        assert bad(ratio(p["b"], base, n, m, 1, base + off, p["tot"], status.ptr)) and bad(ratio(base, p["b"], n, m, 0, base + off, p["tot"], status.ptr)), off
    assert bad(scan(p["a"], n, m, 1, 0, p["out"], p["out"] + size - 8)) and bad(scan(p["a"], n, m, 1, 0, p["out"], p["a"] + 8)), "total_out inside out / inside a"
    assert bad(ratio(p["a"], p["b"], n, m, 1, p["out"], p["tot"], p["out"] + 3)) and bad(ratio(p["a"], p["b"], n, m, 1, p["out"], p["tot"], p["tot"] + 63))
    assert bad(ident(p["sh"], log_n, W, p["sh"] + 32)) and bad(ident(p["sh"], log_n, W, p["sh"]))
    for k in (0, 1, 2, 3, 4):                                    # z_out over every input; total_out and status inside z_out
        assert bad(perm(*(full[:8] + [full[k]] + full[9:]))), k
    assert bad(perm(*(full[:9] + [p["out"] + 8, status.ptr]))) and bad(perm(*(full[:10] + [p["out"] + 5])))
    # m = 0: OK, nothing launched, whatever the pointers
    assert scan(None, n, 0, 1, 0, None, None) == 0 and ratio(None, None, n, 0, 0, None, None, None) == 0
    assert perm(None, None, None, None, None, log_n, W, 0, None, None, None) == 0
    engine.sync()
    for k, d in arrays.items():
        assert np.array_equal(d.download(), fill), f"{k}: nothing written"
    assert (status.download() == 0x5A).all()
    # adjacent halves of one allocation do not overlap: the call runs
    assert scan(p["a"], n, 1, 0, 0, p["a"] + 32 * n, None) == 0
    engine.sync()
    got = arrays["a"].download()
    v = int.from_bytes(np.full(4, SENTINEL, dtype=np.uint64).tobytes(), "little") % R
    assert np.array_equal(got[0], fill[0]) and np.array_equal(np.ascontiguousarray(got[1].T), limbs([v * (k + 1) % R for k in range(n)]))
