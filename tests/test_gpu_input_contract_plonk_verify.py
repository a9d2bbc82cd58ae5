"""The input and memory contract for the entry points of include/sylow_pverify.h (plonk_verify.hip).  They are declared in a header of their
own, under a prefix of their own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror
include/sylow_hip.h.

  * Every scalar (evaluations, public inputs, shifts, the six challenges and the weights) as v and as v + j r: the same bytes out.
  * Every entry point runs between guard bands under two fill bytes (tests/guarded_engine.py, imported and subclassed: the prototypes of
    the new header are added to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte
    left unwritten -- the bytes of every output are the same under both fills and equal the plain engine's.  NULL pub with n_pub = 0 runs.
  * Every SYLOW_HIP_E_ARG case of the header, with nothing written, and the refusal when the scratch limit does not hold one proof."""
import random
import re

import numpy as np
import pytest

import kzg_model as K
import plonk_verify_model as V
import test_gpu_input_contract as T
from groth16_model import g2_gen_mul, limbs
from guarded_engine import FILLS, GuardedEngine
from test_pverify_header import HEADER

R = V.R
TOP = (1 << 256) - 1
E_HIP, E_ARG = -1, -2
LOG_N, LOG_E, WIRES, PROOFS, PUBLIC = 3, 2, 3, 2, 3
SENTINEL = 0x5A5A5A5A5A5A5A5A
OUTPUTS = ("k_out", "y_out", "status", "c_xy", "c_inf", "pi_xy", "pi_inf", "ok", "gt_out", "is_one")


def prototypes():
    """{entry point: [(is a pointer, const, name)]} of the new header"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(sylow_pverify_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = [("*" in p, "const" in p.split(), p.replace("*", " ").split()[-1]) for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_outputs_are_the_non_const_pointers():
    protos = prototypes()
    assert len(protos) == 5 and not set(protos) & set(T.CONTRACT), "include/sylow_hip.h does not declare them"
    for name, params in protos.items():
        pointers = [p for p in params if p[0] and p[2] != "stream"]
        assert all(p[1] == (p[2] not in OUTPUTS) for p in pointers) and any(not p[1] for p in pointers), name


def batch():
    """values below r >> 3, so that v + j r has room; points with known logarithms, the identity flagged at [q_C] and at one W_omega"""
    rng = random.Random(T.SEED + 0x9109)
    small = lambda *shape: [small(*shape[1:]) for _ in range(shape[0])] if len(shape) > 1 else [rng.randrange(R >> 3) for _ in range(shape[0])]
    b = {"evals": small(PROOFS, 2 * WIRES + 1), "pub": small(PROOFS, PUBLIC), "shifts": small(WIRES), "weights": small(PROOFS)}
    for k in V.CHALLENGES:
        b[k] = small(PROOFS)
    P = V.proof_points(WIRES, LOG_E)
    vk_xy, vk_inf = V.points([0 if c == WIRES + 1 else rng.randrange(1, R) for c in range(V.key_points(WIRES))])
    vk_xy[WIRES + 1] = K.GARBAGE
    pr_xy, pr_inf = V.points([rng.randrange(1, R) for _ in range(PROOFS * P)])
    pr_xy, pr_inf = pr_xy.reshape(PROOFS, P, 8).copy(), pr_inf.reshape(PROOFS, P).copy()
    pr_xy[1, P - 1], pr_inf[1, P - 1] = K.GARBAGE, 1
    return b, {"vk": (vk_xy, vk_inf), "proofs": pr_xy, "proof_inf": pr_inf, "tau_g2": g2_gen_mul([V.TAU])[0]}


def lift(tree, largest):
    """v + j r for every value of a nested list: another word for the same element of Fr"""
    if isinstance(tree, list):
        return [lift(t, largest) for t in tree]
    return tree + ((TOP - tree) // R if largest else 1 + tree % ((TOP - tree) // R)) * R


def words(rows):
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


def drive(eng, b, pts):
    """every entry point once, the scalars in the default form and the tuned one, every call with and without public inputs: the list of
    every output"""
    ch = [limbs(b[k]) for k in V.CHALLENGES]
    out = []
    for pub in (words(b["pub"]), None):
        for pins in ({}, {"max_blocks": 1}):
            out += list(eng.plonk_verify_scalars(words(b["evals"]), pub, limbs(b["shifts"]), *ch, LOG_N, LOG_E, **pins))
        common = (pts["vk"], pts["proofs"], words(b["evals"]), pub, limbs(b["shifts"]), *ch)
        (c, ci), (p, pi), y, status = eng.plonk_verify_fold(*common, LOG_N, LOG_E, proof_inf=pts["proof_inf"])
        out += [c, ci, p, pi, y, status]
        out += list(eng.plonk_verify(pts["tau_g2"], *common, LOG_N, LOG_E, proof_inf=pts["proof_inf"]))
        gt, one, status = eng.plonk_batch_verify_weighted(pts["tau_g2"], *common, limbs(b["weights"]), LOG_N, LOG_E, proof_inf=pts["proof_inf"])
        out += [gt, np.array([one]), status]
    return [np.asarray(o) for o in out]


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_representatives_give_the_same_bytes(engine, largest):
    b, pts = batch()
    base = drive(engine, b, pts)
    lifted = {k: lift(v, largest) for k, v in b.items()}
    assert min(lifted["u"]) >= R and min(min(r) for r in lifted["evals"]) >= R and min(lifted["weights"]) >= R
    T._same(drive(engine, lifted, pts), base, "v + j r")
    want = [V.scalars(b["evals"][i], b["pub"][i], b["shifts"], *(b[k][i] for k in V.CHALLENGES), LOG_N, LOG_E) for i in range(PROOFS)]
    assert np.array_equal(base[0], words([w[0] for w in want])) and np.array_equal(base[1], limbs([w[1] for w in want])) and list(base[2]) == [w[2] for w in want]


class GuardedVerifier(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


@pytest.mark.gpu
def test_every_entry_point_stays_inside_its_buffers_and_writes_its_outputs(engine):
    b, pts = batch()
    guarded = GuardedVerifier(engine.device, engine.stream)
    outs, raw = [], []
    for fill in FILLS:
        guarded.fill = fill
        del guarded.written[:]
        outs.append(drive(guarded, b, pts))                         # every call audited inside: guard bands, const inputs, @shape extents
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
    T._same(outs[0], drive(engine, b, pts), "the guarded engine against the plain engine")


@pytest.mark.gpu
def test_argument_errors_write_nothing(engine):
    lib, st = engine.lib, engine.stream
    log_n, log_e, W, m, n_pub = LOG_N, LOG_E, WIRES, PROOFS, PUBLIC
    T_, P = V.terms(W, log_e), V.proof_points(W, log_e)
    fill = np.full(8 * P * m + 64, SENTINEL, dtype=np.uint64)       # every array is as large as the largest
    keys = ("tau", "vk", "pr", "ev", "pub", "sh", "be", "ga", "al", "ze", "v", "u", "w", "k", "y", "c", "pi", "gt")
    arrays = {k: engine.to_device(fill) for k in keys}
    flags = {k: engine.to_device(np.full(64, 0x5A, dtype=np.uint8)) for k in ("vki", "pri", "status", "ci", "pii", "ok", "one")}
    p = {k: d.ptr for k, d in list(arrays.items()) + list(flags.items())}
    bad = lambda rc: rc == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    sub = lambda lst, **kw: [kw.get("i%d" % k, v) for k, v in enumerate(lst)]
    ins = [p["ev"], p["pub"], n_pub, p["sh"], p["be"], p["ga"], p["al"], p["ze"], p["v"], p["u"]]
    pts = [p["vk"], p["vki"], p["pr"], p["pri"]]
    dims = [log_n, log_e, W, m]
    sc_full = ins + dims + [p["k"], p["y"], p["status"]]                                         # dims at 10 .. 13, outputs at 14 .. 16
    fo_full = pts + ins + dims + [p["c"], p["ci"], p["pi"], p["pii"], p["y"], p["status"]]        # ins at 4 .. 13, dims at 14 .. 17, outputs at 18 .. 23
    ve_full = [p["tau"]] + pts + ins + dims + [p["ok"], p["status"]]                               # ins at 5 .. 14, dims at 15 .. 18, outputs at 19, 20
    we_full = [p["tau"]] + pts + ins + [p["w"]] + dims + [p["gt"], p["one"], p["status"]]          # weights at 15, dims at 16 .. 19, outputs at 20 .. 22
    sc = lambda *a: lib.sylow_pverify_scalars_batch(*a, st)
    sc_t = lambda mb: lib.sylow_pverify_scalars_batch_tuned(*sc_full[:14], mb, *sc_full[14:], st)
    fo = lambda *a: lib.sylow_pverify_fold_batch(*a, st)
    ve = lambda *a: lib.sylow_pverify_verify_batch(*a, st)
    we = lambda *a: lib.sylow_pverify_batch_verify_weighted(*a, st)
    calls = ((sc, sc_full, 0, 10), (fo, fo_full, 4, 14), (ve, ve_full, 5, 15), (we, we_full, 5, 16))       # (call, arguments, first of ins, first of dims)
    # NULL where an array is required (vk_inf and proof_inf may be NULL; pub only with n_pub = 0; gt_out or is_one, not both)
    for call, full, i0, d0 in calls:
        required = [i0 + k for k in (0, 1, 3, 4, 5, 6, 7, 8, 9)] + [k for k in range(len(full)) if k >= d0 + 4 or (k < i0 and k not in (i0 - 3, i0 - 1))]
        if call is we:
            required = [k for k in required if k not in (20, 21)] + [15]
        for i in required:
            assert bad(call(*[None if k == i else v for k, v in enumerate(full)])), (len(full), i)
    assert bad(we(*sub(we_full, i20=None, i21=None)))
    # log_n, log_e and W out of range and n_pub above n, whatever m is; the pin
    for call, full, i0, d0 in calls:
        for lg, le, w in ((-1, log_e, W), (log_n, -1, W), (27, 2, W), (29, 0, W), (0, 29, W), (log_n, log_e, 1), (log_n, log_e, 33), (log_n, log_e, -1)):
            for mm in (m, 0):
                assert bad(call(*sub(full, **{"i%d" % d0: lg, "i%d" % (d0 + 1): le, "i%d" % (d0 + 2): w, "i%d" % (d0 + 3): mm}))), (lg, le, w, mm)
        for mm in (m, 0):
            assert bad(call(*sub(full, **{"i%d" % (i0 + 2): (1 << log_n) + 1, "i%d" % (d0 + 3): mm}))), "n_pub above n"
    assert bad(sc_t(0))
    # an output that overlaps an input or another output, by byte ranges
    for call, full, i0, d0 in calls:
        outputs = range(d0 + 4, len(full))
        inputs = [k for k in range(d0) if k != i0 + 2]
        for o in outputs:
            for k in inputs:                                      # one byte in: the shortest input, vk_inf, has 2 W + 2 bytes
                assert bad(call(*sub(full, **{"i%d" % o: full[k] + 1}))), (len(full), o, k)
        for o in list(outputs)[1:]:
            assert bad(call(*sub(full, **{"i%d" % o: full[d0 + 4] + 1}))), (len(full), o)
    assert bad(sc(*sub(sc_full, i14=p["ev"] - 32 * T_ * m + 8))) and bad(sc(*sub(sc_full, i15=p["k"] + 32 * T_ * m - 8)))
    # the scratch limit does not hold one proof of the fold: refused before anything is enqueued
    try:
        engine.set_scratch_limit(64)
        assert fo(*fo_full) == E_HIP and b"does not hold one proof" in lib.sylow_hip_last_error()
        assert ve(*ve_full) == E_HIP and b"does not hold one proof" in lib.sylow_hip_last_error()
    finally:
        engine.set_scratch_limit(0)
    # m = 0: OK, nothing launched, whatever the pointers
    assert sc(*([None, None, 0] + [None] * 7 + [log_n, log_e, W, 0, None, None, None])) == 0
    assert fo(*([None] * 4 + [None, None, 0] + [None] * 7 + [log_n, log_e, W, 0] + [None] * 6)) == 0
    assert ve(*([None] * 5 + [None, None, 0] + [None] * 7 + [log_n, log_e, W, 0, None, None])) == 0
    engine.sync()
    for k, d in arrays.items():
        assert np.array_equal(d.download(), fill), f"{k}: nothing written"
    for k, d in flags.items():
        assert (d.download() == 0x5A).all(), k
    # NULL pub with n_pub = 0 is accepted, and writes every status byte of the batch and no other
    assert sc(*sub(sc_full, i1=None, i2=0)) == 0
    engine.sync()
    assert (flags["status"].download()[:m] <= 2).all() and (flags["status"].download()[m:] == 0x5A).all()
    # the weighted call at m = 0 yields the identity
    assert we(*([None] * 5 + [None, None, 0] + [None] * 8 + [log_n, log_e, W, 0, p["gt"], p["one"], None])) == 0
    engine.sync()
    assert flags["one"].download()[0] == 1 and arrays["gt"].download()[0] == 1
