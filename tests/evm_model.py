"""A byte-level model of the three alt_bn128 precompiles and a generator of batch jobs with named defect classes.  CPU only.

The model is written from the reference adapter's behaviour (examples/reth_bn128.rs:99-217) and EIP-196 / EIP-197, on oracle/pyref.py
integers.  It shares nothing with sylow_amd/evm.py (never import that module here): it is the judge of that module and of the kernels
behind it (tests/test_gpu_evm_batches.py), after tests/test_evm_model.py has pinned it to the reference's own test vectors.

model_add / model_mul / model_pair return a Result: `out` (the output bytes) or `error` (one of the reference's four Error names), and
`status`, the raw per-element status of the C ABI (include/sylow_hip.h SYLOW_HIP_ST_*) for the defect that decides the error -- the one
the reference's `?` meets first.  Host-side errors (gas, length) carry no status: they never reach the device.

Two documented differences from the reference adapter are part of the model:
  * identity pairs of an ecPairing job are skipped, as EIP-197 requires (the reference adapter inherits glued_pairing's Q = identity
    defect and answers false there: SURVEY.md N5, include/sylow_hip.h above sylow_hip_evm_ecadd_batch);
  * ecMul takes any 256-bit scalar and reduces it mod r, as EIP-196 specifies (the reference unwraps Fr::from_be_bytes and would panic
    for a scalar >= r, reth_bn128.rs:150).
"""
from collections import Counter, namedtuple

import numpy as np

from helpers import P, SEED, Xoshiro, crafted_g1_points, fp2_sqrt, limbs
from oracle import pyref as R

OUT_OF_GAS = "OutOfGas"
NOT_A_MEMBER = "Bn128FieldPointNotAMember"
FAILED_TO_CREATE = "Bn128AffineGFailedToCreate"
PAIR_LENGTH = "Bn128PairLength"
ST_OK, ST_NOT_ON_CURVE, ST_NOT_IN_SUBGROUP, ST_DECODE_ERROR = 0, 1, 2, 4          # include/sylow_hip.h
ERROR_OF_STATUS = {ST_DECODE_ERROR: NOT_A_MEMBER, ST_NOT_ON_CURVE: FAILED_TO_CREATE, ST_NOT_IN_SUBGROUP: FAILED_TO_CREATE}
ADD_GAS, MUL_GAS, PAIR_PER_POINT, PAIR_BASE = 500, 40_000, 80_000, 100_000        # Byzantium costs, the ones reth_bn128.rs:229-502 tests with
NO_GAS_LIMIT = 1 << 62
r = R.R_ORDER
U256_MAX = (1 << 256) - 1

Result = namedtuple("Result", "out error status")


def _fail(status):
    return Result(None, ERROR_OF_STATUS[status], status)


def right_pad(b, n):
    """right_pad::<N>: zeros appended up to N bytes, anything beyond N dropped"""
    return bytes(b[:n]) + bytes(max(0, n - len(b)))


def _word(b, k):
    return int.from_bytes(b[32 * k:32 * k + 32], "big")


def _g1(x, y):
    """read_point after both reads succeeded + new_g1_point (reth_bn128.rs:117-125) -> (status, projective point)"""
    if x == 0 and y == 0:
        return ST_OK, R.proj_zero(R.F1)
    if not R.g1_is_on_curve_affine(x, y):
        return ST_NOT_ON_CURVE, None
    return ST_OK, (x, y, 1)


def _read_point(b):
    """read_point (reth_bn128.rs:110-114): x, then y (each must be < p), then the curve"""
    x, y = _word(b, 0), _word(b, 1)
    if x >= P or y >= P:
        return ST_DECODE_ERROR, None
    return _g1(x, y)


_G2_CACHE = {}


def _g2(x, y):
    """reth_bn128.rs:197-207: (0, 0) is the identity, else G2Projective::new (on the twist, then in the r-torsion, g2.rs:460-525)"""
    if x == (0, 0) and y == (0, 0):
        return ST_OK, None
    key = (x, y)
    if key not in _G2_CACHE:
        if not R.g2_is_on_curve_affine(x, y):
            _G2_CACHE[key] = ST_NOT_ON_CURVE
        else:
            _G2_CACHE[key] = ST_OK if R.g2_projective_new((x, y, R.FP2_ONE)) == "ok" else ST_NOT_IN_SUBGROUP
    return _G2_CACHE[key], (x, y)


def _g1_bytes(pt):
    return R.g1_to_be_bytes_scrubbed(R.affine_from_proj(R.F1, pt))


def model_add(data, gas_cost=ADD_GAS, gas_limit=ADD_GAS):
    """run_add, reth_bn128.rs:127-138: gas, padding, ALL of point 1 (both reads, then the curve), only then point 2"""
    if gas_cost > gas_limit:
        return Result(None, OUT_OF_GAS, None)
    b = right_pad(data, 128)
    s1, p1 = _read_point(b[:64])
    if s1:
        return _fail(s1)
    s2, p2 = _read_point(b[64:])
    if s2:
        return _fail(s2)
    return Result(_g1_bytes(R.proj_add(R.F1, p1, p2)), None, ST_OK)


def model_mul(data, gas_cost=MUL_GAS, gas_limit=MUL_GAS):
    """run_mul, reth_bn128.rs:140-154; the scalar never fails: any 256-bit value, reduced mod r (EIP-196; see the module text)"""
    if gas_cost > gas_limit:
        return Result(None, OUT_OF_GAS, None)
    b = right_pad(data, 96)
    s1, p1 = _read_point(b[:64])
    if s1:
        return _fail(s1)
    return Result(_g1_bytes(R.proj_scalar_mul(R.F1, p1, _word(b, 2) % r)), None, ST_OK)


def _decode_pairs(data, per_point, base, gas_limit):
    """run_pair up to the pairing itself (reth_bn128.rs:162-210) -> a Result for a rejected input, else the list of the job's
    non-identity pairs ((x, y), ((x0, x1), (y0, y1)))"""
    if (len(data) // 192) * per_point + base > gas_limit:
        return Result(None, OUT_OF_GAS, None)
    if len(data) % 192:
        return Result(None, PAIR_LENGTH, None)
    pairs = []
    for i in range(len(data) // 192):
        e = data[192 * i:192 * i + 192]
        ax, ay, bay, bax, bby, bbx = (_word(e, k) for k in range(6))            # the six reads, every one before either point
        if max(ax, ay, bay, bax, bby, bbx) >= P:
            return _fail(ST_DECODE_ERROR)
        s1, a = _g1(ax, ay)                                                     # G1 before G2
        if s1:
            return _fail(s1)
        s2, q = _g2((bax, bay), (bbx, bby))
        if s2:
            return _fail(s2)
        if q is not None and a[2] != 0:                                         # EIP-197: an identity on either side contributes one
            pairs.append(((a[0], a[1]), q))
    return pairs


def _products_are_one(jobs):
    """for every list of non-identity pairs: is the product of its pairings one?  One call of the C oracle's glued_pairing"""
    from oracle import coracle as C
    todo = [j for j in {tuple(j): j for j in jobs if j and tuple(j) not in _PRODUCT_CACHE}.values()]
    if todo:
        for j, one in zip(todo, _oracle_products(C, todo)):
            _PRODUCT_CACHE[tuple(j)] = one
    return [not j or _PRODUCT_CACHE[tuple(j)] for j in jobs]


_PRODUCT_CACHE = {}


def _oracle_products(C, jobs):
    flat = [pq for j in jobs for pq in j]
    p = limbs([v for (a, _) in flat for v in (a[0], a[1], 1)]).reshape(-1, 12)
    q = limbs([v for (_, (x, y)) in flat for v in (x[0], x[1], y[0], y[1], 1, 0)]).reshape(-1, 24)
    off = np.concatenate([[0], np.cumsum([len(j) for j in jobs])]).astype(np.uint64)
    gt = C.glued_pairing(p, q, off)
    one = np.zeros(48, dtype=np.uint64)
    one[0] = 1
    return [bool(np.array_equal(gt[k], one)) for k in range(len(jobs))]


def model_pair_many(datas, per_point=PAIR_PER_POINT, base=PAIR_BASE, gas_limits=None):
    dec = [_decode_pairs(d, per_point, base, NO_GAS_LIMIT if gas_limits is None else gas_limits[i]) for i, d in enumerate(datas)]
    live = [i for i, d in enumerate(dec) if not isinstance(d, Result)]
    for i, one in zip(live, _products_are_one([dec[i] for i in live])):
        dec[i] = Result(int(one).to_bytes(32, "big"), None, ST_OK)
    return dec


def model_pair(data, per_point=PAIR_PER_POINT, base=PAIR_BASE, gas_limit=NO_GAS_LIMIT):
    """run_pair, reth_bn128.rs:156-217: gas, length, then pair after pair; 32 bytes holding 1 iff the product is one"""
    return model_pair_many([data], per_point, base, [gas_limit])[0]


# ---- the job generator ---------------------------------------------------------------------------------------------------------------
# A Job is one precompile input with the gas limit it is called with (None: exactly its cost) and the names of the classes it stands
# for.  `tags` are what the pool must hold at least three times each (tests/test_evm_model.py); the pool's order matters for ecMul, where
# a defective point sits next to every scalar.
Job = namedtuple("Job", "data gas_limit tags")
Pool = namedtuple("Pool", "add mul pair")

BAD_WORDS = {"p": P, "p+1": P + 1, "max": U256_MAX}
PAIR_SIZES = (0, 1, 2, 3, 4, 5, 9, 17)
ADD_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
MUL_LENGTHS = (0, 1, 63, 64, 65, 95, 96, 97, 128, 200)
G1_OFF_KINDS = ("y+1", "x0", "y0", "one_one")
POSITIONS = ("first", "mid", "last")
_G1_DEFECT_NAMES = [f"{c}.{n}" for n in BAD_WORDS for c in "xy"] + [f"off.{k}" for k in G1_OFF_KINDS] + ["x.p_y.offcurve"]
# the GLV edge scalars of test_gpu_groups.py::test_g1_scalar_mul_glv_edge_scalars
LAMBDA = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23
GLV_A1, GLV_B1, GLV_A2 = 9931322734385697763, 147946756881789319010696353538189108491, 147946756881789319000765030803803410728


def glv_edge_scalars():
    base = [0, 1, LAMBDA, r - LAMBDA, LAMBDA * LAMBDA % r, GLV_A1, GLV_B1, GLV_A2, (GLV_A1 + GLV_B1 * LAMBDA) % r, 1 << 127, 1 << 128,
            (1 << 128) - 1, (1 << 126) + 1, r - 1, r, r + 1, P - 1, (r + LAMBDA) % P, (3 * LAMBDA) % r, (LAMBDA << 3) % r]
    ks = []
    for v in base:
        ks += [v % P, (v + 1) % P, (v - 1) % P]
    return ks + [(x * LAMBDA + y) % r for x in (1, 2, 7, (1 << 127) - 1) for y in (0, 1, (1 << 127) - 1)]


def _w(v):
    return int(v).to_bytes(32, "big")


def _g1b(pt):
    return _w(pt[0]) + _w(pt[1])


def _g2b(q):
    (x, y) = q
    return _w(x[1]) + _w(x[0]) + _w(y[1]) + _w(y[0])          # x.c1 | x.c0 | y.c1 | y.c0 (EIP-197)


def _set_word(data, k, v):
    return data[:32 * k] + _w(v) + data[32 * k + 32:]


def _mul_any(F, pt, k):
    """[k] pt for a k of any size (pyref's proj_scalar_mul takes the scalar mod p): plain double-and-add on pyref's complete formulas"""
    acc = R.proj_zero(F)
    for bit in bin(k)[2:]:
        acc = R.proj_double(F, acc)
        if bit == "1":
            acc = R.proj_add(F, acc, pt)
    return acc


class _Gen:
    def __init__(self, seed):
        self.rng = Xoshiro(seed + 0xE7)
        self.g1_gen, self.g2_gen = (1, 2, 1), R.proj_from_affine(R.F2, R.G2_GEN_AFF)
        # a table of G2 points with known scalars: the subgroup test of the model is slow and cached per point
        self.g2_table = []
        for _ in range(12):
            b = self.scalar()
            x, y, _inf = R.affine_from_proj(R.F2, _mul_any(R.F2, self.g2_gen, b))
            self.g2_table.append((b, (x, y)))
        self.g1_table = [(a, self.g1(a)) for a in (self.scalar() for _ in range(16))]
        self.twist_outside = [self.twist_point() for _ in range(3)]
        self.small_order = self.small_order_point()

    def scalar(self):
        return self.rng.fp() % (r - 1) + 1

    def pick(self, seq):
        return seq[self.rng.next() % len(seq)]

    def g1(self, a=None):
        x, y, _inf = R.affine_from_proj(R.F1, R.proj_scalar_mul(R.F1, self.g1_gen, self.scalar() if a is None else a))
        return (x, y)

    def twist_point(self):
        """on the twist, outside the r-torsion (the cofactor 2p - r is huge): as test_gpu_groups.py::test_g2_subgroup_check builds them"""
        while True:
            x = (self.rng.fp(), self.rng.fp())
            y = fp2_sqrt(R.fp2_add(R.fp2_mul(R.fp2_square(x), x), R.TWIST_B))
            if y is not None:
                return (x, y)

    def small_order_point(self):
        """a twist point of order 10069 (test_gpu_groups.py::test_g2_small_order_twist_points): [r (2p - r) / 10069] T"""
        h2 = 2 * P - r
        assert h2 % 10069 == 0
        while True:
            x, y = self.twist_point()
            s = _mul_any(R.F2, (x, y, R.FP2_ONE), r * (h2 // 10069))
            if not R.proj_is_zero(R.F2, s):
                sx, sy, _inf = R.affine_from_proj(R.F2, s)
                return (sx, sy)

    def pairs(self, k, balanced):
        """k valid non-identity pairs as 192-byte elements; balanced: sum a_i b_i = 0 mod r, so the product of pairings is one"""
        assert not (balanced and k < 2)
        while True:
            qs = [self.pick(self.g2_table) for _ in range(k)]
            ps = [self.pick(self.g1_table) for _ in range(k)]          # table points: the Python scalar multiplications are the slow part
            if balanced:
                a = -sum(x * b for (x, _), (b, _) in zip(ps[:-1], qs[:-1])) * pow(qs[-1][0], -1, r) % r
                ps[-1] = (a, self.g1(a)) if a else (0, None)
            if all(a for a, _ in ps) and (sum(x * b for (x, _), (b, _) in zip(ps, qs)) % r == 0) == balanced:
                return [_g1b(pt) + _g2b(q) for (_, pt), (_, q) in zip(ps, qs)]

    def g1_off(self, kind):
        x, y = self.g1()
        return {"y+1": (x, (y + 1) % P), "x0": (0, y), "y0": (x, 0), "one_one": (1, 1)}[kind]

    def g2_off_word(self, word):
        """a valid G2 encoding with one of its four words changed (still < p)"""
        b = _g2b(self.pick(self.g2_table)[1])
        return _set_word(b, word, (_word(b, word) + 1 + self.rng.next() % 1000) % P)

    def g2_zeroed(self, mask):
        """a valid G2 encoding with the words of `mask` (4 bits, not all) set to zero: not the identity, and not on the twist"""
        b = _g2b(self.pick(self.g2_table)[1])
        for k in range(4):
            if (mask >> k) & 1:
                b = _set_word(b, k, 0)
        return b


def _at(k, where):
    return {"first": 0, "mid": k // 2, "last": k - 1}[where]


def _pair_pool(g):
    jobs = []
    add = lambda els, tags, gas=None: jobs.append(Job(b"".join(els) if isinstance(els, list) else els, gas, tuple(tags)))
    # valid jobs of every size, products that are one and that are not
    for k in PAIR_SIZES:
        for rep in range(3):
            if k == 0:
                add([], ["pair.size.0", "pair.valid"])
                continue
            if k >= 2:
                add(g.pairs(k, True), [f"pair.size.{k}", "pair.valid", "pair.balanced"])
            if k == 1 or rep < 2:
                add(g.pairs(k, False), [f"pair.size.{k}", "pair.valid", "pair.unbalanced"])
    # jobs made only of identity pairs
    ident = {"PO": lambda: _g1b(g.g1()) + bytes(128), "OQ": lambda: bytes(64) + _g2b(g.pick(g.g2_table)[1]), "OO": lambda: bytes(192)}
    for kinds in (["OO"], ["PO"], ["OQ"], ["PO", "OQ"], ["OO", "PO", "OQ", "OO"]):
        add([ident[k]() for k in kinds], ["pair.all_identity", "pair.valid"])
    # one identity pair inside otherwise balanced / unbalanced jobs: the answer is the one of the job without it
    for kind in ident:
        for where in POSITIONS:
            for balanced in (True, False):
                for rep in range(3):
                    els = g.pairs(2 + rep, balanced)
                    els.insert(_at(len(els) + 1, where), ident[kind]())
                    add(els, [f"pair.ident.{kind}", f"pair.ident.{where}", f"pair.ident.{kind}.{where}.{'bal' if balanced else 'unbal'}",
                              "pair.valid", "pair.balanced" if balanced else "pair.unbalanced"])
    # bases for the defects: balanced jobs (their answer without the defect would be 1), three or more pairs
    bases = [g.pairs(k, True) for k in (3, 4, 5, 9, 3, 17)]
    nb = [0]

    def base():
        nb[0] += 1
        return list(bases[nb[0] % len(bases)])

    def with_el(where, fn):
        els = base()
        i = _at(len(els), where)
        els[i] = fn(els[i])
        return els
    # one field word >= p: each of the six positions x each value x each place in the job
    for pos in range(6):
        for name, v in BAD_WORDS.items():
            for where in POSITIONS:
                for rep in range(3):
                    add(with_el(where, lambda e: _set_word(e, pos, v)),
                        [f"pair.field.pos{pos}.{name}.{where}", f"pair.field.pos{pos}", f"pair.field.{name}", f"pair.field.{where}", "pair.defect", "expect.4"])
    # G1 off the curve
    for kind in G1_OFF_KINDS:
        for where in POSITIONS:
            add(with_el(where, lambda e: _g1b(g.g1_off(kind)) + e[64:]), [f"pair.g1off.{kind}", f"pair.g1off.{where}", "pair.defect", "expect.1"])
    # G2 off the twist: one word changed; one, two or three of the four words zero
    for word in range(4):
        for where in POSITIONS:
            add(with_el(where, lambda e: e[:64] + g.g2_off_word(word)), [f"pair.g2off.word{word}", "pair.defect", "expect.1"])
    for mask in range(1, 15):
        for where in POSITIONS:
            add(with_el(where, lambda e: e[:64] + g.g2_zeroed(mask)),
                [f"pair.g2off.zero{bin(mask).count('1')}", f"pair.g2off.mask{mask:04b}", "pair.defect", "expect.1"])
    # G2 on the twist, outside the r-torsion
    for where in POSITIONS:
        for q in g.twist_outside:
            add(with_el(where, lambda e: e[:64] + _g2b(q)), ["pair.g2.notsub", "pair.defect", "expect.2"])
        add(with_el(where, lambda e: e[:64] + _g2b(g.small_order)), ["pair.g2.smallorder", "pair.defect", "expect.2"])
    # a defective pair ADDED to a balanced job: the pairs that remain multiply to one, and the job must still answer 0 with its status
    for where in POSITIONS:
        for tag, el in (("4", lambda: _set_word(g.pairs(1, False)[0], 0, P)), ("1", lambda: _g1b(g.g1_off("y+1")) + g.pairs(1, False)[0][64:]),
                        ("2", lambda: g.pairs(1, False)[0][:64] + _g2b(g.twist_outside[0]))):
            els = base()
            els.insert(_at(len(els) + 1, where), el())
            add(els, ["pair.defect.inserted", "pair.defect", f"expect.{tag}"])
    # a single defective pair: nothing remains
    for rep in range(3):
        add([_g1b(g.g1_off("y+1")) + g.pairs(1, False)[0][64:]], ["pair.defect.single", "pair.defect", "expect.1"])
        add([_set_word(g.pairs(1, False)[0], 5, P)], ["pair.defect.single", "pair.defect", "expect.4"])
    # two defects in one job: the order decides
    for rep in range(3):
        els = base()
        els[0] = _g1b(g.g1_off(G1_OFF_KINDS[rep])) + els[0][64:]
        els[1] = _set_word(els[1], rep, BAD_WORDS["p"])
        add(els, ["pair.two.g1off0_field1", "pair.defect", "expect.1"])              # pair 0 is finished before pair 1 is read
        els = base()
        i = _at(len(els), POSITIONS[rep])
        els[i] = _set_word(_g1b(g.g1_off("y+1")) + els[i][64:], 2 + rep, BAD_WORDS["max"])
        add(els, ["pair.two.same_pair_g1off_g2field", "pair.defect", "expect.4"])    # six reads before either point
        els = base()
        els[0] = els[0][:64] + _g2b(g.twist_outside[rep])
        els[2] = _g1b(g.g1_off("x0")) + els[2][64:]
        add(els, ["pair.two.g2sub0_g1off2", "pair.defect", "expect.2"])
        els = base()
        els[-1] = _g1b(g.g1_off("one_one")) + g.g2_off_word(rep)                     # G1 before G2 within the pair: both give status 1
        els[0] = els[0][:64] + _g2b(g.small_order)
        add(els, ["pair.two.g2sub_first_g1off_last", "pair.defect", "expect.2"])
    # gas: one below the cost wins over everything; lengths that are no multiple of 192
    for rep in range(3):
        k = 2 + rep
        cost = k * PAIR_PER_POINT + PAIR_BASE
        add(g.pairs(k, True), ["pair.gas.valid", "pair.host"], cost - 1)
        add(b"".join(g.pairs(k, True)) + bytes([1 + rep]) * (1 + 95 * rep), ["pair.gas.badlen", "pair.host"], cost - 1)
        els = with_el(POSITIONS[rep], lambda e: _g1b(g.g1_off("y+1")) + e[64:])
        add(els, ["pair.gas.badpoint", "pair.host"], len(els) * PAIR_PER_POINT + PAIR_BASE - 1)
        for n in (191, 193, 383):
            add(b"".join(g.pairs(2, True))[:n], [f"pair.len.{n}", "pair.host"])
    return jobs


def _g1_defects(g):
    """name -> 64 bytes: every way a G1 operand can be wrong, with the status it must give"""
    out = {}
    for name, v in BAD_WORDS.items():
        x, y = g.g1()
        out[f"x.{name}"] = (_w(v) + _w(y), ST_DECODE_ERROR)
        out[f"y.{name}"] = (_w(x) + _w(v), ST_DECODE_ERROR)
    for kind in G1_OFF_KINDS:
        out[f"off.{kind}"] = (_g1b(g.g1_off(kind)), ST_NOT_ON_CURVE)
    out["x.p_y.offcurve"] = (_w(P) + _w(1), ST_DECODE_ERROR)            # (p, 1): reads fail before the curve is looked at
    return out


def _add_pool(g):
    jobs = []
    add = lambda data, tags, gas=None: jobs.append(Job(data, gas, tuple(tags)))
    crafted = crafted_g1_points()
    for rep in range(3):
        p, q = g.g1(), g.g1()
        add(_g1b(p) + _g1b(q), ["add.PQ", "add.valid"])
        add(_g1b(p) + _g1b(p), ["add.PP", "add.valid"])
        add(_g1b(p) + _g1b((p[0], P - p[1])), ["add.PnegP", "add.valid"])
        add(bytes(64) + _g1b(q), ["add.OQ", "add.valid"])
        add(_g1b(p) + bytes(64), ["add.PO", "add.valid"])
        add(bytes(128), ["add.OO", "add.valid"])
    for i, c in enumerate(crafted):
        other = crafted[(i + 1) % len(crafted)] if i % 3 == 0 else c if i % 3 == 1 else g.g1()
        add(_g1b(c) + _g1b(other), ["add.crafted", "add.valid"])
    for rep in range(3):
        d = _g1_defects(g)
        for name, (enc, st) in d.items():
            add(enc + _g1b(g.g1()), [f"add.def1.{name}", "add.defect", f"expect.{st}"])
            add(_g1b(g.g1()) + enc, [f"add.def2.{name}", "add.defect", f"expect.{st}"])
            add(bytes(64) + enc, [f"add.def2.{name}", "add.defect", f"expect.{st}"])
        # one defect on each operand: operand 1's decides, whatever operand 2 holds
        for n1, n2 in (("off.y+1", "x.p"), ("off.one_one", "y.max"), ("x.p+1", "off.y0"), ("y.p", "off.x0"), ("off.x0", "off.y+1"), ("x.max", "y.p")):
            kind = "offcurve_then_ge_p" if (n1.startswith("off") and not n2.startswith("off")) else "other"
            add(d[n1][0] + d[n2][0], ["add.both", f"add.both.{kind}", "add.defect", f"expect.{d[n1][1]}"])
    # every length class, on P | Q, on O | Q and on P | 0x30.. (a word just below p in its top byte)
    for rep in range(3):
        full = [_g1b(g.g1()) + _g1b(g.g1()) + bytes([0xAB]) * 80, bytes(64) + _g1b(g.g1()) + bytes([0x01]) * 80,
                _g1b(g.g1()) + bytes([0x30]) + bytes(63) + bytes([0xFF]) * 80][rep]
        for n in ADD_LENGTHS:
            add(full[:n], [f"add.len.{n}"])
        add(_g1b(g.g1()) + _g1b(g.g1()), ["add.gas"], ADD_GAS - 1)
        add(_g1b(g.g1_off("y+1")) + _g1b(g.g1()), ["add.gas"], ADD_GAS - 1)
    return jobs


def _mul_scalars(g):
    ks = []
    for m in range(6):
        for d in (-1, 0, 1):
            if 0 <= m * r + d <= U256_MAX:
                ks.append((f"mul.k.{m}r{d:+d}", m * r + d))
    ks += [("mul.k.max", U256_MAX), ("mul.k.2^255", 1 << 255), ("mul.k.p", P), ("mul.k.p-1", P - 1), ("mul.k.5r+top", U256_MAX - 1)]
    ks = [kv for kv in ks for _ in range(3)]
    ks += [("mul.k.glv", k) for k in glv_edge_scalars()]
    ks += [("mul.k.random", g.rng.u256()) for _ in range(24)]
    return ks


def _mul_pool(g):
    jobs = []
    add = lambda data, tags, gas=None: jobs.append(Job(data, gas, tuple(tags)))
    crafted = crafted_g1_points()
    defects = [v for d in (_g1_defects(g) for _ in range(3)) for v in d.items()]
    # every scalar on a valid point, with a defective point on the same scalar right after it: a wrong row offset shows
    for i, (tag, k) in enumerate(_mul_scalars(g)):
        pt = crafted[i % len(crafted)] if i % 4 == 3 else g.g1()
        add(_g1b(pt) + _w(k), [tag, "mul.pt.crafted" if i % 4 == 3 else "mul.pt.P", "mul.valid"])
        if i % 7 == 0:
            add(bytes(64) + _w(k), [tag, "mul.pt.O", "mul.valid"])
        name, (enc, st) = defects[i % len(defects)]
        add(enc + _w(k), [f"mul.def.{name}", "mul.defect_neighbour", "mul.defect", f"expect.{st}"])
    for rep in range(3):
        full = [_g1b(g.g1()) + _w(g.rng.u256()) + bytes([0xCD]) * 104, bytes(64) + _w(r + 5) + bytes([0x01]) * 104,
                _g1b(crafted[rep]) + _w(U256_MAX) + bytes([0xFF]) * 104][rep]
        for n in MUL_LENGTHS:
            add(full[:n], [f"mul.len.{n}"])
        add(_g1b(g.g1()) + _w(7), ["mul.gas"], MUL_GAS - 1)
        add(_g1b(g.g1_off("x0")) + _w(7), ["mul.gas"], MUL_GAS - 1)
    return jobs


_POOLS = {}


def build_pool(seed=SEED):
    """the pool of jobs for one seed (cached): Pool(add, mul, pair), each a list of Job in a fixed order"""
    if seed not in _POOLS:
        g = _Gen(seed)
        _POOLS[seed] = Pool(_add_pool(g), _mul_pool(g), _pair_pool(g))
    return _POOLS[seed]


def required_tags():
    """every class the pool must hold at least three times"""
    t = [f"pair.size.{k}" for k in PAIR_SIZES] + ["pair.balanced", "pair.unbalanced", "pair.all_identity"]
    t += [f"pair.ident.{kind}.{where}.{b}" for kind in ("PO", "OQ", "OO") for where in POSITIONS for b in ("bal", "unbal")]
    t += [f"pair.field.pos{pos}.{name}.{where}" for pos in range(6) for name in BAD_WORDS for where in POSITIONS]
    t += [f"pair.g1off.{k}" for k in G1_OFF_KINDS] + [f"pair.g2off.word{k}" for k in range(4)] + [f"pair.g2off.zero{k}" for k in (1, 2, 3)]
    t += [f"pair.g2off.mask{m:04b}" for m in range(1, 15)] + ["pair.g2.notsub", "pair.g2.smallorder"]
    t += ["pair.two.g1off0_field1", "pair.two.same_pair_g1off_g2field", "pair.two.g2sub0_g1off2", "pair.two.g2sub_first_g1off_last"]
    t += ["pair.defect.inserted", "pair.defect.single", "pair.gas.valid", "pair.gas.badlen", "pair.gas.badpoint", "pair.len.191", "pair.len.193", "pair.len.383"]
    names = list(_G1_DEFECT_NAMES)
    t += ["add.PQ", "add.PP", "add.PnegP", "add.OQ", "add.PO", "add.OO", "add.crafted", "add.both.offcurve_then_ge_p", "add.both.other", "add.gas"]
    t += [f"add.def{k}.{n}" for k in (1, 2) for n in names] + [f"add.len.{n}" for n in ADD_LENGTHS]
    t += [f"mul.k.{m}r{d:+d}" for m in range(6) for d in (-1, 0, 1) if 0 <= m * r + d <= U256_MAX]
    t += ["mul.k.max", "mul.k.2^255", "mul.k.p", "mul.k.p-1", "mul.k.glv", "mul.k.random", "mul.pt.P", "mul.pt.O", "mul.pt.crafted", "mul.defect_neighbour", "mul.gas"]
    t += [f"mul.def.{n}" for n in names] + [f"mul.len.{n}" for n in MUL_LENGTHS]
    return t


def tag_counts(jobs):
    return Counter(t for j in jobs for t in j.tags)


# ---- the model over a pool -----------------------------------------------------------------------------------------------------------
def cost_of(kind, job):
    return {"add": ADD_GAS, "mul": MUL_GAS}.get(kind) or (len(job.data) // 192) * PAIR_PER_POINT + PAIR_BASE


def limit_of(kind, job):
    return cost_of(kind, job) if job.gas_limit is None else job.gas_limit


_EXPECT = {}


def expected(kind, seed=SEED):
    """for every job of the pool, in order: (the precompile's Result under the job's gas limit, the device's Result = the same input
    with gas out of the picture, or None where the input's length keeps it from the device entry point)"""
    if (kind, seed) not in _EXPECT:
        jobs = getattr(build_pool(seed), kind)
        if kind == "pair":
            dev = [None if len(j.data) % 192 else d for j, d in zip(jobs, model_pair_many([j.data for j in jobs]))]
            host = model_pair_many([j.data for j in jobs], gas_limits=[limit_of(kind, j) for j in jobs])
        else:
            fn = model_add if kind == "add" else model_mul
            dev = [fn(j.data) for j in jobs]
            host = [fn(j.data, cost_of(kind, j), limit_of(kind, j)) for j in jobs]
        _EXPECT[(kind, seed)] = list(zip(host, dev))
    return _EXPECT[(kind, seed)]
