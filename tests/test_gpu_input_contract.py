"""The input contract of the whole C ABI (include/sylow_hip.h, Conventions): field elements cross as 4 uint64 limbs and "inputs >= p are
reduced mod p exactly like `Fp::new`"; every optional infinity-flag array "may be NULL = none".

CONTRACT has one row per declared entry point: the arguments that hold Fp-valued words and their word layout, the optional input flag
arrays, or the reason the row is exempt.  A CPU test fails when an entry point has no row, so a new one cannot skip the contract.

The GPU cases call each non-exempt entry point on a meaningful canonical batch (valid points where the operation needs them, identity
flags, Z = 0 rows, invalid signatures), then again with each Fp argument replaced by representatives x + k p (helpers.representatives:
one argument at a time, all at once, and the largest k that fits 256 bits), and require every output -- values, flags, status bytes,
booleans -- to be bit-identical.  Rows with optional flags also compare NULL flags with all-zero flag arrays.  The pairing, verification,
Miller-loop and final-exponentiation rows run at one size per route (plk_multi.hip / plk_quad.hip caps): one element (one wavefront),
the two-per-wavefront range, the quad range, and one lane-pair round plus a tail (the tail on quads on the side stream)."""
import os
import re
import sys

import numpy as np
import pytest

from helpers import P, SEED, U256, Xoshiro, crafted_g2_points, limbs, pack, rand_fp_array, representatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP, FP2, FP6, FP12, G1A, G2A, G1P, G2P, LINES, LINE = "Fp", "Fp2", "Fp6", "Fp12", "G1 affine", "G2 affine", "G1 projective", "G2 projective", \
    "line coefficients [87*24]", "line (ell_0, ell_vw, ell_vv)"


class Row:
    def __init__(self, fp=None, flags=(), exempt=None):
        self.fp, self.flags, self.exempt = dict(fp or {}), tuple(flags), exempt


def ex(reason):
    return Row(exempt=reason)


RUNTIME = "runtime, options, memory or streams: no field input"
HOOK = "raw test hook: operands applied exactly as given (test_gpu_f29_bounds.py, test_gpu_pairing_layouts.py)"
FR = "Fr-valued arguments: tested with their own edge values (test_gpu_fields.py, test_gpu_fr_threshold.py)"
BYTES = "byte codec: values >= p are rejected by contract (test_gpu_bytes.py, test_gpu_evm.py, test_gpu_host_pipeline.py)"
SCALAR = "scalar arguments only (reduced like Fp::new: test_gpu_groups.py, test_gpu_msm.py, test_gpu_hash_bls.py)"
FLAGS = "flag arrays and collectives: no field input"

CONTRACT = {
    **{s: ex(RUNTIME) for s in ["init", "init_devices", "set_device", "shutdown", "trim", "set_scratch_limit", "set_option", "get_option",
                                "clock_probe", "wall_clock_khz", "last_error", "device_count", "malloc", "free", "memcpy_h2d", "memcpy_d2h",
                                "stream_sync", "host_malloc", "host_free", "g2_line_table_words"]},
    "host_xoshiro_fp": ex("a generator: no input"),
    "aos_to_soa": ex("a word transpose: moves words as given, no arithmetic"),
    "soa_to_aos": ex("a word transpose: moves words as given, no arithmetic"),
    **{s: ex(HOOK) for s in ["f29_hook_batch", "f29_raw_hook_batch", "fp12_hook_batch"]},
    **{s: ex(FR) for s in ["fr_add_batch", "fr_sub_batch", "fr_mul_batch", "fr_sqr_batch", "fr_neg_batch", "fr_inv_batch", "fr_to_be_bytes_batch"]},
    **{s: ex(BYTES) for s in ["fp_from_be_bytes_batch", "fr_from_be_bytes_batch", "g1_from_be_bytes_batch", "g2_from_be_bytes_batch",
                              "evm_ecadd_batch", "evm_ecmul_batch", "evm_ecpairing_batch", "pairing_host_bytes", "bls_verify_host_bytes",
                              "hash_to_field_batch", "hash_to_g1_batch"]},
    **{s: ex(SCALAR) for s in ["g1_generator_mul_batch", "g2_generator_mul_batch", "bls_sign_batch"]},
    "fp_compute_naf_batch": ex("the raw 256-bit words by design (fp.rs compute_naf on the integer)"),
    "flags_all": ex(FLAGS), "all_valid": ex(FLAGS),
    # ---- Fp and the tower
    **{s: Row({"a": FP, "b": FP}) for s in ["fp_add_batch", "fp_sub_batch", "fp_mul_batch"]},
    **{s: Row({"a": FP}) for s in ["fp_sqr_batch", "fp_neg_batch", "fp_inv_batch", "fp_sqrt_batch", "fp_is_square_batch", "fp_to_be_bytes_batch"]},
    "fp_pow_batch": Row({"a": FP}),                                    # the exponent e is a raw 256-bit integer by design
    "fext_add_batch": Row({"a": "Fp2 / Fp6 / Fp12", "b": "Fp2 / Fp6 / Fp12"}),
    "fext_sub_batch": Row({"a": "Fp2 / Fp6 / Fp12", "b": "Fp2 / Fp6 / Fp12"}),
    "fext_neg_batch": Row({"a": "Fp2 / Fp6 / Fp12"}),
    "fext_scale_batch": Row({"a": "Fp2 / Fp6 / Fp12", "k": FP}),
    "fp2_mul_batch": Row({"a": FP2, "b": FP2}),
    **{s: Row({"a": FP2}) for s in ["fp2_sqr_batch", "fp2_inv_batch", "fp2_residue_mul_batch", "fp2_frobenius_batch"]},
    "fp6_mul_batch": Row({"a": FP6, "b": FP6}),
    **{s: Row({"a": FP6}) for s in ["fp6_inv_batch", "fp6_sqr_batch", "fp6_residue_mul_batch", "fp6_frobenius_batch"]},
    "fp12_mul_batch": Row({"a": FP12, "b": FP12}),
    **{s: Row({"a": FP12}) for s in ["fp12_sqr_batch", "fp12_inv_batch", "fp12_frobenius_batch", "fp12_cyclotomic_sqr_batch"]},
    "fp12_sparse_mul_batch": Row({"f": FP12, "ell": LINE}),
    "gt_pow_batch": Row({"gt": FP12}),                                 # k: the raw 256-bit scalar walked by design
    "svdw_map_batch": Row({"u": FP}),
    # ---- groups
    "g1_scalar_mul_batch": Row({"p_xy": G1A}, ["p_inf"]),
    "g2_scalar_mul_batch": Row({"p_xy": G2A}, ["p_inf"]),
    "g2_scalar_mul_subgroup_batch": Row({"p_xy": G2A}, ["p_inf"]),
    **{s: Row({"a_xy": G1A, "b_xy": G1A}, ["a_inf", "b_inf"]) for s in ["g1_add_batch", "g1_sub_batch"]},
    **{s: Row({"a_xy": G2A, "b_xy": G2A}, ["a_inf", "b_inf"]) for s in ["g2_add_batch", "g2_sub_batch"]},
    "g1_double_batch": Row({"a_xy": G1A}, ["a_inf"]),
    "g2_double_batch": Row({"a_xy": G2A}, ["a_inf"]),
    "g1_projective_new_batch": Row({"p_xyz": G1P}),
    "g2_projective_new_batch": Row({"p_xyz": G2P}),
    "g1_ct_eq_batch": Row({"a_xyz": G1P, "b_xyz": G1P}),
    "g2_ct_eq_batch": Row({"a_xyz": G2P, "b_xyz": G2P}),
    "g1_normalize_batch": Row({"p_xyz": G1P}),
    "g2_normalize_batch": Row({"p_xyz": G2P}),
    "g1_lincomb_batch": Row({"p_xy": G1A}, ["p_inf"]),
    "g1_msm": Row({"p_xy": G1A}, ["p_inf"]),
    "g1_msm_tuned": Row({"p_xy": G1A}, ["p_inf"]),
    "g1_sum_batch": Row({"p_xy": G1A}, ["p_inf"]),
    "g1_on_curve_batch": Row({"p_xy": G1A}, ["p_inf"]),
    "g2_psi_batch": Row({"q_xy": G2A}, ["q_inf"]),
    "g2_subgroup_check_batch": Row({"q_xy": G2A}, ["q_inf"]),
    "g1_to_be_bytes_batch": Row({"p_xy": G1A}, ["p_inf"]),
    "g2_to_be_bytes_batch": Row({"p_xy": G2A}, ["p_inf"]),
    # ---- pairing
    "miller_loop_batch": Row({"p_xy": G1A, "q_xy": G2A}),
    "final_exp_batch": Row({"f": FP12}),
    "pairing_batch": Row({"p_xy": G1A, "q_xy": G2A}, ["p_inf", "q_inf"]),
    "pairing_host": Row({"p_aos": G1A + " (AoS, host)", "q_aos": G2A + " (AoS, host)"}, ["p_inf", "q_inf"]),
    "multi_pairing_batch": Row({"p_xy": G1A, "q_xy": G2A}, ["p_inf", "q_inf"]),
    "glued_miller_loop_batch": Row({"p_xy": G1A, "q_xy": G2A}),
    "pairing_product_batch": Row({"p_xy": G1A, "q_xy": G2A}, ["p_inf", "q_inf"]),
    "pairing_product_partial_batch": Row({"p_xy": G1A, "q_xy": G2A}, ["p_inf", "q_inf"]),
    "pairing_product_all": Row({"p_xy": G1A, "q_xy": G2A}, ["p_inf", "q_inf"]),
    "fp12_product_final_exp": Row({"parts": FP12}),
    "g2_precompute_batch": Row({"q_xy": G2A}),
    "miller_loop_precomputed_batch": Row({"coeffs": LINES, "p_xy": G1A}),
    "glued_miller_loop_precomputed_batch": Row({"coeffs": LINES, "p_xy": G1A}),
    # ---- BLS (message bytes are not field elements; weights are scalars)
    **{s: Row({"pk_xy": G2A, "sig_xy": G1A}, ["pk_inf", "sig_inf"]) for s in ["bls_verify_batch", "bls_verify_fused_batch",
                                                                             "bls_verify_two_pairings_batch", "bls_verify_same_signer_batch",
                                                                             "bls_aggregate_partial_batch", "bls_aggregate_verify_batch",
                                                                             "bls_weighted_partial_batch", "bls_batch_verify_weighted"]},
    "bls_verify_host": Row({"pk_aos": G2A + " (AoS, host)", "sig_aos": G1A + " (AoS, host)"}, ["pk_inf", "sig_inf"]),
    "g2_line_table": Row({"q_xy": G2A}),
    "bls_verify_line_table_batch": Row({"sig_xy": G1A}, ["pk_inf", "sig_inf"]),   # pk_table: opaque device digits from g2_line_table
}
CONTRACT = {"sylow_hip_" + k: v for k, v in CONTRACT.items()}


# ================================================================ CPU: the table is complete and names real parameters ==========
def test_every_declared_entry_point_has_a_contract_row():
    import __graft_entry__
    from test_rust_ffi import parse_header
    declared = set(__graft_entry__.declared_symbols())
    assert not declared - set(CONTRACT), f"entry points without an input-contract row: {sorted(declared - set(CONTRACT))}"
    assert not set(CONTRACT) - declared, f"rows for entry points the header no longer declares: {sorted(set(CONTRACT) - declared)}"
    protos = parse_header()
    for name, row in CONTRACT.items():
        params = {p[3] for p in protos[name][1]}
        if row.exempt:
            assert not row.fp and not row.flags and row.exempt.strip(), name
            continue
        assert row.fp, f"{name}: a non-exempt row names its Fp arguments"
        assert set(row.fp) | set(row.flags) <= params, (name, sorted(set(row.fp) | set(row.flags) - params))
        assert name in CASES, f"{name}: no GPU case"
    assert set(CASES) == {n for n, r in CONTRACT.items() if not r.exempt}


def test_optional_flags_match_the_shape_annotations():
    """every optional (`?`) u8 input named *_inf in a @shape line is a flag argument of its row"""
    from sylow_amd import _shapes
    for name, (_, shapes) in _shapes.parse().items():
        row = CONTRACT[name]
        opt_flags = {p for p, sh in shapes.items() if sh.optional and sh.dtype == "u8" and p.endswith("_inf")}
        if not row.exempt:
            assert opt_flags == set(row.flags), (name, sorted(opt_flags), row.flags)


def test_representatives_cover_the_special_words():
    x = limbs([0] * 5 + [1, P - 1, U256 - 1 - 5 * P, U256 - 5 * P, 12345])
    rnd, big = representatives(x, 1), representatives(x, 1, largest=True)
    to_int = lambda a: [sum(int(r[k]) << (64 * k) for k in range(4)) for r in a]
    for r in (rnd, big):
        assert [v % P for v in to_int(r)] == to_int(x) and all(P <= v < U256 for v in to_int(r))
    assert {P, 2 * P, 5 * P} <= set(to_int(rnd[:5]))
    assert to_int(big)[7] == U256 - 1 and to_int(big)[8] == U256 - P        # k = 5 fits below 2^256 - 5 p, k = 4 from there on
    assert to_int(representatives(limbs([1] * 40), 2)).count(P + 1) > 0


def _src(name):
    return open(os.path.join(ROOT, "sylow_amd", "csrc", name)).read()


def route_caps(cus):
    """the batch sizes where the pairing-family routes change, read from the sources: one wavefront per element up to `cus`, two per
    wavefront above it up to WIDE_MAX (pairings) / WIDE_VERIFY_MAX (verifications); quads up to cus * 4 * 16; lane-pair rounds of
    cus * BLOCK / 2 elements, a tail of one or two rounds on quads"""
    cap = lambda fn: int(re.search(fn + r"\(\) \{.*?wide_pack\(\) \? (\d+) :", _src("plk_multi.hip"), re.S).group(1))
    wide_max, wide_verify_max = cap("wide_batch_max"), cap("wide_verify_max")
    q = re.search(r"return \(size_t\)\(cus \? cus : 256\) \* (\d+) \* (\d+);", _src("plk_quad.hip"))
    r = re.search(r"const size_t round = \(size_t\)\(cus \? cus : 256\) \* \(BLOCK / (\d+)\);", _src("plk_quad.hip"))
    block = int(re.search(r"constexpr int BLOCK = (\d+);", _src("common.hpp")).group(1))
    return dict(wide_pack=cus, wide_max=wide_max, wide_verify_max=wide_verify_max, quad_max=cus * int(q.group(1)) * int(q.group(2)),
                round=cus * block // int(r.group(1)))


def route_sizes(cus, verify=False):
    c = route_caps(cus)
    two = c["wide_pack"] + 45                                      # two elements per wavefront
    quad = 7000 if c["wide_max"] < 7000 <= c["quad_max"] else c["wide_max"] + 857
    tail = c["round"] + 777                                        # one round on lane pairs, the tail on quads
    sizes = {"one": 1, "two_per_wave": two, "quad": quad, "round_tail": tail}
    cap = c["wide_verify_max"] if verify else c["wide_max"]
    assert 1 < c["wide_pack"] < two <= cap < quad <= c["quad_max"] < tail - 777 and 777 <= c["quad_max"]
    return sizes


def test_route_sizes_straddle_the_caps():
    c = route_caps(256)
    assert (c["wide_max"], c["wide_verify_max"], c["quad_max"], c["round"]) == (6144, 4096, 16384, 32768)
    assert route_sizes(256) == {"one": 1, "two_per_wave": 301, "quad": 7000, "round_tail": 33545}
    route_sizes(256, verify=True)


# ================================================================ GPU =======================================================
class Ctx:
    """what one call of a case sees: `fp(arg, a)` returns the canonical array or its representatives, `flag(arg, f)` the canonical flags,
    all-zero flags or None (NULL)"""

    def __init__(self, targets=(), largest=False, flags="given"):
        self.targets, self.largest, self.flags = set(targets), largest, flags
        self.seen_fp, self.seen_flags = set(), set()

    def fp(self, arg, a):
        self.seen_fp.add(arg)
        if arg not in self.targets:
            return a
        return representatives(a, seed=SEED + sum(map(ord, arg)) + 7 * len(self.seen_fp), largest=self.largest)

    def flag(self, arg, f):
        self.seen_flags.add(arg)
        if self.flags == "null":
            return None
        return np.zeros_like(f) if self.flags == "zero" else f


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: output {i} differs in {int(np.sum(x != y)) if x.shape == y.shape else 'shape'} words"


def check_row(engine, name, case):
    row = CONTRACT[name]
    c0 = Ctx()
    base = case(engine, c0)
    assert c0.seen_fp == set(row.fp) and c0.seen_flags == set(row.flags), (name, c0.seen_fp, c0.seen_flags)
    for arg in row.fp:
        _same(case(engine, Ctx({arg})), base, f"{name}: {arg} as representatives")
    if len(row.fp) > 1:
        _same(case(engine, Ctx(row.fp)), base, f"{name}: every Fp argument as representatives")
    _same(case(engine, Ctx(row.fp, largest=True)), base, f"{name}: the largest representatives")
    if row.flags:
        _same(case(engine, Ctx(flags="null")), case(engine, Ctx(flags="zero")), f"{name}: NULL flags against all-zero flags")
        _same(case(engine, Ctx(row.fp, flags="null")), case(engine, Ctx(flags="zero")), f"{name}: NULL flags, representatives")
    return base


# ---- canonical data ---------------------------------------------------------------------------------------------------------
D = 64


def _fp_ints(a):
    return [sum(int(r[k]) << (64 * k) for k in range(4)) for r in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


@pytest.fixture(scope="module")
def pool(engine):
    from oracle import pyref as R
    from test_gpu_multi_pairing import G1, G2
    rng = Xoshiro(SEED + 0x1C)
    sk = limbs([rng.fp() for _ in range(D)])
    g1, _ = engine.g1_scalar_mul(np.repeat(pack(G1, 8), D, 0), limbs([rng.fp() for _ in range(D)]))
    g2, _ = engine.g2_scalar_mul(np.repeat(pack(G2, 16), D, 0), limbs([rng.fp() for _ in range(D)]))
    msgs = [b"contract %d" % i + bytes([i]) * (i % 7) for i in range(D)]
    sig, _ = engine.bls_sign(sk, msgs)
    pk, _ = engine.g2_generator_mul(sk)
    gt = engine.pairing(g1[:8], g2[:8], pipelined=False)
    # projective forms (x z, y z, z) with random z, and z = 0 rows
    zs = [rng.fp() for _ in range(D)]
    p1 = np.zeros((D, 12), dtype=np.uint64)
    p2 = np.zeros((D, 24), dtype=np.uint64)
    for i in range(D):
        x, y = _fp_ints(g1[i])
        p1[i] = limbs([x * zs[i] % P, y * zs[i] % P, zs[i]]).reshape(12)
        q = _fp_ints(g2[i])
        z2 = (zs[i], zs[(i + 1) % D])
        xs, ys = R.fp2_mul((q[0], q[1]), z2), R.fp2_mul((q[2], q[3]), z2)
        p2[i] = limbs([*xs, *ys, *z2]).reshape(24)
    for i in range(0, D, 8):                                   # the identity as (0, 1, 0), and as (x, y, 0) with x, y != 0
        p1[i] = limbs([0, 1, 0]).reshape(12) if i % 16 == 0 else np.concatenate([p1[i, :8], np.zeros(4, np.uint64)])
        p2[i] = limbs([0, 0, 1, 0, 0, 0]).reshape(24) if i % 16 == 0 else np.concatenate([p2[i, :16], np.zeros(8, np.uint64)])
    return dict(sk=sk, g1=g1, g2=g2, msgs=msgs, sig=sig, pk=pk, gt=gt, p1=p1, p2=p2)


def _flags(n, seed, density=11):
    f = np.zeros(n, dtype=np.uint8)
    f[(np.arange(n) * 7 + seed) % density == 0] = 1
    f[0] = 0
    return f


def _tile(a, n, step=1):
    idx = (np.arange(n) * step) % a.shape[0]
    return np.ascontiguousarray(a[idx])


def _fp_values(n, seed):
    """canonical Fp values: random, then 0, 1, p - 1 and the value whose largest representative is 2^256 - 1"""
    a = rand_fp_array(Xoshiro(seed), n, 1)
    a[:4] = limbs([0, 1, P - 1, U256 - 1 - 5 * P])
    return a


def _msgs_for(pool, n, bad_every=5):
    """messages of n verifications against pool signatures: every bad_every-th one (element 0 excepted) is another message"""
    return [pool["msgs"][i % D] if i % bad_every != bad_every - 1 else pool["msgs"][(i + 1) % D] for i in range(n)]


# ---- the cases ----------------------------------------------------------------------------------------------------------------
CASES = {}


def case(*names):
    def reg(fn):
        for nm in names:
            CASES["sylow_hip_" + nm] = (lambda nm: lambda eng, c, pool: fn(eng, c, pool, nm))(nm)
        return fn
    return reg


N_FIELD = 96


@case("fp_add_batch", "fp_sub_batch", "fp_mul_batch")
def _fp_bin(eng, c, pool, nm):
    a, b = _fp_values(N_FIELD, SEED + 1), _fp_values(N_FIELD, SEED + 2)[::-1].copy()
    return [eng._binop("sylow_hip_" + nm, 4, c.fp("a", a), c.fp("b", b))]


@case("fp_sqr_batch", "fp_neg_batch", "fp_inv_batch")
def _fp_un(eng, c, pool, nm):
    return [eng._unop("sylow_hip_" + nm, 4, c.fp("a", _fp_values(N_FIELD, SEED + 3)))]


@case("fp_pow_batch")
def _fp_pow(eng, c, pool, nm):
    rng = Xoshiro(SEED + 4)
    e = limbs([rng.u256() for _ in range(N_FIELD - 3)] + [0, 1, U256 - 1])
    return [eng.fp_pow(c.fp("a", _fp_values(N_FIELD, SEED + 5)), e)]


@case("fp_sqrt_batch")
def _fp_sqrt(eng, c, pool, nm):
    v = _fp_values(N_FIELD, SEED + 6)
    sq = eng.fp_sqr(v[: N_FIELD // 2])                            # half squares, half random (about half of those non-squares)
    return list(eng.fp_sqrt(c.fp("a", np.concatenate([v[:4], sq, v[N_FIELD // 2 + 4:]]))))


@case("fp_is_square_batch")
def _fp_is_square(eng, c, pool, nm):
    v = _fp_values(N_FIELD, SEED + 7)
    return [eng.fp_is_square(c.fp("a", np.concatenate([v, eng.fp_sqr(v)])))]


@case("fp_to_be_bytes_batch")
def _fp_to_bytes(eng, c, pool, nm):
    return [np.frombuffer(b"".join(eng.fp_to_be_bytes(c.fp("a", _fp_values(N_FIELD, SEED + 8)))), dtype=np.uint8)]


@case("fext_add_batch", "fext_sub_batch", "fext_neg_batch", "fext_scale_batch")
def _fext(eng, c, pool, nm):
    op = nm.split("_")[1]
    out = []
    for deg in (2, 6, 12):
        a = rand_fp_array(Xoshiro(SEED + 9 + deg), N_FIELD, deg)
        a[0] = 0
        a[1, :4] = limbs([U256 - 1 - 5 * P])
        if op == "neg":
            out.append(eng.fext_op(op, c.fp("a", a)))
        elif op == "scale":
            out.append(eng.fext_op(op, c.fp("a", a), c.fp("k", _fp_values(N_FIELD, SEED + 10))))
        else:
            out.append(eng.fext_op(op, c.fp("a", a), c.fp("b", rand_fp_array(Xoshiro(SEED + 11 + deg), N_FIELD, deg))))
    return out


WIDTH = {"fp2": 8, "fp6": 24, "fp12": 48}


def _tower_in(width, seed):
    a = rand_fp_array(Xoshiro(seed), N_FIELD, width // 4)
    a[0] = 0
    a[1] = 0
    a[1, 0] = 1
    a[2, :4] = limbs([U256 - 1 - 5 * P])
    return a


@case("fp2_mul_batch", "fp6_mul_batch", "fp12_mul_batch")
def _tower_bin(eng, c, pool, nm):
    w = WIDTH[nm.split("_")[0]]
    return [eng._binop("sylow_hip_" + nm, w, c.fp("a", _tower_in(w, SEED + 12)), c.fp("b", _tower_in(w, SEED + 13)))]


@case("fp2_sqr_batch", "fp2_inv_batch", "fp2_residue_mul_batch", "fp6_inv_batch", "fp6_sqr_batch", "fp6_residue_mul_batch",
      "fp12_sqr_batch", "fp12_inv_batch")
def _tower_un(eng, c, pool, nm):
    w = WIDTH[nm.split("_")[0]]
    return [eng._unop("sylow_hip_" + nm, w, c.fp("a", _tower_in(w, SEED + 14)))]


@case("fp2_frobenius_batch", "fp6_frobenius_batch", "fp12_frobenius_batch")
def _frob(eng, c, pool, nm):
    w = WIDTH[nm.split("_")[0]]
    a = _tower_in(w, SEED + 15)
    exps = (1, 2, 3) if w == 48 else range(6)
    f = {8: eng.fp2_frobenius, 24: eng.fp6_frobenius, 48: eng.fp12_frobenius}[w]
    return [f(c.fp("a", a), e) for e in exps]


@case("fp12_cyclotomic_sqr_batch")
def _cyc(eng, c, pool, nm):
    return [eng.fp12_cyclotomic_sqr(c.fp("a", pool["gt"]))]


@case("fp12_sparse_mul_batch")
def _sparse(eng, c, pool, nm):
    f, ell = _tower_in(48, SEED + 16), rand_fp_array(Xoshiro(SEED + 17), N_FIELD, 6)
    ell[3] = 0
    return [eng.fp12_sparse_mul(c.fp("f", f), c.fp("ell", ell))]


@case("gt_pow_batch")
def _gt_pow(eng, c, pool, nm):
    rng = Xoshiro(SEED + 18)
    k = limbs([rng.u256() for _ in range(6)] + [0, U256 - 1])
    return [eng.gt_pow(c.fp("gt", pool["gt"]), k)]


@case("svdw_map_batch")
def _svdw(eng, c, pool, nm):
    return list(eng.svdw_map(c.fp("u", _fp_values(N_FIELD, SEED + 19))))


# ---- groups
def _g1_off_curve(n, seed):
    return rand_fp_array(Xoshiro(seed), n, 2)


@case("g1_scalar_mul_batch", "g2_scalar_mul_batch", "g2_scalar_mul_subgroup_batch")
def _smul(eng, c, pool, nm):
    pts = pool["g1"] if nm.startswith("g1") else pool["g2"]
    rng = Xoshiro(SEED + 20)
    k = limbs([rng.fp() for _ in range(D - 2)] + [0, 1])
    inf = _flags(D, 3)
    return list(eng._scalar_mul("sylow_hip_" + nm, pts.shape[1], c.fp("p_xy", pts), c.flag("p_inf", inf), k))


@case("g1_add_batch", "g1_sub_batch", "g2_add_batch", "g2_sub_batch")
def _gadd(eng, c, pool, nm):
    pts = pool["g1"] if nm.startswith("g1") else pool["g2"]
    w = pts.shape[1]
    a, b = pts.copy(), _tile(pts, D, 5)
    b[1::4] = a[1::4]                                            # P + P (the doubling case of the complete formulas)
    neg = eng.g1_sub if w == 8 else eng.g2_sub
    b[2::4] = neg(np.zeros_like(a[2::4]), a[2::4], np.ones(len(a[2::4]), np.uint8))[0]  # -P: P + (-P) = identity
    return list(eng._group_binop("sylow_hip_" + nm, w, c.fp("a_xy", a), c.fp("b_xy", b), c.flag("a_inf", _flags(D, 1)), c.flag("b_inf", _flags(D, 4, 7))))


@case("g1_double_batch", "g2_double_batch")
def _gdbl(eng, c, pool, nm):
    pts = pool["g1"] if nm.startswith("g1") else pool["g2"]
    return list(eng._double("sylow_hip_" + nm, pts.shape[1], c.fp("a_xy", pts), c.flag("a_inf", _flags(D, 2))))


def _proj(pool, nm):
    return pool["p1"] if nm.startswith("g1") else pool["p2"]


@case("g1_normalize_batch", "g2_normalize_batch")
def _normalize(eng, c, pool, nm):
    p = _proj(pool, nm)
    return list(eng._normalize("sylow_hip_" + nm, p.shape[1], p.shape[1] * 2 // 3, c.fp("p_xyz", p)))


@case("g1_projective_new_batch", "g2_projective_new_batch")
def _projective_new(eng, c, pool, nm):
    p = _proj(pool, nm).copy()
    p[3::8, 4:8] = p[5::8, 4:8]                                   # off the curve
    if nm.startswith("g2"):
        pts = crafted_g2_points(4)                                # on the twist, outside the r-torsion
        for j, (x, y) in enumerate(pts):
            p[6 + 8 * j] = limbs([*x, *y, 1, 0]).reshape(24)
    return [eng._projective_new("sylow_hip_" + nm, p.shape[1], c.fp("p_xyz", p))]


@case("g1_ct_eq_batch", "g2_ct_eq_batch")
def _ct_eq(eng, c, pool, nm):
    p = _proj(pool, nm)
    w = p.shape[1]
    b = _tile(p, D, 3)
    b[1::3] = p[1::3]                                             # the same words
    b[0::8] = np.roll(p[0::8], 1, axis=0)                        # identity against identity in another Z = 0 form
    # the same point under another Z: (X s, Y s, Z s)
    aff = pool["g1"] if w == 12 else pool["g2"]
    one = np.zeros((D, w // 3), dtype=np.uint64)
    one[:, 0] = 1
    b[2::5] = np.concatenate([aff, one], axis=1)[2::5]
    return [eng._ct_eq("sylow_hip_" + nm, w, c.fp("a_xyz", p), c.fp("b_xyz", b))]


@case("g1_lincomb_batch")
def _lincomb(eng, c, pool, nm):
    rng = Xoshiro(SEED + 21)
    nj, nt = 5, 9
    p = _tile(pool["g1"], nj * nt, 3)
    k = limbs([rng.fp() for _ in range(nj * nt)])
    return list(eng.g1_lincomb(c.fp("p_xy", p), k, nj, nt, p_inf=c.flag("p_inf", _flags(nj * nt, 2, 6))))


@case("g1_msm", "g1_msm_tuned")
def _msm(eng, c, pool, nm):
    rng = Xoshiro(SEED + 22)
    n = 3 * D
    p = _tile(pool["g1"], n, 5)
    k = limbs([rng.fp() for _ in range(n)])
    kw = dict(window=6, min_n=0) if nm == "g1_msm_tuned" else {}            # the bucket route; the plain call takes the per-point route
    return list(eng.g1_msm(c.fp("p_xy", p), k, p_inf=c.flag("p_inf", _flags(n, 5, 9)), **kw))


@case("g1_sum_batch")
def _sum(eng, c, pool, nm):
    p = np.concatenate([pool["g1"], pool["g1"][:5]])             # repeated points: the doubling case of the fold
    return list(eng.g1_sum(c.fp("p_xy", p), p_inf=c.flag("p_inf", _flags(p.shape[0], 1, 5))))


@case("g1_on_curve_batch")
def _on_curve(eng, c, pool, nm):
    p = np.concatenate([pool["g1"], _g1_off_curve(16, SEED + 23)])
    return [eng.g1_on_curve(c.fp("p_xy", p), p_inf=c.flag("p_inf", _flags(p.shape[0], 3, 4)))]


def _g2_mixed(pool):
    """pool points, twist points outside the r-torsion, points off the twist"""
    if "g2_mixed" not in pool:
        extra = [limbs([*x, *y]).reshape(16) for x, y in crafted_g2_points(6)]
        pool["g2_mixed"] = np.concatenate([pool["g2"], np.array(extra), rand_fp_array(Xoshiro(SEED + 24), 6, 4)])
    return pool["g2_mixed"]


@case("g2_psi_batch")
def _psi(eng, c, pool, nm):
    q = _g2_mixed(pool)
    return list(eng.g2_psi(c.fp("q_xy", q), q_inf=c.flag("q_inf", _flags(q.shape[0], 2, 5))))


@case("g2_subgroup_check_batch")
def _subgroup(eng, c, pool, nm):
    q = _g2_mixed(pool)
    return [eng.g2_subgroup_check(c.fp("q_xy", q), q_inf=c.flag("q_inf", _flags(q.shape[0], 2, 5)))]


@case("g1_to_be_bytes_batch", "g2_to_be_bytes_batch")
def _to_bytes(eng, c, pool, nm):
    pts = pool["g1"] if nm.startswith("g1") else pool["g2"]
    f = eng.g1_to_be_bytes if nm.startswith("g1") else eng.g2_to_be_bytes
    return [np.frombuffer(b"".join(f(c.fp("p_xy", pts), c.flag("p_inf", _flags(D, 1, 6)))), dtype=np.uint8)]


# ---- pairings, at one size per route
@pytest.fixture(scope="module")
def sizes():
    import torch
    return route_sizes(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def verify_sizes():
    import torch
    return route_sizes(torch.cuda.get_device_properties(0).multi_processor_count, verify=True)


ROUTED = {"sylow_hip_miller_loop_batch", "sylow_hip_final_exp_batch", "sylow_hip_pairing_batch", "sylow_hip_pairing_host"}
ROUTED_VERIFY = {"sylow_hip_bls_verify_batch", "sylow_hip_bls_verify_fused_batch", "sylow_hip_bls_verify_two_pairings_batch",
                 "sylow_hip_bls_verify_same_signer_batch", "sylow_hip_bls_verify_line_table_batch", "sylow_hip_bls_verify_host"}
ROUTE = {"n": 64}                                                 # the batch size of the routed cases (set per parametrized run)


def _pq(pool, n):
    return _tile(pool["g1"], n, 3), _tile(pool["g2"], n, 5)


@case("miller_loop_batch")
def _miller(eng, c, pool, nm):
    p, q = _pq(pool, ROUTE["n"])
    return [eng.miller_loop(c.fp("p_xy", p), c.fp("q_xy", q))]


@case("final_exp_batch")
def _final_exp(eng, c, pool, nm):
    n = ROUTE["n"]
    f = _tile(rand_fp_array(Xoshiro(SEED + 25), 97, 12), n, 1)
    f[n // 2] = 0
    f[n // 2, 0] = 1                                              # the unit
    return [eng.final_exp(c.fp("f", f))]


@case("pairing_batch", "pairing_host")
def _pairing(eng, c, pool, nm):
    n = ROUTE["n"]
    p, q = _pq(pool, n)
    pi, qi = _flags(n, 1, 13), _flags(n, 5, 17)
    if nm == "pairing_host":
        return [eng.pairing(c.fp("p_aos", p), c.fp("q_aos", q), c.flag("p_inf", pi), c.flag("q_inf", qi))]
    return [eng.pairing(c.fp("p_xy", p), c.fp("q_xy", q), c.flag("p_inf", pi), c.flag("q_inf", qi), pipelined=False)]


OFFSETS = np.array([0, 1, 1, 3, 7, 8, 14, 30, 31, 40], dtype=np.uint64)   # jobs of 1, 0, 2, 4, 1, 6, 16, 1, 9 pairs


@case("multi_pairing_batch", "pairing_product_batch", "pairing_product_partial_batch", "pairing_product_all")
def _multi(eng, c, pool, nm):
    n = int(OFFSETS[-1])
    p, q = _pq(pool, n)
    pi, qi = _flags(n, 2, 9), _flags(n, 3, 11)
    args = lambda: (c.fp("p_xy", p), c.fp("q_xy", q))
    out = []
    for skip in (False, True):
        fl = dict(p_inf=c.flag("p_inf", pi), q_inf=c.flag("q_inf", qi), skip_infinity=skip)
        if nm == "multi_pairing_batch":
            out += list(eng.multi_pairing(*args(), OFFSETS, **fl))
        elif nm == "pairing_product_batch":
            out += [*eng.pairing_product(*args(), **fl)]
        elif nm == "pairing_product_partial_batch":
            out += [eng.pairing_product_partial(*args(), **fl)]
        else:
            out += [*eng.pairing_product_all(*args(), **fl)]
    return out


@case("glued_miller_loop_batch")
def _glued(eng, c, pool, nm):
    p, q = _pq(pool, int(OFFSETS[-1]))
    return [eng.glued_miller_loop(c.fp("p_xy", p), c.fp("q_xy", q), OFFSETS)]


@case("fp12_product_final_exp")
def _prod_fe(eng, c, pool, nm):
    parts = rand_fp_array(Xoshiro(SEED + 26), 5, 12)
    return [*eng.fp12_product_final_exp(c.fp("parts", parts)), *eng.fp12_product_final_exp(c.fp("parts", pool["gt"][:3]))]


@case("g2_precompute_batch")
def _precompute(eng, c, pool, nm):
    return [eng.g2_precompute(c.fp("q_xy", pool["g2"][:16]))]


@pytest.fixture(scope="module")
def coeffs(engine, pool):
    return engine.g2_precompute(pool["g2"][:12])


@case("miller_loop_precomputed_batch", "glued_miller_loop_precomputed_batch")
def _ml_pre(eng, c, pool, nm):
    co = pool["coeffs"]
    n = int(OFFSETS[-1])
    p = _tile(pool["g1"], n, 7)
    idx = (np.arange(n) * 5) % co.shape[0]
    if nm == "miller_loop_precomputed_batch":
        return [eng.miller_loop_precomputed(c.fp("coeffs", co), c.fp("p_xy", p), table_idx=idx)]
    return [eng.glued_miller_loop_precomputed(c.fp("coeffs", co), c.fp("p_xy", p), OFFSETS, table_idx=idx)]


# ---- BLS
def _verify_inputs(pool, n):
    pk, sig = _tile(pool["pk"], n), _tile(pool["sig"], n)
    return pk, sig, _msgs_for(pool, n), _flags(n, 3, 19), _flags(n, 6, 23)


@case("bls_verify_batch", "bls_verify_fused_batch", "bls_verify_two_pairings_batch", "bls_verify_host")
def _verify(eng, c, pool, nm):
    pk, sig, msgs, ki, si = _verify_inputs(pool, ROUTE["n"])
    host = nm == "bls_verify_host"
    a = "_aos" if host else "_xy"
    kw = dict(fused=nm == "bls_verify_fused_batch", two_pairings=nm == "bls_verify_two_pairings_batch", pipelined=host)
    return [eng.bls_verify(c.fp("pk" + a, pk), msgs, c.fp("sig" + a, sig), pk_inf=c.flag("pk_inf", ki), sig_inf=c.flag("sig_inf", si), **kw)]


def _same_signer_inputs(eng, pool, n):
    rng = Xoshiro(SEED + 27)
    sk = limbs([rng.fp()])
    key = pool.setdefault("signer", {})
    if n not in key:
        msgs = [b"same signer %d" % (i % 97) for i in range(n)]
        sig, _ = eng.bls_sign(np.repeat(sk, n, 0), msgs)
        pk, _ = eng.g2_generator_mul(sk)
        msgs = [m if i % 6 != 5 else b"forged" for i, m in enumerate(msgs)]
        key[n] = (pk, sig, msgs)
    return key[n]


@case("bls_verify_same_signer_batch")
def _same_signer(eng, c, pool, nm):
    n = ROUTE["n"]
    pk, sig, msgs = _same_signer_inputs(eng, pool, n)
    return [eng.bls_verify_same_signer(c.fp("pk_xy", pk), msgs, c.fp("sig_xy", sig), pk_inf=c.flag("pk_inf", np.zeros(1, np.uint8)),
                                       sig_inf=c.flag("sig_inf", _flags(n, 2, 29)))]


@case("g2_line_table")
def _line_table(eng, c, pool, nm):
    out = []
    for i in (0, 7):
        t = eng.g2_line_table(c.fp("q_xy", pool["g2"][i:i + 1]))
        out.append(t.download())
    return out


@case("bls_verify_line_table_batch")
def _verify_line_table(eng, c, pool, nm):
    n = ROUTE["n"]
    pk, sig, msgs = _same_signer_inputs(eng, pool, n)
    table = eng.g2_line_table(pk)
    return [eng.bls_verify_line_table(table, msgs, c.fp("sig_xy", sig), pk_inf=c.flag("pk_inf", np.zeros(1, np.uint8)),
                                      sig_inf=c.flag("sig_inf", _flags(n, 2, 29)))]


@case("bls_aggregate_partial_batch", "bls_aggregate_verify_batch", "bls_weighted_partial_batch", "bls_batch_verify_weighted")
def _aggregate(eng, c, pool, nm):
    n = 24
    out = []
    for n_pk in (n, 1):
        if n_pk == 1:
            pk, sig, msgs = _same_signer_inputs(eng, pool, n)
        else:
            pk, sig, msgs, _, _ = _verify_inputs(pool, n)
            if nm in ("bls_aggregate_verify_batch",):
                msgs = [pool["msgs"][i] for i in range(n)]        # all valid: the product is the identity
        ki, si = np.zeros(n_pk, np.uint8), _flags(n, 4, 7)
        w = limbs([Xoshiro(SEED + 28 + i).next() for i in range(n)])
        dpk, dsig = eng.to_device_soa(c.fp("pk_xy", pk), 16), eng.to_device_soa(c.fp("sig_xy", sig), 8)
        fk, fs = c.flag("pk_inf", ki), c.flag("sig_inf", si)
        dki, dsi = eng._flags(fk, n_pk), eng._flags(fs, n)
        dm, doff = eng._msgs(msgs)
        dw = eng.to_device_soa(w, 4)
        dgt, dis = eng.empty((48, 1)), eng.empty((1,), np.uint8)
        dis.upload(np.full(1, 7, np.uint8))
        head = (dpk.ptr, eng._ptr(dki), n_pk, dm.ptr, doff.ptr, dsig.ptr, eng._ptr(dsi))
        if nm == "bls_aggregate_partial_batch":
            eng._call("sylow_hip_" + nm, *head, n, dgt.ptr)
        elif nm == "bls_aggregate_verify_batch":
            eng._call("sylow_hip_" + nm, *head, n, None, dgt.ptr, dis.ptr)
        elif nm == "bls_weighted_partial_batch":
            eng._call("sylow_hip_" + nm, *head, dw.ptr, n, dgt.ptr)
        else:
            eng._call("sylow_hip_" + nm, *head, dw.ptr, n, None, dgt.ptr, dis.ptr)
        out += [dgt.download(), dis.download()]
    return out


# ---- the GPU tests -------------------------------------------------------------------------------------------------------------
PLAIN = sorted(set(CASES) - ROUTED - ROUTED_VERIFY)


@pytest.fixture(scope="module")
def pool_all(engine, pool, coeffs):
    pool["coeffs"] = coeffs
    return pool


@pytest.mark.gpu
@pytest.mark.parametrize("name", PLAIN)
def test_entry_point_reduces_representatives(engine, pool_all, name):
    base = check_row(engine, name, lambda eng, c: CASES[name](eng, c, pool_all))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["one", "two_per_wave", "quad", "round_tail"])
@pytest.mark.parametrize("name", sorted(ROUTED | ROUTED_VERIFY))
def test_routed_entry_point_reduces_representatives(engine, pool_all, sizes, verify_sizes, name, route):
    n = ROUTE["n"] = (verify_sizes if name in ROUTED_VERIFY else sizes)[route]
    try:
        base = check_row(engine, name, lambda eng, c: CASES[name](eng, c, pool_all))
    finally:
        ROUTE["n"] = 64
    if name in ROUTED_VERIFY:
        ok = np.asarray(base[0])
        assert ok.any() and (n < 7 or not ok.all()), f"{name}: the batch should hold valid and invalid signatures"


@pytest.mark.gpu
def test_projective_zero_as_p_and_2p_is_the_identity(engine, pool_all):
    """Z = p and Z = 2p (== 0 under Fp::new) in normalize, projective_new and ct_eq, written explicitly rather than drawn"""
    for w, nm in ((12, "g1"), (24, "g2")):
        p = (pool_all["p1"] if w == 12 else pool_all["p2"])[:8].copy()
        zw = w // 3
        for j, k in enumerate((1, 2, 5, 1, 2, 5, 1, 2)):
            z = [k * P] + [0] * (zw // 4 - 1)
            p[j, 2 * zw:] = limbs(z).reshape(zw)
        xy, inf = getattr(engine, nm + "_normalize")(p)
        assert inf.all()
        st = getattr(engine, nm + "_projective_new")(p)
        canon = p.copy()
        canon[:, 2 * zw:] = 0
        assert np.array_equal(st, getattr(engine, nm + "_projective_new")(canon))
        ident = np.zeros((8, w), dtype=np.uint64)
        ident[:, zw] = 1                                           # (0, 1, 0)
        assert getattr(engine, nm + "_ct_eq")(p, ident).all()
