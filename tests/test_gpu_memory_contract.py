"""Where the entry points touch memory (include/sylow_hip.h, Conventions: "a call reads and writes only the extents its @shape line
gives; every element of every output array is written on success; arrays declared const are not modified").

Every call here runs on a GuardedEngine (guarded_engine.py: each buffer between two guard bands, the whole allocation pre-filled) under
two fill bytes, 0x5A and 0xFF -- under 0xFF every word past an input's extent is >= p and every flag byte past n is set -- and on the
plain session engine.  The audit after each guarded call catches a write outside an array, a modified const input and a write beyond an
output's @shape extent.  The outputs of the two guarded runs must be bit-identical: an element no kernel stores keeps the fill, and a
result that leaks from a dead tail lane's clamped or over-read input changes with it.  Both must equal the plain engine's output.  The
same comparison runs on the device bytes of every output inside its @shape extent (GuardedEngine.written), because the Python layer
returns some one-byte outputs as a bool (is_one), and both fill bytes are true.

  a. the harness is live: a stray byte just outside an array and an output nobody wrote are both reported;
  b. every driver of the input-contract files (CASES of test_gpu_input_contract*.py), once;
  c. the drivers of DRIVERS at n = 1 .. 257, one either side of a lane pair, a quad, an eight-lane group, a half wavefront, a wavefront,
     two wavefronts and a 256-lane block, on every forced route of the pairing, verification and wide layouts;
  e. the four host-array entry points between guard bands in host memory.

The last test of the file asserts that every @shape array of every driven entry point (MEMORY_CONTRACT of test_guarded_engine.py) went
through the audit, so it needs the whole file to have run."""
import glob
import importlib
import os
import time

import numpy as np
import pytest

import test_gpu_input_contract as T
from guarded_engine import FILLS, GUARD, GuardedEngine, audit_bytes
from helpers import P, SEED, U256, Xoshiro, limbs, rand_fp_array
from test_gpu_input_contract import coeffs, pool, pool_all  # noqa: F401  (fixtures)

for _f in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_input_contract_*.py"))):
    importlib.import_module(os.path.basename(_f)[:-3])              # their rows and cases register in T.CONTRACT / T.CASES

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 7, 8, 9, 15, 17, 31, 33, 63, 65, 127, 129, 255, 257)
NMAX = 257
LEAK = "output depends on bytes outside an input's extent or on the output's previous contents"
HOST_AUDITED = set()             # (entry point, parameter) of the host arrays audited in section e
WALL = {"t0": None}


@pytest.fixture(scope="module")
def guarded(engine):
    WALL["t0"] = time.time()
    return GuardedEngine(0)


def same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, f"{what}: output {i} has shapes {x.shape} and {y.shape}"
        if not np.array_equal(x, y):
            at = np.flatnonzero(x.reshape(-1) != y.reshape(-1))
            raise AssertionError(f"{what}: output {i} differs in {at.size} of {x.size} elements, first at flat index {int(at[0])} "
                                 f"({x.reshape(-1)[at[0]]!r} against {y.reshape(-1)[at[0]]!r})")


def three_runs(guarded, engine, run, what):
    """run(eng) -> list of arrays: guarded under both fills (audited inside), then plain"""
    outs, raw = [], []
    for fill in FILLS:
        guarded.fill = fill
        del guarded.written[:]
        outs.append([np.asarray(o) for o in run(guarded)])
        raw.append(list(guarded.written))
    guarded.fill = FILLS[0]
    del guarded.written[:]
    same(outs[0], outs[1], f"{what}: fill 0x{FILLS[0]:02X} against 0x{FILLS[1]:02X}: {LEAK}")
    # the same on the device bytes themselves: what the Python layer returns as a bool (is_one) is true under either fill
    # (a driver may make its inputs with calls of its own on the first run and keep them: the logs are matched per array from the last call back)
    by_array = [{}, {}]
    for log, arrays in zip(raw, by_array):
        for name, param, x in log:
            arrays.setdefault((name, param), []).append(x)
    for (name, param), ys in by_array[1].items():
        xs = by_array[0].get((name, param), [])
        assert xs, f"{what}: {name} ran under 0x{FILLS[1]:02X} and not under 0x{FILLS[0]:02X}"
        k = min(len(xs), len(ys))
        same(xs[-k:], ys[-k:], f"{what}: fill 0x{FILLS[0]:02X} against 0x{FILLS[1]:02X}, the bytes of {param} after {name}: {LEAK}")
    same(outs[0], [np.asarray(o) for o in run(engine)], f"{what}: the guarded engine against the plain engine")
    return outs[0]


class options:
    """route selectors set in process, restored on the way out"""

    def __init__(self, engine, **opts):
        self.engine, self.opts, self.prev = engine, opts, {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.prev[k] = self.engine.get_option(k)
        for k, v in self.opts.items():
            self.engine.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.engine.set_option(k, v)


# ================================================================ a. the harness is live ============================================
def _fp_add_on(guarded, da, db, do, n):
    guarded._call("sylow_hip_fp_add_batch", da.ptr, db.ptr, do.ptr, n)


@pytest.mark.parametrize("where", ["past the end", "in front"])
def test_a_stray_byte_outside_an_array_is_reported(guarded, where):
    n = 5
    a = rand_fp_array(Xoshiro(SEED + 0xA1), n, 1)
    da, db, do = guarded.to_device_soa(a, 4), guarded.to_device_soa(a, 4), guarded.empty((4, n))
    _fp_add_on(guarded, da, db, do, n)                              # clean
    one = np.array([guarded.fill ^ 0xFF], dtype=np.uint8)
    at = do.ptr + do.nbytes if where == "past the end" else do.ptr - 1
    assert guarded.lib.sylow_hip_memcpy_h2d(at, one.ctypes.data, 1, guarded.stream) == 0
    guarded.sync()
    with pytest.raises(AssertionError) as e:
        _fp_add_on(guarded, da, db, do, n)
    msg = str(e.value)
    assert "sylow_hip_fp_add_batch" in msg and " out" in msg, msg
    assert msg.endswith(f"at byte offset {do.nbytes}" if where == "past the end" else "at byte offset -1"), msg
    # the same for an input: the stray byte is found whichever argument it sits next to
    at = da.ptr + da.nbytes if where == "past the end" else da.ptr - 1
    do2 = guarded.empty((4, n))
    assert guarded.lib.sylow_hip_memcpy_h2d(at, one.ctypes.data, 1, guarded.stream) == 0
    guarded.sync()
    with pytest.raises(AssertionError) as e:
        _fp_add_on(guarded, da, db, do2, n)
    msg = str(e.value)
    assert (f"past the end of a ({da.nbytes} bytes)" if where == "past the end" else "in front of a,") in msg, msg


def test_the_raw_bytes_of_every_output_are_logged(guarded):
    """what three_runs compares between the fills besides the returned values: the device bytes of each non-const argument"""
    n = 3
    a = rand_fp_array(Xoshiro(SEED + 0xA2), n, 1)
    da, do = guarded.to_device_soa(a, 4), guarded.empty((4, n))
    del guarded.written[:]
    _fp_add_on(guarded, da, da, do, n)
    assert [(w[0], w[1]) for w in guarded.written] == [("sylow_hip_fp_add_batch", "out")]
    assert guarded.written[0][2].tobytes() == do.download().tobytes() and guarded.written[0][2].size == 32 * n
    del guarded.written[:]


def test_an_output_nobody_wrote_differs_between_the_fills(guarded, engine):
    def unwritten(eng):
        return [eng.empty((4, 3)).download(), eng.empty((3,), np.uint8).download()]
    with pytest.raises(AssertionError, match="output depends on bytes outside"):
        three_runs(guarded, engine, unwritten, "no call")

    def unwritten_and_returned_as_a_bool(eng):                      # 0x5A and 0xFF are both true: only the logged byte tells
        if eng is guarded:
            guarded.written.append(("no call", "is_one", eng.empty((1,), np.uint8).download()))
        return [np.array([True])]
    with pytest.raises(AssertionError, match="the bytes of is_one after no call: output depends on bytes outside"):
        three_runs(guarded, engine, unwritten_and_returned_as_a_bool, "no call")


# ================================================================ b. every input-contract driver, once ================================
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_input_contract_driver_stays_inside_its_buffers(guarded, engine, pool_all, name):
    out = three_runs(guarded, engine, lambda eng: T.CASES[name](eng, T.Ctx(), pool_all), name)
    assert out, name


# ================================================================ c. ragged sizes ======================================================
class Data:
    pass


def _flag_rows(n, step, first):
    f = np.zeros(n, dtype=np.uint8)
    f[first::step] = 1
    return f


@pytest.fixture(scope="module")
def data(engine, pool):
    """every input at n = 257, made once; the drivers slice.  Row 0 of each batch is flagged as the identity in the first flag array."""
    import evm_model
    import test_gpu_input_contract_groth16 as G16
    import test_gpu_input_contract_kzg as KZG
    d = Data()
    n = NMAX
    d.pool = pool
    d.g1, d.g2 = T._tile(pool["g1"], n, 3), T._tile(pool["g2"], n, 5)
    d.fa, d.fb = _flag_rows(n, 11, 0), _flag_rows(n, 13, 5)
    rng = Xoshiro(SEED + 0xC0)
    d.k = limbs([rng.fp() for _ in range(n - 3)] + [0, 1, P - 1])
    d.k[4] = 0                                                      # k = 0: an identity among the outputs of every size above 4
    d.fp_a, d.fp_b = T._fp_values(n, SEED + 0xC1), T._fp_values(n, SEED + 0xC2)[::-1].copy()
    d.sq = d.fp_a.copy()
    d.sq[::2] = engine.fp_sqr(d.fp_a[::2])                          # squares at the even rows, random values (half of them non-squares) between
    d.e = limbs([rng.u256() for _ in range(n - 3)] + [0, 1, U256 - 1])
    d.tower = {w: rand_fp_array(Xoshiro(SEED + 0xC3 + w), n, w // 4) for w in (8, 24, 48)}
    for w in d.tower:
        d.tower[w][1] = 0                                           # a zero row (its inverse is zero by convention)
    d.blobs = [bytes(r) for r in np.ascontiguousarray(d.fp_a[:, ::-1]).astype(">u8").view(np.uint8).reshape(n, 32)]
    for i in range(2, n, 9):
        d.blobs[i] = b"\xff" * 32                                   # >= p and >= r: status 0 (CtOption none)
    d.msgs = [b"ragged %d" % i + bytes([i & 255]) * (i % 5) for i in range(n)]
    d.msgs[3] = b""
    d.sk = limbs([rng.fp() for _ in range(n)])
    d.sk[0] = 0                                                     # sk = 0: the identity signature
    # verification rows: pool signatures tiled, every fifth message another one
    d.pk, d.sig, d.vmsgs, _, _ = T._verify_inputs(pool, n)
    d.ss_pk, d.ss_sig, d.ss_msgs = T._same_signer_inputs(engine, pool, n)
    d.p1, d.p2 = T._tile(pool["p1"], n, 1), T._tile(pool["p2"], n, 1)
    d.g2_mixed = T._tile(T._g2_mixed(pool), n, 7)
    d.f12 = d.tower[48].copy()
    d.f12[1, 0] = 1
    # wire formats: valid points, identities (flagged rows) and rows of bytes that decode to nothing
    d.g1_be, d.g2_be = engine.g1_to_be_bytes(d.g1, d.fa), engine.g2_to_be_bytes(d.g2, d.fb)
    junk = np.random.default_rng(SEED & 0xFFFF).integers(0, 256, size=(n, 128), dtype=np.uint8)
    for i in range(1, n, 6):
        d.g1_be[i], d.g2_be[i] = bytes(junk[i, :64]), bytes(junk[i])
    jobs = evm_model.build_pool(SEED)
    d.evm_add = [evm_model.right_pad(jobs.add[i % len(jobs.add)].data, 128) for i in range(n)]
    d.evm_mul = [evm_model.right_pad(jobs.mul[i % len(jobs.mul)].data, 96) for i in range(n)]
    whole = [j.data for j in jobs.pair if len(j.data) % 192 == 0]
    one = [x for x in whole if len(x) == 192]
    d.evm_pair = [whole[(7 * i) % len(whole)] for i in range(n)]
    d.evm_pair_last = one[0]
    d.kzg = KZG.instance().take(np.arange(n) % KZG.N)
    d.g16 = G16.instance().take(np.arange(n) % G16.N)
    d.polys = rand_fp_array(Xoshiro(SEED + 0xC4), (n + 1) * 8, 1).reshape(n + 1, 8, 4)
    d.polys[2] = d.polys[2, 0]                                      # a constant polynomial: zero quotient, identity proof
    return d


def _raw_fixed(eng, name, rows, n):
    d_in = eng.to_device(np.frombuffer(b"".join(rows[:n]), dtype=np.uint8))
    d_out, d_st = eng.empty((64 * n,), np.uint8), eng.empty((n,), np.uint8)
    eng._call(name, d_in.ptr, d_out.ptr, d_st.ptr, n)
    return [d_out.download(), d_st.download()]


def _raw_pair(eng, jobs):
    counts = [len(j) // 192 for j in jobs]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    d_in, d_off = eng.to_device(np.frombuffer(b"".join(jobs), dtype=np.uint8)), eng.to_device(off)
    d_res, d_st = eng.empty((len(jobs),), np.uint8), eng.empty((len(jobs),), np.uint8)
    eng._call("sylow_hip_evm_ecpairing_batch", d_in.ptr, d_off.ptr, len(jobs), int(off[-1]), d_res.ptr, d_st.ptr)
    return [d_res.download(), d_st.download()]


def _transpose(eng, name, a):
    n, w = a.shape
    src = eng.to_device(a if name == "sylow_hip_aos_to_soa" else np.ascontiguousarray(a.T))
    dst = eng.empty((w, n) if name == "sylow_hip_aos_to_soa" else (n, w))
    eng._call(name, src.ptr, dst.ptr, w, n)
    return [dst.download()]


def _flags_reduce(eng, d, n):
    out = []
    for f in (np.ones(n, np.uint8), 1 - d.fa[:n]):                  # all set; row 0 clear
        df = eng.to_device(f)
        out += [np.array([eng.flags_all(df)]), np.array([eng.all_valid(df)])]
    return out


def _f29_limbs(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 28, size=(n, 9), dtype=np.int64).astype(np.int32)


def _ragged_offsets(n):
    """job offsets over n pairs: jobs of 1, 0, 2, 4, ... pairs, the last job holding exactly one pair"""
    off = [0]
    for step in (1, 0, 2, 4, 1, 6, 16, 3, 9, 33, 64, 127):
        if off[-1] + step >= n:
            break
        off.append(off[-1] + step)
    if off[-1] < n - 1:
        off.append(n - 1)
    return np.array(off + [n], dtype=np.uint64)


def _multi_pairing(eng, d, n):
    off = _ragged_offsets(n)
    out = []
    for skip in (False, True):
        out += list(eng.multi_pairing(d.g1[:n], d.g2[:n], off, p_inf=d.fa[:n], q_inf=d.fb[:n], skip_infinity=skip))
    return out


def _lincomb(eng, d, n):
    """n jobs of 1 and of 3 terms (term-major rows)"""
    out = []
    for nt in (1, 3):
        rows = min(n * nt, NMAX)
        nj = rows // nt
        out += list(eng.g1_lincomb(d.g1[:nj * nt], d.k[:nj * nt], nj, nt, p_inf=d.fa[:nj * nt]))
    return out


def _evm_pairing(eng, d, n):
    return _raw_pair(eng, d.evm_pair[:n - 1] + [d.evm_pair_last])


def _kzg_args(g, n):
    return g.c[:n], g.z_words()[:n], g.y_words()[:n], g.pi[:n]


def _g16_verify(eng, d, n):
    g = d.g16
    return [eng.groth16_verify(g.vk(), g.a[:n], g.b[:n], g.c[:n], g.input_words()[:n], a_inf=d.fb[:n], c_inf=_flag_rows(n, 17, 0))]


def _bls_verify(form):
    kw = dict(fused=form == "fused", two_pairings=form == "two_pairings", pipelined=False)
    return lambda eng, d, n: [eng.bls_verify(d.pk[:n], d.vmsgs[:n], d.sig[:n], pk_inf=d.fa[:n], sig_inf=d.fb[:n], **kw)]


def _fext(op):
    def run(eng, d, n):
        out = []
        for w in (8, 24, 48):
            b = None if op == "neg" else d.fp_b[:n] if op == "scale" else d.tower[w][:n][::-1]
            out.append(eng.fext_op(op, d.tower[w][:n], b))
        return out
    return run


def _sparse(n, seed):
    """a CSR matrix of n rows over 5 columns: row i holds i % 4 entries (empty rows included), one column index past the last column"""
    counts = [i % 4 for i in range(n)]
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    nnz = int(row_ptr[-1])
    col = (np.arange(nnz, dtype=np.uint64) * 3) % 5
    if nnz:
        col[-1] = 5
    return row_ptr, col, rand_fp_array(Xoshiro(seed), max(nnz, 1), 1)[:nnz]


def _spmv(eng, d, n, **kw):
    return [eng.fr_spmv(_sparse(n, SEED + 0xC5), d.polys[:3, :5], n_out=n + 2, **kw)]


def _groups(m):
    return [0, 1, 1, m] if m > 1 else [0, 0, 1]


PAIRING = {
    "sylow_hip_pairing_batch": lambda eng, d, n: [eng.pairing(d.g1[:n], d.g2[:n], d.fa[:n], d.fb[:n], pipelined=False)],
    "sylow_hip_miller_loop_batch": lambda eng, d, n: [eng.miller_loop(d.g1[:n], d.g2[:n])],
    "sylow_hip_final_exp_batch": lambda eng, d, n: [eng.final_exp(d.f12[:n])],
}
VERIFY = {
    "sylow_hip_bls_verify_batch": _bls_verify("default"),
    "sylow_hip_bls_verify_fused_batch": _bls_verify("fused"),
    "sylow_hip_bls_verify_two_pairings_batch": _bls_verify("two_pairings"),
    "sylow_hip_bls_verify_same_signer_batch": lambda eng, d, n: [eng.bls_verify_same_signer(d.ss_pk, d.ss_msgs[:n], d.ss_sig[:n], sig_inf=d.fa[:n])],
    "sylow_hip_bls_verify_line_table_batch": lambda eng, d, n: [eng.bls_verify_line_table(eng.g2_line_table(d.ss_pk), d.ss_msgs[:n], d.ss_sig[:n],
                                                                                          sig_inf=d.fa[:n])],
}
WIDE = {
    "sylow_hip_g1_scalar_mul_batch": lambda eng, d, n: list(eng.g1_scalar_mul(d.g1[:n], d.k[:n], d.fa[:n])),
    "sylow_hip_bls_sign_batch": lambda eng, d, n: list(eng.bls_sign(d.sk[:n], d.msgs[:n])),
    "sylow_hip_bls_sign_expander_batch": lambda eng, d, n: list(eng.bls_sign(d.sk[:n], d.msgs[:n], expander="xmd_sha256", dst=b"MEMORY-CONTRACT")),
    "sylow_hip_hash_to_g1_batch": lambda eng, d, n: list(eng.hash_to_g1(d.msgs[:n])),
    "sylow_hip_hash_to_g1_expander_batch": lambda eng, d, n: list(eng.hash_to_g1(d.msgs[:n], dst=b"MEMORY-CONTRACT", expander="xof_shake128")),
    "sylow_hip_evm_ecmul_batch": lambda eng, d, n: _raw_fixed(eng, "sylow_hip_evm_ecmul_batch", d.evm_mul, n),
}
GROUPS = {
    "sylow_hip_g2_scalar_mul_batch": lambda eng, d, n: list(eng.g2_scalar_mul(d.g2[:n], d.k[:n], d.fa[:n])),
    "sylow_hip_g2_scalar_mul_subgroup_batch": lambda eng, d, n: list(eng.g2_scalar_mul(d.g2[:n], d.k[:n], d.fa[:n], subgroup=True)),
    "sylow_hip_g1_generator_mul_batch": lambda eng, d, n: list(eng.g1_generator_mul(d.k[:n])),
    "sylow_hip_g2_generator_mul_batch": lambda eng, d, n: list(eng.g2_generator_mul(d.k[:n])),
    "sylow_hip_g1_add_batch": lambda eng, d, n: list(eng.g1_add(d.g1[:n], d.g1[:n][::-1], d.fa[:n], d.fa[:n])),      # row 0: O + O
    "sylow_hip_g1_sub_batch": lambda eng, d, n: list(eng.g1_sub(d.g1[:n], d.g1[:n][::-1], d.fa[:n], d.fa[:n])),      # the middle row: P - P
    "sylow_hip_g1_double_batch": lambda eng, d, n: list(eng.g1_double(d.g1[:n], d.fa[:n])),
    "sylow_hip_g1_normalize_batch": lambda eng, d, n: list(eng.g1_normalize(d.p1[:n])),
    "sylow_hip_g2_add_batch": lambda eng, d, n: list(eng.g2_add(d.g2[:n], d.g2[:n][::-1], d.fa[:n], d.fa[:n])),
    "sylow_hip_g2_normalize_batch": lambda eng, d, n: list(eng.g2_normalize(d.p2[:n])),
    "sylow_hip_g1_sum_batch": lambda eng, d, n: list(eng.g1_sum(d.g1[:n], d.fa[:n])),
    "sylow_hip_g2_sum_batch": lambda eng, d, n: list(eng.g2_sum(d.g2[:n], d.fa[:n])),
    "sylow_hip_g2_subgroup_check_batch": lambda eng, d, n: [eng.g2_subgroup_check(d.g2_mixed[:n], d.fa[:n])],
    "sylow_hip_evm_ecadd_batch": lambda eng, d, n: _raw_fixed(eng, "sylow_hip_evm_ecadd_batch", d.evm_add, n),
    "sylow_hip_g1_from_be_bytes_batch": lambda eng, d, n: list(eng.g1_from_be_bytes(d.g1_be[:n])),
    "sylow_hip_g2_from_be_bytes_batch": lambda eng, d, n: list(eng.g2_from_be_bytes(d.g2_be[:n])),
}
FIELDS = {
    **{"sylow_hip_%s_%s_batch" % (f, op): (lambda nm: lambda eng, d, n: [eng._binop(nm, 4, d.fp_a[:n], d.fp_b[:n])])("sylow_hip_%s_%s_batch" % (f, op))
       for f in ("fp", "fr") for op in ("add", "sub", "mul")},
    **{"sylow_hip_%s_%s_batch" % (f, op): (lambda nm: lambda eng, d, n: [eng._unop(nm, 4, d.fp_a[:n])])("sylow_hip_%s_%s_batch" % (f, op))
       for f in ("fp", "fr") for op in ("sqr", "neg", "inv")},          # fp_inv: two elements per thread; rows 0 of fp_a is 0
    "sylow_hip_fr_batch_inv": lambda eng, d, n: [eng.fr_batch_inv(d.fp_a[:n])],
    "sylow_hip_fp_pow_batch": lambda eng, d, n: [eng.fp_pow(d.fp_a[:n], d.e[:n])],
    "sylow_hip_fp_sqrt_batch": lambda eng, d, n: list(eng.fp_sqrt(d.sq[:n])),
    "sylow_hip_fp_is_square_batch": lambda eng, d, n: [eng.fp_is_square(d.sq[::-1][:n])],     # n = 1: a non-square or a square by the draw; both occur from n = 2
    "sylow_hip_fp_compute_naf_batch": lambda eng, d, n: list(eng.fp_compute_naf(d.e[::-1][:n])),
    "sylow_hip_fext_add_batch": _fext("add"), "sylow_hip_fext_sub_batch": _fext("sub"), "sylow_hip_fext_neg_batch": _fext("neg"),
    "sylow_hip_fext_scale_batch": _fext("scale"),
    "sylow_hip_fp2_mul_batch": lambda eng, d, n: [eng.fp2_mul(d.tower[8][:n], d.tower[8][:n][::-1])],
    "sylow_hip_fp2_inv_batch": lambda eng, d, n: [eng.fp2_inv(d.tower[8][:n])],
    "sylow_hip_fp6_mul_batch": lambda eng, d, n: [eng.fp6_mul(d.tower[24][:n], d.tower[24][:n][::-1])],
    "sylow_hip_fp12_mul_batch": lambda eng, d, n: [eng.fp12_mul(d.tower[48][:n], d.tower[48][:n][::-1])],
    "sylow_hip_fp_to_be_bytes_batch": lambda eng, d, n: [np.frombuffer(b"".join(eng.fp_to_be_bytes(d.fp_a[:n])), dtype=np.uint8)],
    "sylow_hip_fr_to_be_bytes_batch": lambda eng, d, n: [np.frombuffer(b"".join(eng.fr_to_be_bytes(d.fp_a[:n])), dtype=np.uint8)],
    "sylow_hip_fp_from_be_bytes_batch": lambda eng, d, n: list(eng.fp_from_be_bytes(d.blobs[:n])),
    "sylow_hip_fr_from_be_bytes_batch": lambda eng, d, n: list(eng.fr_from_be_bytes(d.blobs[:n])),
    "sylow_hip_aos_to_soa": lambda eng, d, n: _transpose(eng, "sylow_hip_aos_to_soa", d.tower[24][:n]),
    "sylow_hip_soa_to_aos": lambda eng, d, n: _transpose(eng, "sylow_hip_soa_to_aos", d.tower[24][:n]),
    "sylow_hip_f29_hook_batch": lambda eng, d, n: [eng.f29_hook(1, d.fp_a[:n], d.fp_b[:n])],
    "sylow_hip_f29_raw_hook_batch": lambda eng, d, n: [eng.f29_raw(0, _f29_limbs(n, 1)), eng.f29_raw(2, _f29_limbs(n, 2), _f29_limbs(n, 3)),
                                                       eng.f29_raw(6, *[_f29_limbs(n, s) for s in (4, 5, 6, 7)]),      # dot2: four operands
                                                       eng.f29_raw(13, *[_f29_limbs(n, s) for s in (4, 5, 6, 7)], k0=1, k1=1)],      # out [18][n]
    "sylow_hip_fp12_hook_batch": lambda eng, d, n: [eng.fp12_hook(16, d.tower[48][:n], d.tower[48][:n][::-1]), eng.fp12_hook(17, d.tower[48][:n])],
    "sylow_hip_hash_to_field_batch": lambda eng, d, n: [eng.hash_to_field(d.msgs[:n])],
    "sylow_hip_hash_to_field_expander_batch": lambda eng, d, n: [eng.hash_to_field(d.msgs[:n], dst=b"MEMORY-CONTRACT", expander="xmd_sha256")],
    "sylow_hip_expand_message_batch": lambda eng, d, n: [eng.expand_message(d.msgs[:n], 77, expander="xmd_keccak256", dst=b"MEMORY-CONTRACT")],
    "sylow_hip_flags_all": _flags_reduce, "sylow_hip_all_valid": _flags_reduce,
    # n polynomials of 5 coefficients / of 8 values
    "sylow_hip_kzg_quotient_batch": lambda eng, d, n: list(eng.kzg_quotient(d.polys[:n, :5], d.fp_b[:n])),
    "sylow_hip_kzg_quotient_evals_batch": lambda eng, d, n: list(eng.kzg_quotient_evals(d.polys[:n], d.fp_b[:n])),
    "sylow_hip_groth16_quotient_batch": lambda eng, d, n: [eng.groth16_quotient(d.polys[:n], d.polys[:n][::-1], d.polys[:n] if n % 2 else d.polys[1:n + 1])],
    "sylow_hip_fr_lincomb_batch": lambda eng, d, n: [eng.fr_lincomb(d.polys[:n, :5], d.fp_b[:n], _groups(n))],
    "sylow_hip_fr_group_powers_batch": lambda eng, d, n: [eng.fr_group_powers(d.fp_a[5:5 + len(_groups(n)) - 1], _groups(n), n)],
    "sylow_hip_fr_spmv_batch": lambda eng, d, n: _spmv(eng, d, n),
    "sylow_hip_fr_spmv_batch_tuned": lambda eng, d, n: _spmv(eng, d, n, lanes_log=2),
}
STATUS = {
    "sylow_hip_kzg_verify_batch": lambda eng, d, n: [eng.kzg_verify(d.kzg.tau_g2, *_kzg_args(d.kzg, n), c_inf=d.fb[:n], pi_inf=_flag_rows(n, 17, 0))],
    "sylow_hip_groth16_verify_batch": _g16_verify,
    "sylow_hip_g1_msm": lambda eng, d, n: list(eng.g1_msm(d.g1[:n], d.k[:n], p_inf=d.fa[:n])),
    "sylow_hip_g1_msm_tuned": lambda eng, d, n: list(eng.g1_msm(d.g1[:n], d.k[:n], p_inf=d.fa[:n], window=6, min_n=0)),
}
JOBS = {
    "sylow_hip_multi_pairing_batch": _multi_pairing,
    "sylow_hip_g1_lincomb_batch": _lincomb,
    "sylow_hip_evm_ecpairing_batch": _evm_pairing,
}
DRIVERS = {**PAIRING, **VERIFY, **WIDE, **GROUPS, **FIELDS, **STATUS, **JOBS}

PAIR_ROUTES = {
    "default": {},
    "two_per_wavefront_off": {"WIDE_PACK": 0},
    "two_per_wavefront_on": {"WIDE_PACK": 1},
    "quads": {"QUAD_MAX": 1 << 20, "WIDE_TAIL": 0},
    "lane_pairs": {"QUAD_MAX": 0, "WIDE_TAIL": 0},
}
WIDE_ROUTES = {"eight_lanes": {}, "one_lane": {"SIGN_WIDE_MAX": 0}}


def ragged(guarded, engine, data, name, route, opts):
    with options(engine, **opts):
        for n in SIZES:
            three_runs(guarded, engine, lambda eng: DRIVERS[name](eng, data, n), f"{name} at n = {n} on route {route}")


@pytest.mark.parametrize("route", sorted(PAIR_ROUTES))
@pytest.mark.parametrize("name", sorted(PAIRING))
def test_ragged_pairing(guarded, engine, data, name, route):
    ragged(guarded, engine, data, name, route, PAIR_ROUTES[route])


@pytest.mark.parametrize("route", sorted(PAIR_ROUTES))
@pytest.mark.parametrize("name", sorted(VERIFY))
def test_ragged_bls_verify(guarded, engine, data, name, route):
    ragged(guarded, engine, data, name, route, PAIR_ROUTES[route])


@pytest.mark.parametrize("route", sorted(WIDE_ROUTES))
@pytest.mark.parametrize("name", sorted(WIDE))
def test_ragged_wide_and_one_lane(guarded, engine, data, name, route):
    ragged(guarded, engine, data, name, route, WIDE_ROUTES[route])


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_ragged_group_ops(guarded, engine, data, name):
    ragged(guarded, engine, data, name, "default", {})


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_ragged_fields(guarded, engine, data, name):
    ragged(guarded, engine, data, name, "default", {})


@pytest.mark.parametrize("name", sorted(STATUS))
def test_ragged_status_only_outputs(guarded, engine, data, name):
    ragged(guarded, engine, data, name, "default", {})


@pytest.mark.parametrize("name", sorted(JOBS))
def test_ragged_jobs(guarded, engine, data, name):
    ragged(guarded, engine, data, name, "default", {})              # n rows; the last job always holds one pair / one term row


@pytest.mark.parametrize("tuned", [False, True])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("log_n", [0, 1, 3])
def test_ragged_fr_ntt(guarded, engine, data, log_n, m, tuned):
    vals = data.polys[:m, :1 << log_n]
    for inverse, shift in ((False, None), (True, None), (False, data.fp_b[7])):
        three_runs(guarded, engine, lambda eng: [eng.fr_ntt(vals, inverse=inverse, shift=shift, stages=1 if tuned else -1)],
                   f"fr_ntt log_n = {log_n}, m = {m}, inverse = {inverse}, shift = {shift is not None}")


def test_both_output_values_occur(engine, data):
    """the batches hold identity rows and invalid rows: flags and statuses take the zero and the non-zero value"""
    n = NMAX
    for name in ("sylow_hip_bls_verify_batch", "sylow_hip_bls_verify_same_signer_batch", "sylow_hip_kzg_verify_batch", "sylow_hip_groth16_verify_batch",
                 "sylow_hip_g2_subgroup_check_batch", "sylow_hip_fp_is_square_batch"):
        flags = np.asarray(DRIVERS[name](engine, data, n)[-1])
        assert flags.any() and not flags.all(), name
    for name in ("sylow_hip_g1_scalar_mul_batch", "sylow_hip_bls_sign_batch", "sylow_hip_g2_scalar_mul_batch", "sylow_hip_g1_add_batch",
                 "sylow_hip_g1_normalize_batch", "sylow_hip_evm_ecmul_batch", "sylow_hip_evm_ecadd_batch", "sylow_hip_fp_from_be_bytes_batch",
                 "sylow_hip_g1_from_be_bytes_batch"):
        flags = np.asarray(DRIVERS[name](engine, data, n)[-1])
        assert flags.any() and not flags.all(), name
    res, st = DRIVERS["sylow_hip_evm_ecpairing_batch"](engine, data, NMAX)
    assert st.any() and not st.all() and res.any(), "ecPairing jobs: valid, invalid, and products that are one"


# ================================================================ e. the host-array entry points =====================================
class HostArrays:
    """numpy views into padded host arrays: guard + body + guard, the whole allocation filled first"""

    def __init__(self, fill):
        self.fill, self.items = fill, []

    def place(self, name, param, arr=None, shape=None, dtype=None, const=True):
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            shape, dtype = arr.shape, arr.dtype
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        raw = np.full(nbytes + 2 * GUARD, self.fill, dtype=np.uint8)
        view = raw[GUARD:GUARD + nbytes].view(dtype).reshape(shape)
        if arr is not None:
            view[...] = arr
        self.items.append((name, param, raw, raw.copy(), nbytes, const))
        return view

    def audit(self):
        for name, param, raw, before, nbytes, const in self.items:
            audit_bytes(name, param, before, raw, self.fill, nbytes, const, None)
            HOST_AUDITED.add((name, param))


def _blob(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8), off


def _host_runs(engine, call, plain, what):
    """call(HostArrays) -> list of output views, under both fills; plain() -> the same through the unpadded Python layer"""
    outs = []
    for fill in FILLS:
        h = HostArrays(fill)
        out = call(h)
        h.audit()
        outs.append([np.array(o) for o in out])
    same(outs[0], outs[1], f"{what}: fill 0x{FILLS[0]:02X} against 0x{FILLS[1]:02X}: {LEAK}")
    same(outs[0], plain(), f"{what}: padded host arrays against the plain call")


def _tiled(a, n):
    return T._tile(np.asarray(a), n, 1)


@pytest.mark.parametrize("n,chunk", [(37, 5), (37, 100), (1037, 5), (1037, 100)])
def test_pairing_host_stays_inside_host_arrays(engine, data, n, chunk):
    nm = "sylow_hip_pairing_host"
    p, q, fa, fb = _tiled(data.g1, n), _tiled(data.g2, n), _tiled(data.fa, n), _tiled(data.fb, n)

    def call(h):
        hp, hpi, hq, hqi = h.place(nm, "p_aos", p), h.place(nm, "p_inf", fa), h.place(nm, "q_aos", q), h.place(nm, "q_inf", fb)
        gt = h.place(nm, "gt_aos", shape=(n, 48), dtype=np.uint64, const=False)
        assert engine.lib.sylow_hip_pairing_host(hp.ctypes.data, hpi.ctypes.data, hq.ctypes.data, hqi.ctypes.data, gt.ctypes.data, n, chunk) == 0
        return [gt]
    _host_runs(engine, call, lambda: [engine.pairing(p, q, fa, fb, chunk=chunk)], f"{nm} n = {n}, chunk = {chunk}")


@pytest.mark.parametrize("n,chunk", [(37, 5), (37, 100), (1037, 5), (1037, 100)])
def test_bls_verify_host_stays_inside_host_arrays(engine, data, n, chunk):
    nm = "sylow_hip_bls_verify_host"
    pk, sig, fa, fb = _tiled(data.pk, n), _tiled(data.sig, n), _tiled(data.fa, n), _tiled(data.fb, n)
    msgs = [data.vmsgs[i % NMAX] for i in range(n)]
    blob, off = _blob(msgs)

    def call(h):
        hk, hki, hm, ho = h.place(nm, "pk_aos", pk), h.place(nm, "pk_inf", fa), h.place(nm, "msgs", blob), h.place(nm, "msg_offsets", off)
        hs, hsi = h.place(nm, "sig_aos", sig), h.place(nm, "sig_inf", fb)
        ok = h.place(nm, "ok", shape=(n,), dtype=np.uint8, const=False)
        assert engine.lib.sylow_hip_bls_verify_host(hk.ctypes.data, hki.ctypes.data, hm.ctypes.data, ho.ctypes.data, hs.ctypes.data, hsi.ctypes.data,
                                                    ok.ctypes.data, n, chunk) == 0
        return [ok]
    _host_runs(engine, call, lambda: [engine.bls_verify(pk, msgs, sig, fa, fb, chunk=chunk)], f"{nm} n = {n}, chunk = {chunk}")


@pytest.mark.parametrize("n,chunk", [(37, 5), (37, 100), (1037, 5), (1037, 100)])
def test_pairing_host_bytes_stays_inside_host_arrays(engine, data, n, chunk):
    nm = "sylow_hip_pairing_host_bytes"
    pb, qb = [data.g1_be[i % NMAX] for i in range(n)], [data.g2_be[i % NMAX] for i in range(n)]

    def call(h):
        hp = h.place(nm, "p_be", np.frombuffer(b"".join(pb), dtype=np.uint8))
        hq = h.place(nm, "q_be", np.frombuffer(b"".join(qb), dtype=np.uint8))
        gt = h.place(nm, "gt_aos", shape=(n, 48), dtype=np.uint64, const=False)
        sp, sq = h.place(nm, "status_p", shape=(n,), dtype=np.uint8, const=False), h.place(nm, "status_q", shape=(n,), dtype=np.uint8, const=False)
        assert engine.lib.sylow_hip_pairing_host_bytes(hp.ctypes.data, hq.ctypes.data, gt.ctypes.data, sp.ctypes.data, sq.ctypes.data, n, chunk) == 0
        assert sp.any() and not sp.all() and sq.any() and not sq.all()
        return [gt, sp, sq]
    _host_runs(engine, call, lambda: list(engine.pairing_from_bytes(pb, qb, chunk=chunk)), f"{nm} n = {n}, chunk = {chunk}")


@pytest.mark.parametrize("n,chunk", [(37, 5), (37, 100), (1037, 5), (1037, 100)])
def test_bls_verify_host_bytes_stays_inside_host_arrays(engine, data, n, chunk):
    nm = "sylow_hip_bls_verify_host_bytes"
    if "wire" not in data.__dict__:
        pk_be, sig_be = engine.g2_to_be_bytes(data.pk), engine.g1_to_be_bytes(data.sig)
        for i in range(4, NMAX - 1, 7):
            pk_be[i], sig_be[i + 1] = data.g2_be[1], data.g1_be[1]   # rows that decode to nothing
        data.wire = (pk_be, sig_be)
    kb, sb = [data.wire[0][i % NMAX] for i in range(n)], [data.wire[1][i % NMAX] for i in range(n)]
    msgs = [data.vmsgs[i % NMAX] for i in range(n)]
    blob, off = _blob(msgs)

    def call(h):
        hk, hm, ho = h.place(nm, "pk_be", np.frombuffer(b"".join(kb), dtype=np.uint8)), h.place(nm, "msgs", blob), h.place(nm, "msg_offsets", off)
        hs = h.place(nm, "sig_be", np.frombuffer(b"".join(sb), dtype=np.uint8))
        ok, sk, ss = (h.place(nm, p, shape=(n,), dtype=np.uint8, const=False) for p in ("ok", "status_pk", "status_sig"))
        assert engine.lib.sylow_hip_bls_verify_host_bytes(hk.ctypes.data, hm.ctypes.data, ho.ctypes.data, hs.ctypes.data, ok.ctypes.data,
                                                          sk.ctypes.data, ss.ctypes.data, n, chunk) == 0
        assert ok.any() and not ok.all() and sk.any() and ss.any()
        return [ok, sk, ss]
    _host_runs(engine, call, lambda: list(engine.bls_verify_from_bytes(kb, msgs, sb, chunk=chunk)), f"{nm} n = {n}, chunk = {chunk}")


@pytest.mark.parametrize("n,stride", [(1, 1), (37, 37), (37, 50)])
def test_host_xoshiro_fp_stays_inside_its_array(engine, n, stride):
    nm = "sylow_hip_host_xoshiro_fp"
    words = 3 * stride + n

    def call(h):
        out = h.place(nm, "out_host", shape=(words,), dtype=np.uint64, const=False)
        assert engine.lib.sylow_hip_host_xoshiro_fp(SEED, out.ctypes.data, n, stride) == 0
        return [np.array([out[w * stride:w * stride + n] for w in range(4)])]        # the gaps of a stride > n are not the call's to write
    _host_runs(engine, call, lambda: [engine.xoshiro_fp_soa(SEED, n)], f"{nm} n = {n}, stride = {stride}")


# ================================================================ coverage ============================================================
def test_every_shape_array_of_every_driven_entry_point_was_audited(guarded):
    from sylow_amd import _shapes
    from test_guarded_engine import MEMORY_CONTRACT, NOT_AUDITED
    audited = guarded.audited | HOST_AUDITED
    assert len(audited) > 100, (f"only {len(audited)} (entry point, array) pairs were audited in this process: this test sums up the whole file and "
                                "cannot pass on its own or in a subset of it")
    missing = []
    for name, row in sorted(MEMORY_CONTRACT.items()):
        if row.exempt:
            continue
        for param in _shapes.table().get(name, ((), {}))[1]:
            if (name, param) not in audited and param not in NOT_AUDITED and (name, param) not in NOT_AUDITED:
                missing.append((name, param))
    assert not missing, f"@shape arrays of driven entry points that no audited call passed: {missing}"
    print(f"memory contract: {len(audited)} (entry point, array) pairs audited, {time.time() - WALL['t0']:.1f} s for the file")
