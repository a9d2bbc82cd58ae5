"""GPU: every argument error of sylow_hip_g1_ntt_batch, its _tuned form and sylow_hip_kzg_srs_lagrange -- SYLOW_HIP_E_ARG, no launch, nothing
written (sentinel-filled outputs stay as they were) -- m = 0 with NULL pointers, adjacent halves of one allocation accepted, and the Python
layer's refusal of a short buffer before the launch.  And the input contract of tests/test_gpu_input_contract.py for the three: the
coordinate words are Fp values (representatives x + k p give the same outputs), p_inf = NULL is an all-zero flag array.  The rows and the
cases are registered in that file's tables when the suite is collected, so its CPU completeness tests see them."""
import numpy as np
import pytest

import g1_ntt_model as M
import test_gpu_input_contract as T

E_ARG = -2
SENTINEL = 0x5A5A5A5A5A5A5A5A
LOG_N = 4
ROWS = {
    "sylow_hip_g1_ntt_batch": T.Row({"p_xy": T.G1A}, ["p_inf"]),
    "sylow_hip_g1_ntt_batch_tuned": T.Row({"p_xy": T.G1A}, ["p_inf"]),
    "sylow_hip_kzg_srs_lagrange": T.Row({"srs_g1_xy": T.G1A}),
}
T.CONTRACT.update(ROWS)
_DATA = []


def data():
    """two arrays of 16 points, a zero logarithm in each (it comes from the oracle as (0, 1) + its flag), and the monomial SRS of a tau"""
    if not _DATA:
        rng = T.Xoshiro(T.SEED + 0x61)
        logs = [rng.u256() % M.R for _ in range(2 << LOG_N)]
        logs[3] = logs[20] = 0
        xy, inf = M.points(logs)
        srs, sinf = M.points(M.monomial_logs(0xC0FFEE0DDBA11, 1 << LOG_N))
        assert list(np.flatnonzero(inf)) == [3, 20] and not sinf.any()
        _DATA.append((xy.reshape(2, 1 << LOG_N, 8), inf.reshape(2, 1 << LOG_N), srs))
    return _DATA[0]


@T.case("g1_ntt_batch", "g1_ntt_batch_tuned")
def _g1_ntt(eng, c, pool, nm):
    xy, inf, _ = data()
    words = c.fp("p_xy", xy.reshape(-1, 8)).reshape(xy.shape)
    flags = c.flag("p_inf", inf.reshape(-1))
    flags = None if flags is None else flags.reshape(inf.shape)
    tuned = nm.endswith("_tuned")
    return list(eng.g1_ntt(words, flags, inverse=tuned, max_blocks=1 if tuned else -1))


@T.case("kzg_srs_lagrange")
def _srs(eng, c, pool, nm):
    return list(eng.kzg_srs_lagrange(c.fp("srs_g1_xy", data()[2])))


def test_rows_name_real_parameters():
    from sylow_amd import _shapes
    from test_rust_ffi import parse_header
    protos, shapes = parse_header(), _shapes.parse()
    for name, row in ROWS.items():
        assert name in protos and T.CONTRACT[name] is row and name in T.CASES
        assert set(row.fp) | set(row.flags) <= {p[3] for p in protos[name][1]}, name
        assert {p for p, sh in shapes[name][1].items() if sh.optional} == set(row.flags), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_reduces_representatives_and_null_flags(engine, name):
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"
    assert not np.asarray(base[1]).any()            # a zero logarithm among random ones transforms to no identity


@pytest.mark.gpu
def test_argument_errors_write_nothing_and_empty_batch(engine):
    lib = engine.lib
    n, log_n = 8, 3
    pxy, pinf = M.points(list(range(1, 2 * n + 1)))
    two = np.ascontiguousarray(pxy.reshape(2, n, 8).transpose(0, 2, 1))        # [2][8][n]: two arrays' worth, the halves adjacent
    fill = np.full((2, 8, n), SENTINEL, dtype=np.uint64)
    din, dinf = engine.to_device(two), engine.to_device(np.zeros((2, n), dtype=np.uint8))
    dout, doi = engine.to_device(fill), engine.to_device(np.full((2, n), 7, np.uint8))
    plain = lambda *a: lib.sylow_hip_g1_ntt_batch(*a, engine.stream)
    tuned = lambda *a: lib.sylow_hip_g1_ntt_batch_tuned(*a, engine.stream)
    srs = lambda *a: lib.sylow_hip_kzg_srs_lagrange(*a, engine.stream)
    assert plain(None, dinf.ptr, log_n, 1, 0, dout.ptr, doi.ptr) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    assert plain(din.ptr, dinf.ptr, log_n, 1, 0, None, doi.ptr) == E_ARG and plain(din.ptr, dinf.ptr, log_n, 1, 0, dout.ptr, None) == E_ARG
    assert plain(din.ptr, None, -1, 1, 0, dout.ptr, doi.ptr) == E_ARG and plain(din.ptr, None, 29, 1, 0, dout.ptr, doi.ptr) == E_ARG
    assert plain(din.ptr, None, 29, 0, 0, dout.ptr, doi.ptr) == E_ARG        # log_n is checked before m = 0 returns
    assert plain(din.ptr, None, log_n, 1, 2, dout.ptr, doi.ptr) == E_ARG and plain(din.ptr, None, log_n, 1, -1, dout.ptr, doi.ptr) == E_ARG
    assert tuned(din.ptr, None, log_n, 1, 0, 0, dout.ptr, doi.ptr) == E_ARG  # max_blocks == 0
    size = 64 * n
    for off in (0, 64, size - 8, -(size - 8)):                               # out_xy inside p_xy's byte range, from either side
        base = dout.ptr + size if off < 0 else dout.ptr
        assert plain(base, None, log_n, 1, 0, base + off, doi.ptr) == E_ARG, off
        assert tuned(base, None, log_n, 1, 1, 1, base + off, doi.ptr) == E_ARG, off
    assert plain(dout.ptr, None, log_n, 2, 0, dout.ptr + size, doi.ptr) == E_ARG      # two arrays: the second half is inside the range
    for off in (0, 1, n - 1, -(n - 1)):                                       # out_inf inside p_inf's byte range, from either side
        base = doi.ptr + n if off < 0 else doi.ptr
        assert plain(din.ptr, base, log_n, 1, 0, dout.ptr, base + off) == E_ARG, off
    assert srs(None, log_n, dout.ptr, doi.ptr) == E_ARG and srs(din.ptr, log_n, None, doi.ptr) == E_ARG and srs(din.ptr, log_n, dout.ptr, None) == E_ARG
    assert srs(din.ptr, -1, dout.ptr, doi.ptr) == E_ARG and srs(din.ptr, 29, dout.ptr, doi.ptr) == E_ARG and srs(dout.ptr, log_n, dout.ptr + 8, doi.ptr) == E_ARG
    # m = 0: OK, nothing launched, NULL pointers and all
    assert plain(din.ptr, None, log_n, 0, 0, dout.ptr, doi.ptr) == 0 and plain(None, None, log_n, 0, 1, None, None) == 0
    assert tuned(None, None, 0, 0, 0, 5, None, None) == 0
    engine.sync()
    assert np.array_equal(dout.download(), fill) and (doi.download() == 7).all() and np.array_equal(din.download(), two), "nothing written"
    # adjacent halves of one allocation do not overlap: the call runs, flags likewise
    dboth, fboth = engine.to_device(np.concatenate([two[:1], fill[:1]])), engine.to_device(np.concatenate([np.zeros(n, np.uint8), np.full(n, 7, np.uint8)]))
    assert plain(dboth.ptr, fboth.ptr, log_n, 1, 0, dboth.ptr + size, fboth.ptr + n) == 0
    engine.sync()
    got, flags = dboth.download(), fboth.download()
    wxy, winf = M.expected(list(range(1, n + 1)), log_n)
    assert np.array_equal(got[0], two[0]) and np.array_equal(np.ascontiguousarray(got[1].T), wxy)
    assert not flags[:n].any() and np.array_equal(flags[n:], winf)


@pytest.mark.gpu
def test_short_buffer_is_refused_before_the_launch(engine):
    import sylow_amd
    din, dout, doi = engine.empty((1, 8, 16)), engine.empty((1, 8, 8)), engine.empty((16,), np.uint8)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="out_xy holds"):
        engine._call("sylow_hip_g1_ntt_batch", din.ptr, None, 4, 1, 0, dout.ptr, doi.ptr)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="out_xy holds"):
        engine._call("sylow_hip_g1_ntt_batch_tuned", din.ptr, None, 4, 1, 0, 2, dout.ptr, doi.ptr)
    big, short = engine.empty((8, 16)), engine.empty((8,), np.uint8)
    with pytest.raises(sylow_amd._lib.SylowHipError, match="out_inf holds"):
        engine._call("sylow_hip_kzg_srs_lagrange", din.ptr, 4, big.ptr, short.ptr)
