"""CPU: the integer model of the KZG prover (tests/kzg_prove_model.py) -- the quotient identity, the kernel's decomposition against the plain
recurrence at the real lane and block sizes, and the four new entry points at the boundary: declared, exported, bound and annotated."""
import os
import random

import pytest

import kzg_prove_model as M
from kzg_prove_model import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sylow_hip_kzg_quotient_batch", "sylow_hip_kzg_commit_batch", "sylow_hip_kzg_commit_batch_tuned", "sylow_hip_kzg_open_batch"]


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def test_quotient_satisfies_the_division_identity():
    rng = random.Random(0x51)
    for n in (1, 2, 3, 17, 300):
        for z in (0, 1, R - 1, rng.randrange(R)):
            f = rand_poly(rng, n)
            q, y = M.quotient(f, z)
            assert len(q) == n and q[n - 1] == 0 and y == M.evaluate(f, z)
            for _ in range(3):
                x = rng.randrange(R)
                assert (M.evaluate(f, x) - y) % R == (x - z) * M.evaluate(q, x) % R


def test_quotient_takes_scalars_mod_r():
    rng = random.Random(0x52)
    f = rand_poly(rng, 9)
    z = rng.randrange(R)
    wide = [c + R * (i % 5) for i, c in enumerate(f)]
    assert all(w <= M.TOP for w in wide)
    q0, y0 = M.quotient(f, z)
    assert M.quotient(wide, z + R) == ([v % R for v in q0], y0) and M.chunked_quotient(wide, z + 2 * R, 4, 8) == (q0, y0)


def test_chunked_quotient_is_the_recurrence_at_the_kernels_sizes():
    k = M.plan_constants()
    L, B, CH = k["KZG_POLY_LANE_COEFFS"], k["KZG_POLY_BLOCK"], k["KZG_POLY_CHUNK"]
    rng = random.Random(0x53)
    for n in (1, 2, L - 1, L, L + 1, CH - 1, CH, CH + 1, 2 * CH + 1):
        f = rand_poly(rng, n)
        for z in (0, 1, R - 1, rng.randrange(R)):
            assert M.chunked_quotient(f, z, L, B) == M.quotient(f, z), (n, z)


def test_chunked_quotient_is_the_recurrence_at_small_sizes():
    """L = 4, B = 8: chunks of 32, so len = 1 .. 200 crosses every lane, chunk and tail boundary; 257 .. 300 also crosses the carry level's
    tile of 8 chunks"""
    rng = random.Random(0x54)
    for n in list(range(1, 201)) + [256, 257, 258, 289, 300]:
        f = rand_poly(rng, n)
        z = (0, 1, R - 1, rng.randrange(R))[n % 4]
        assert M.chunked_quotient(f, z, 4, 8) == M.quotient(f, z), n


def test_entry_points_are_declared_exported_and_bound():
    import __graft_entry__
    import sylow_amd
    from sylow_amd import _lib
    declared = __graft_entry__.declared_symbols()
    lib = sylow_amd.load()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_shape_lines_parse_and_check_sizes():
    from sylow_amd import _shapes
    table = _shapes.parse()
    for name in NAMES:
        assert name in table, name
    names, shapes = table["sylow_hip_kzg_quotient_batch"]
    assert names[:6] == ["coeffs", "len", "m", "z", "q_out", "y_out"]
    assert shapes["q_out"].optional and shapes["y_out"].optional and not shapes["coeffs"].optional
    assert shapes["coeffs"].nbytes({"len": 5, "m": 3}) == 4 * 5 * 3 * 8 and shapes["y_out"].nbytes({"len": 5, "m": 3}) == 96
    for name in NAMES[1:]:
        assert not any(sh.optional for sh in table[name][1].values()), name
        assert table[name][1]["srs_g1_xy"].nbytes({"len": 7, "m": 2}) == 8 * 7 * 8
    # check_call: (name, args without the stream, {base pointer: bytes})
    live = {0x1000: 4 * 5 * 3 * 8, 0x2000: 4 * 3 * 8, 0x3000: 4 * 5 * 3 * 8, 0x4000: 4 * 3 * 8}
    _shapes.check_call("sylow_hip_kzg_quotient_batch", (0x1000, 5, 3, 0x2000, 0x3000, 0x4000), live)
    _shapes.check_call("sylow_hip_kzg_quotient_batch", (0x1000, 5, 3, 0x2000, None, 0x4000), live)
    with pytest.raises(ValueError, match="q_out holds"):
        _shapes.check_call("sylow_hip_kzg_quotient_batch", (0x1000, 6, 3, 0x2000, 0x3000, 0x4000), {**live, 0x1000: 1 << 20})
    with pytest.raises(ValueError, match="z must not be NULL"):
        _shapes.check_call("sylow_hip_kzg_quotient_batch", (0x1000, 5, 3, None, 0x3000, 0x4000), live)
    live = {0x1000: 8 * 5 * 8, 0x2000: 4 * 5 * 3 * 8, 0x3000: 8 * 3 * 8, 0x4000: 3}
    _shapes.check_call("sylow_hip_kzg_commit_batch", (0x1000, 0x2000, 5, 3, 0x3000, 0x4000), live)
    _shapes.check_call("sylow_hip_kzg_commit_batch_tuned", (0x1000, 0x2000, 5, 3, 8, 0, 0x3000, 0x4000), live)
    with pytest.raises(ValueError, match="out_inf holds"):
        _shapes.check_call("sylow_hip_kzg_commit_batch", (0x1000, 0x2000, 5, 4, 0x3000, 0x4000), {**live, 0x2000: 1 << 20, 0x3000: 1 << 20})
    with pytest.raises(ValueError, match="srs_g1_xy holds"):
        _shapes.check_call("sylow_hip_kzg_open_batch", (0x1000, 0x2000, 6, 3, 0x3000, 0x3000, 0x3000, 0x4000), {**live, 0x2000: 1 << 20, 0x3000: 1 << 20})
