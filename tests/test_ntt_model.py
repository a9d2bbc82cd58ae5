"""CPU tests of tests/ntt_model.py (the integer model the GPU tests of the Fr transform compare against) and of the binding's declarations:
the root, the definition against the radix-2 recursion, the kernel's pass decomposition against both, and n^-1 as the plan header forms it."""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ntt_model as M                                      # noqa: E402

R = M.R
NEW_SYMBOLS = ("sylow_hip_fr_ntt_batch", "sylow_hip_fr_ntt_batch_tuned", "sylow_hip_kzg_commit_evals_batch")


def rand(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1 << 256) for _ in range(n)]


def test_root_has_order_exactly_2_28():
    assert (R - 1) % (1 << 28) == 0 and ((R - 1) >> 28) % 2 == 1
    assert pow(M.W, 1 << 28, R) == 1 and pow(M.W, 1 << 27, R) == R - 1
    assert pow(5, (R - 1) // 2, R) == R - 1              # 5 is a non-residue
    assert M.omega(0) == 1 and M.omega(1) == R - 1 and M.omega(28) == M.W
    for log_n in range(1, 29):
        assert pow(M.omega(log_n), 1 << (log_n - 1), R) == R - 1


@pytest.mark.parametrize("log_n", range(7))
def test_direct_equals_radix2(log_n):
    a = rand(1 << log_n, 10 + log_n)
    for inverse in (False, True):
        for shift in (None, 5, (1 << 256) - 1):
            assert M.ntt_direct(a, log_n, inverse, shift) == M.ntt_radix2(a, log_n, inverse, shift), (inverse, shift)
    assert M.ntt_radix2(M.ntt_radix2(a, log_n, False, 7), log_n, True, 7) == [v % R for v in a]


@pytest.mark.parametrize("log_n", range(13))
def test_passes_equal_radix2(log_n):
    a = rand(1 << log_n, 40 + log_n)
    want = M.ntt_radix2(a, log_n)
    want_inv = M.ntt_radix2(a, log_n, True)
    for stages in range(1, 7):
        assert M.ntt_passes(a, log_n, stages) == want, stages
        assert M.ntt_passes(a, log_n, stages, inverse=True) == want_inv, stages
    if log_n <= 8:
        for stages in (1, 3, 10):
            for shift in (3, R, R + 1):
                assert M.ntt_passes(a, log_n, stages, False, shift) == M.ntt_radix2(a, log_n, False, shift)
                assert M.ntt_passes(a, log_n, stages, True, shift) == M.ntt_radix2(a, log_n, True, shift)


def test_passes_ping_pong_ends_in_out():
    for log_n, stages, inverse, shift, want in ((0, 4, False, None, ["out"]), (4, 4, False, None, ["out"]), (5, 4, False, None, ["buf", "out"]),
                                                (9, 4, False, None, ["out", "buf", "out"]), (4, 4, True, None, ["buf", "out"]),
                                                (5, 4, False, 3, ["out", "buf", "out"]), (5, 4, True, 3, ["out", "buf", "out"])):
        trace = []
        M.ntt_passes([1] * (1 << log_n), log_n, stages, inverse, shift, trace)
        assert trace == want, (log_n, stages, inverse, shift)
    assert M.pass_plan(9, 4) == [(4, 0), (4, 4), (1, 8)] and M.pass_plan(0, 4) == []


def test_n_inverse_as_the_header_forms_it():
    for log_n in range(29):
        assert M.n_inverse(log_n) == pow(1 << log_n, -1, R)


def test_plan_constants_are_read():
    c = M.plan_constants()
    assert c["NTT_LOG_N_MAX"] == 28 and 1 <= c["NTT_STAGES_DEFAULT"] <= c["NTT_STAGES_MAX"] == c["NTT_TILE_LOG"]
    assert c["NTT_BLOCK"] == 256 and c["NTT_GRID_CAP"] == 1 << 20


def test_new_symbols_are_declared_everywhere():
    from sylow_amd import _lib, _shapes
    header = open(os.path.join(ROOT, "include", "sylow_hip.h")).read()
    table = _shapes.parse()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"int32_t\s+" + name + r"\s*\(", header), name
        assert name in table, name
    assert len(_lib.SIGNATURES["sylow_hip_fr_ntt_batch_tuned"]) == len(_lib.SIGNATURES["sylow_hip_fr_ntt_batch"]) + 1
    # the shapes in bytes: m arrays of 2^log_n elements of 32 bytes
    names, shapes = table["sylow_hip_fr_ntt_batch"]
    assert shapes["in"].nbytes({"log_n": 5, "m": 3}) == 32 * 32 * 3 == shapes["out"].nbytes({"log_n": 5, "m": 3})
    assert shapes["shift"].optional and shapes["shift"].nbytes({}) == 32
