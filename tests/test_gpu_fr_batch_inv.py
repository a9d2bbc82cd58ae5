"""GPU: sylow_hip_fr_batch_inv (kzg_evals.hip) -- the inverses of n elements of Fr that share ONE inversion per chunk -- against the integer
model of tests/kzg_evals_model.py and, at every size, word for word against sylow_hip_fr_inv_batch, the per-element power the library had
before (independent code: runtime.hip).  Sizes come from kzg_evals_plan.hpp: a lane's elements L, a chunk CH = 256 L.  The design has no
level above the chunk (every chunk pays its own inversion), so there is no tile to cross; 257 chunks run all the same, for the grid."""
import random

import numpy as np
import pytest

import kzg_evals_model as E
from groth16_model import ints, limbs
from kzg_evals_model import EDGE_WORDS, R

pytestmark = pytest.mark.gpu
E_ARG = -2
K = E.plan_constants()
L, BLOCK, CH = K["EVALS_LANE_ELEMS"], K["EVALS_BLOCK"], K["EVALS_CHUNK"]
SENTINEL = 0x5A5A5A5A5A5A5A5A
SIZES = [1, L - 1, L, L + 1, CH - 1, CH, CH + 1, 3 * CH + L + 1]
ONE = limbs([1]).reshape(4)


def rand_words(rng, n):
    """any 256-bit words"""
    return np.frombuffer(rng.randbytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()


def check(engine, a, model=True):
    """a [n, 4] words: the call against fr_inv_batch, against a * out = [a != 0], and (model) against pow"""
    out = engine.fr_batch_inv(a)
    assert np.array_equal(out, engine.fr_inv(a)), f"{int((out != engine.fr_inv(a)).any(axis=1).sum())} of {len(a)} elements differ from fr_inv_batch"
    prod = engine.fr_mul(a, out)
    nonzero = np.array([v % R != 0 for v in ints(a)]) if len(a) <= 4 * CH else None
    if nonzero is not None:
        assert np.array_equal(prod[nonzero], np.tile(ONE, (int(nonzero.sum()), 1))) and not prod[~nonzero].any(), "a * out is 1 exactly where a != 0"
        assert not out[~nonzero].any(), "inv(0) = 0"
    else:                                                       # large arrays: every product is 0 or 1, and 0 only where out is
        is_one, is_zero = (prod == ONE).all(axis=1), ~prod.any(axis=1)
        assert (is_one | is_zero).all() and np.array_equal(is_zero, ~out.any(axis=1))
    if model:
        assert np.array_equal(out, limbs(E.batch_inv(ints(a)))), "the model"
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_against_the_model_and_fr_inv_batch(engine, n):
    rng = random.Random(0xD0 + n)
    out = check(engine, rand_words(rng, n))
    assert all(v < R for v in ints(out[: 2 * L]))              # canonical, whatever words came in


def test_257_chunks(engine):
    """More chunks than a block has lanes, the last of one element: the grid, not a tile -- this design has no level above the chunk."""
    rng = random.Random(0xD1)
    n = BLOCK * CH + 1
    a = rand_words(rng, n)
    a[[0, CH - 1, CH, n - 1, n // 2]] = limbs([0, R, 2 * R, 0, R])
    out = check(engine, a, model=False)
    at = [1, CH + 1, n - 2, 100 * CH + 77]
    assert np.array_equal(out[at], limbs([E.inv(v) for v in ints(a[at])]))


@pytest.mark.parametrize("at", ["first of the array", "last of lane 0", "first of lane 1", "last of chunk 0", "first of chunk 1", "last of a lane inside",
                                "last of the array"])
def test_a_lone_zero(engine, at):
    n = 3 * CH + L + 1
    k = {"first of the array": 0, "last of lane 0": L - 1, "first of lane 1": L, "last of chunk 0": CH - 1, "first of chunk 1": CH,
         "last of a lane inside": CH + 17 * L + L - 1, "last of the array": n - 1}[at]
    rng = random.Random(0xD2 + k)
    a = limbs([rng.randrange(1, R) for _ in range(n)])
    a[k] = limbs([R])[0] if k % 2 else 0                        # 0 written either way
    out = check(engine, a)
    assert not out[k].any() and out[np.arange(n) != k].any(axis=1).all()


def test_a_chunk_of_zeros_between_live_chunks_and_all_zeros(engine):
    rng = random.Random(0xD3)
    n = 3 * CH + L + 1
    a = limbs([rng.randrange(1, R) for _ in range(n)])
    a[CH:2 * CH] = limbs([0, R, 2 * R, 0] * (CH // 4))          # the chunk's product is the empty one: 1
    out = check(engine, a)
    assert not out[CH:2 * CH].any() and out[:CH].any(axis=1).all() and out[2 * CH:].any(axis=1).all()
    for n in (1, L + 1, CH + 3):
        zeros = limbs([[0, R, 2 * R][i % 3] for i in range(n)])
        assert not check(engine, zeros).any()


def test_edge_words(engine):
    rng = random.Random(0xD4)
    check(engine, limbs(EDGE_WORDS))
    for n in (L + 1, CH + 1):
        a = rand_words(rng, n)
        for i, w in enumerate(EDGE_WORDS):
            a[(i * 37) % n if i % 2 else n - 1 - (i * 11) % n] = limbs([w])[0]
        check(engine, a)


def test_api_batch_inv(engine):
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0xD5)
    vals = [rng.randrange(R) for _ in range(L + 3)] + [0]
    a = api.Fr.from_ints(vals)
    assert (a.batch_inv() == a.inv()).all() and ints(a.batch_inv().v) == [E.inv(v) for v in vals]


def test_argument_errors_overlap_and_empty(engine):
    lib = engine.lib
    n = 8
    fill = np.full((2, 4, n), SENTINEL, dtype=np.uint64)        # two arrays' worth: the halves are adjacent, not overlapping
    da, do = engine.to_device(fill), engine.to_device(fill)
    call = lambda *a: lib.sylow_hip_fr_batch_inv(*a, engine.stream)
    assert call(None, do.ptr, n) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    assert call(da.ptr, None, n) == E_ARG
    size = 32 * n
    for off in (0, 32, size - 8, -(size - 8)):                  # out inside a's byte range, from either side
        base = da.ptr + size if off < 0 else da.ptr
        assert call(base, base + off, n) == E_ARG, off
    assert call(da.ptr, da.ptr + size, 2 * n) == E_ARG          # twice as long: the second half is inside the range
    assert call(da.ptr, do.ptr, 0) == 0 and call(None, None, 0) == 0      # n = 0: OK, nothing launched
    engine.sync()
    assert np.array_equal(do.download(), fill) and np.array_equal(da.download(), fill), "nothing written"
    assert call(da.ptr, da.ptr + size, n) == 0                  # adjacent halves of one allocation do not overlap: the call runs
    engine.sync()
    got = da.download()
    v = int.from_bytes(np.full(4, SENTINEL, dtype=np.uint64).tobytes(), "little")
    assert np.array_equal(got[0], fill[0]) and np.array_equal(np.ascontiguousarray(got[1].T), limbs([E.inv(v)] * n))
