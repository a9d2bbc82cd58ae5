"""GPU: the grouped linear combination over Fr and the powers of the fold challenges -- sylow_hip_fr_lincomb_batch and
sylow_hip_fr_group_powers_batch (kzg_multi.hip) -- word for word against the integer model of tests/kzg_multi_model.py.  Sizes come from
kzg_multi_plan.hpp: T columns per tile, FL products per reduction, the cap of the grid's y."""
import random

import numpy as np
import pytest

import kzg_multi_model as M
import kzg_prove_model as KP
from kzg_multi_model import P, R, TOP

pytestmark = pytest.mark.gpu
E_ARG = -2
K = M.plan_constants()
T, FL, Y_CAP = K["KZGM_LINCOMB_TILE"], K["KZGM_LINCOMB_FLUSH"], K["KZGM_GRID_Y_CAP"]
RAGGED = [0, 1, 2, FL - 1, 0, FL, FL + 1, 2 * FL + 1, 0]            # an empty group first, in the middle and last
SENTINEL = 0x5A5A5A5A5A5A5A5A


def words(rng, n, edges=True):
    out = [rng.randrange(1 << 256) for _ in range(n)]
    if edges:
        for i, w in enumerate(M.EDGE_WORDS):
            if i < n:
                out[(i * 5) % n] = w
    return out


def check(engine, a, w, gs):
    got = engine.fr_lincomb(KP.poly_words(a), M.limbs(w), gs)
    want = M.lincomb(a, w, gs)
    assert got.shape == (len(gs) - 1, len(a[0]), 4)
    for g, row in enumerate(want):
        assert np.array_equal(got[g], M.limbs(row)), f"group {g}: {int((got[g] != M.limbs(row)).any(axis=1).sum())} columns differ"
    return got


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 2 * T + 1])
def test_ragged_groups_at_every_tile_edge(engine, n):
    rng = random.Random(0xD0 + n)
    gs = M.offsets(RAGGED)
    a = [words(rng, n) for _ in range(gs[-1])]
    got = check(engine, a, words(rng, gs[-1]), gs)
    assert not got[0].any() and not got[4].any() and not got[8].any()      # the empty groups are written, as zeros
    assert all(v < R for v in M.ints(got.reshape(-1, 4)))                   # canonical, whatever the words were


@pytest.mark.parametrize("coeff", [TOP, R - 1])
def test_accumulator_bound(engine, coeff):
    """FL + 1 terms of the largest factors: every product is (r - 1)^2 after the loads reduce their words, FL of them and the residue of
    the round before must fit the sixteen limbs."""
    m, n = FL + 1, T + 1
    check(engine, [[coeff] * n for _ in range(m)], [R - 1] * m, [0, m])
    check(engine, [[coeff] * n for _ in range(2 * m)], [R - 1] * m + [TOP] * m, [0, 2 * m])


def test_edge_words_on_both_sides(engine):
    e = M.EDGE_WORDS
    a = [[x] * len(e) for x in e]                                           # polynomial j holds word j in every column
    gs = M.offsets([len(e)])
    for wj in e:
        check(engine, a, [wj] * len(e), gs)
    check(engine, [list(e) for _ in e], e, M.offsets([3, len(e) - 3]))       # every word in every column against every word as weight
    assert {0, 1, R - 1, R, R + 1, P, TOP} == set(e)


def test_groups_past_the_cap_of_the_grid(engine):
    """G one above the cap of the grid's y at len = 1: the last group is reached by the stride"""
    rng = random.Random(0xD1)
    sizes = [rng.choice([0, 1, 1, 2, 3]) for _ in range(Y_CAP + 1)]
    sizes[-1] = 2
    gs = M.offsets(sizes)
    a = [words(rng, 1, edges=False) for _ in range(gs[-1])]
    check(engine, a, words(rng, gs[-1]), gs)


def test_group_powers(engine):
    rng = random.Random(0xD2)
    sizes = [0, 5, 1, 0, 40, 3, 2, 0]
    gamma = [7, 0, 1, 9, R - 1, R + 1, TOP, 11]
    gs = M.offsets(sizes)
    got = engine.fr_group_powers(M.limbs(gamma), gs, gs[-1])
    assert np.array_equal(got, M.limbs(M.powers(gamma, gs)))
    assert M.ints(got)[:5] == [1, 0, 0, 0, 0]                               # gamma = 0: 1, 0, 0, ...
    # one group longer than 2^16 (the exponent has 17 bits), and many groups past one block of lanes
    m = (1 << 16) + 3
    g = rng.randrange(R)
    got = engine.fr_group_powers(M.limbs([g]), [0, m], m)
    want, p = [], 1
    for _ in range(m):
        want.append(p)
        p = p * g % R
    assert np.array_equal(got, M.limbs(want))
    sizes = [rng.choice([0, 1, 2, 5]) for _ in range(700)]
    gs, gamma = M.offsets(sizes), [rng.randrange(1 << 256) for _ in sizes]
    assert np.array_equal(engine.fr_group_powers(M.limbs(gamma), gs, gs[-1]), M.limbs(M.powers(gamma, gs)))


def test_python_layer_takes_group_sizes(engine):
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0xD3)
    a = [words(rng, 5) for _ in range(4)]
    w = words(rng, 4)
    got = api.fr_lincomb(a, w, [1, 0, 3])
    assert np.array_equal(got, np.stack([M.limbs(row) for row in M.lincomb(a, w, [0, 1, 1, 4])]))
    with pytest.raises(ValueError):
        api.fr_lincomb(a, w, [1, 2])


def test_argument_errors_write_nothing_and_empty_batch(engine):
    lib = engine.lib
    n, m, G = 8, 3, 2
    fill = np.full((m, 4, n), SENTINEL, dtype=np.uint64)
    da, dw, do = engine.to_device(fill), engine.to_device(fill[0, :, :m].copy()), engine.to_device(fill)
    gs = np.array([0, 1, 3], dtype=np.uint64)
    lin = lambda *x: lib.sylow_hip_fr_lincomb_batch(*x, engine.stream)
    good = (da.ptr, n, m, dw.ptr, gs.ctypes.data, G, do.ptr)
    for i in (0, 3, 4, 6):                                                  # every required pointer as NULL
        assert lin(*[None if k == i else v for k, v in enumerate(good)]) == E_ARG, i
    assert b"bad argument" in lib.sylow_hip_last_error()
    assert lin(da.ptr, 0, m, dw.ptr, gs.ctypes.data, G, do.ptr) == E_ARG    # len = 0
    assert lin(da.ptr, 0, 0, dw.ptr, gs.ctypes.data, G, do.ptr) == E_ARG    # ... is checked before the empty batch returns
    for bad in ([0, 2, 1], [1, 1, 3], [0, 1, 2], [0, 1, 4], [0, 4, 3]):     # decreasing, not from 0, not ending at m (short, long), both
        b = np.array(bad, dtype=np.uint64)
        assert lin(da.ptr, n, m, dw.ptr, b.ctypes.data, G, do.ptr) == E_ARG, bad
    size = 32 * n
    for off in (0, 8, m * size - 8):                                        # out inside a's byte range
        assert lin(da.ptr, n, m, dw.ptr, gs.ctypes.data, G, da.ptr + off) == E_ARG, off
    tail = np.array([0, 0, 1], dtype=np.uint64)
    assert lin(da.ptr + 2 * size, n, 1, dw.ptr, tail.ctypes.data, G, da.ptr + size - 8) == E_ARG      # from the other side
    assert lin(da.ptr, n, 0, dw.ptr, gs.ctypes.data, G, do.ptr) == 0 and lin(da.ptr, n, m, dw.ptr, gs.ctypes.data, 0, do.ptr) == 0
    assert lin(None, n, 0, None, None, 0, None) == 0                        # the empty batch: OK, nothing launched
    pw = lambda *x: lib.sylow_hip_fr_group_powers_batch(*x, engine.stream)
    assert pw(None, gs.ctypes.data, G, m, do.ptr) == E_ARG and pw(dw.ptr, None, G, m, do.ptr) == E_ARG and pw(dw.ptr, gs.ctypes.data, G, m, None) == E_ARG
    assert pw(dw.ptr, gs.ctypes.data, G, m + 1, do.ptr) == E_ARG and pw(dw.ptr, gs.ctypes.data, G, 0, do.ptr) == 0 and pw(None, None, 0, m, None) == 0
    engine.sync()
    for d in (da, do):
        assert np.array_equal(d.download(), fill), "nothing written"
    # adjacent, not overlapping: the second and third array of one allocation fold into its first
    pair = np.array([0, 2], dtype=np.uint64)
    assert lin(da.ptr + size, n, 2, dw.ptr, pair.ctypes.data, 1, da.ptr) == 0
    engine.sync()
    v = int.from_bytes(np.full(4, SENTINEL, dtype=np.uint64).tobytes(), "little") % R
    got = da.download()
    assert np.array_equal(got[1:], fill[1:]) and np.array_equal(got[0].T, M.limbs([2 * v * v % R] * n))
