"""GPU: the radix-2 transform over G1 points -- sylow_hip_g1_ntt_batch(_tuned) (g1_ntt.hip) -- word for word against the model of
tests/g1_ntt_model.py (the integer transform over the discrete logarithms, then the oracle's fixed-base product) at n <= 256, and at 2^10
and 2^13 against the library's own independent route to the same points: g1_generator_mul(fr_ntt(s)).  The inputs of a size are made once
per module and shared.

Planted among the random logarithms of every array that has room: 0 as a FLAGGED point whose words are garbage, 0 as an UNFLAGGED (0, 1),
a pair s, r - s half a transform apart (U + V is the identity in the first stage) and a pair s, s half a transform apart (U - V is the
identity, U + V a doubling).  Arrays of fewer than 8 points carry them by turns (array j of a batch takes turn j)."""
import random

import numpy as np
import pytest

import g1_ntt_model as M
import ntt_model as N
from groth16_model import limbs
from ntt_model import R

pytestmark = pytest.mark.gpu
IDENTITY = limbs([0, 1]).reshape(8)
GARBAGE = np.array([0xDEADBEEF00000001, 2, 3, 0x1111111111111111, 0xFFFFFFFFFFFFFFFF, 5, 6, 0x2FFFFFFFFFFFFFFF], dtype=np.uint64)
FLAGGED, BARE = "flagged", "bare"          # the two ways a zero logarithm is handed over
_INPUTS = {}


def planted(rng, n, turn):
    """(logs, {index: FLAGGED | BARE})"""
    s = [rng.randrange(1, R) for _ in range(n)]
    how, h = {}, n // 2
    if n >= 8:
        s[0], s[1] = 0, 0
        how = {0: FLAGGED, 1: BARE}
        s[2 + h] = R - s[2]
        s[3 + h] = s[3]
    elif n == 4:
        if turn % 3 == 0:
            s[2], s[3] = R - s[0], s[1]
        elif turn % 3 == 1:
            s[0], s[1], how = 0, 0, {0: FLAGGED, 1: BARE}
    elif n == 2:
        if turn % 3 == 0:
            s[1] = R - s[0]
        elif turn % 3 == 1:
            s[1] = s[0]
        else:
            s, how = [0, 0], {0: FLAGGED, 1: BARE}
    elif turn % 3:
        s, how = [0], {0: FLAGGED if turn % 3 == 1 else BARE}
    return s, how


def array_of(logs, how):
    """(words [n, 8], flags [n]) of the points s_k G1gen, zeros handed over as `how` says"""
    xy, inf = M.points(logs)
    for i, kind in how.items():
        assert inf[i]
        xy[i], inf[i] = (GARBAGE, 1) if kind == FLAGGED else (IDENTITY, 0)
    return xy, inf


def inputs(log_n):
    """three arrays of 2^log_n points from different seeds, made once: [(logs, words, flags)]"""
    if log_n not in _INPUTS:
        out = []
        for j in range(3):
            logs, how = planted(random.Random(0x6170 + 16 * log_n + j), 1 << log_n, j)
            out.append((logs,) + array_of(logs, how))
        _INPUTS[log_n] = out
    return _INPUTS[log_n]


def check(got, want, what):
    (gxy, ginf), (wxy, winf) = got, want
    assert np.array_equal(np.asarray(ginf).astype(np.uint8), np.asarray(winf).astype(np.uint8)), f"{what}: flags {list(ginf)[:16]} against {list(winf)[:16]}"
    bad = np.flatnonzero((np.asarray(gxy) != np.asarray(wxy)).any(axis=-1).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} points differ, first at {bad[:8]}"


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 8])
def test_against_the_model(engine, log_n, inverse, m):
    arrays = inputs(log_n)[:m]
    xy, inf = engine.g1_ntt(np.stack([a[1] for a in arrays]), np.stack([a[2] for a in arrays]), inverse=inverse)
    assert xy.shape == (m, 1 << log_n, 8) and inf.shape == (m, 1 << log_n)
    for j, (logs, _, _) in enumerate(arrays):
        check((xy[j], inf[j]), M.expected(logs, log_n, inverse), f"array {j}")


def test_the_planted_cases_are_what_they_claim():
    """CPU side of the inputs: at n = 8 the first stage meets U + V = 0 at butterfly 2 and U - V = 0 at butterfly 3, and both zeros are there"""
    logs, xy, inf = inputs(3)[0]
    assert (logs[2] + logs[6]) % R == 0 and logs[3] == logs[7] and logs[0] == 0 and logs[1] == 0
    assert inf[0] == 1 and np.array_equal(xy[0], GARBAGE) and inf[1] == 0 and np.array_equal(xy[1], IDENTITY) and not inf[2:].any()


@pytest.mark.parametrize("log_n", [1, 3, 6])
def test_probes(engine, log_n):
    n, s = 1 << log_n, 0x1234567 + log_n
    pxy, _ = M.points([s])
    ids = np.tile(GARBAGE, (n, 1))
    # a delta at 0 gives P everywhere; a delta at 1 gives w^i P: the root and the natural order
    for at, want in ((0, [s] * n), (1, [s * pow(N.omega(log_n), i, R) % R for i in range(n)])):
        xy, inf = ids.copy(), np.ones(n, dtype=np.uint8)
        xy[at], inf[at] = pxy[0], 0
        check(engine.g1_ntt(xy, inf), M.points(want), f"delta at {at}")
    # all points equal: n P at 0 and flagged canonical identities everywhere else
    xy, inf = engine.g1_ntt(np.tile(pxy[0], (n, 1)), None)
    check((xy, inf), M.points([n * s] + [0] * (n - 1)), "all equal")
    assert list(inf) == [0] + [1] * (n - 1) and all(np.array_equal(row, IDENTITY) for row in xy[1:])
    # all flagged gives all flagged, both ways
    for inverse in (False, True):
        xy, inf = engine.g1_ntt(ids, np.ones(n, dtype=np.uint8), inverse=inverse)
        assert inf.all() and all(np.array_equal(row, IDENTITY) for row in xy)


@pytest.mark.parametrize("log_n", [3, 6])
def test_round_trips_word_for_word(engine, log_n):
    rng = random.Random(0x6171 + log_n)
    logs = [rng.randrange(R) for _ in range(1 << log_n)]
    logs[5] = 0                                                         # a canonical identity, flagged, among them
    pxy, pinf = M.points(logs)
    for first in (False, True):
        mid = engine.g1_ntt(pxy, pinf, inverse=first)
        check(engine.g1_ntt(mid[0], mid[1], inverse=not first), (pxy, pinf), "intt(ntt(P))" if not first else "ntt(intt(P))")


# ---- larger sizes, against g1_generator_mul(fr_ntt(s)) ---------------------------------------------------------------------------------
_LARGE = {}


def large(engine, log_n):
    """(points [n, 8], {inverse: (words, flags)}) made once per size by the library's other route"""
    if log_n not in _LARGE:
        n = 1 << log_n
        s = np.frombuffer(random.Random(0x6172 + log_n).randbytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
        s[:, 3] &= 0x0FFFFFFFFFFFFFFF                                   # below r
        pxy, pinf = engine.g1_generator_mul(s)
        assert not pinf.any()
        _LARGE[log_n] = (pxy, {inv: engine.g1_generator_mul(engine.fr_ntt(s, inverse=inv)) for inv in (False, True)})
    return _LARGE[log_n]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", [10, 13])
def test_against_the_generator_route(engine, log_n, inverse):
    pxy, want = large(engine, log_n)
    got = engine.g1_ntt(pxy, None, inverse=inverse)
    check(got, want[inverse], "default plan")
    assert not got[1].any()


@pytest.mark.parametrize("max_blocks", [1, 3])
@pytest.mark.parametrize("log_n", [10, 13])
def test_the_grid_stride_walk_gives_the_same_words(engine, log_n, max_blocks):
    """256 lanes per block: 2^10 points are 2 blocks of butterflies per stage, so max_blocks = 1 strides; 2^13 points are 16"""
    pxy, want = large(engine, log_n)
    inverse = max_blocks == 1
    check(engine.g1_ntt(pxy, None, inverse=inverse, max_blocks=max_blocks), want[inverse], f"max_blocks = {max_blocks}")


def test_null_flags_are_all_zero_flags(engine):
    pxy, want = large(engine, 10)
    check(engine.g1_ntt(pxy, np.zeros(len(pxy), dtype=np.uint8)), want[False], "an all-zero flag array")
    check(engine.g1_ntt(pxy, None), want[False], "p_inf = NULL")


def test_api_layer(engine):
    from sylow_amd import api
    api.set_engine(engine)
    arrays = inputs(3)
    pts = [api.G1Affine(a[1], a[2]) for a in arrays]
    out = api.g1_ntt(pts)
    back = api.g1_intt(out)
    for j, (logs, _, _) in enumerate(arrays):
        check((out[j].xy, out[j].infinity), M.expected(logs, 3), f"api array {j}")
        check((back[j].xy, back[j].infinity), M.points(logs), f"api round trip {j}")
    one = api.g1_ntt(pts[0], inverse=True)
    check((one.xy, one.infinity), M.expected(arrays[0][0], 3, True), "one array")
    with pytest.raises(ValueError):
        api.g1_ntt(api.G1Affine(arrays[0][1][:6]))
