"""GPU: the scans over Fr of include/sylow_hip_fr_scan.h (fr_scan.hip) -- sylow_hip_fr_scan_batch and sylow_hip_fr_ratio_scan_batch, with their
_tuned forms -- word for word against the integer model of tests/fr_scan_model.py and, independently of the model, word for word through entry
points the library had before: out[k + 1] = out[k] o a[k] by fr_mul / fr_add, and out[k + 1] den[k] = out[k] num[k] for the ratio scan.  Sizes
come from fr_scan_plan.hpp: a lane's elements L, a chunk CH = 256 L, the tile of the second level."""
import random

import numpy as np
import pytest

import fr_scan_model as M
from groth16_model import ints, limbs
from kzg_evals_model import EDGE_WORDS

pytestmark = pytest.mark.gpu
R = M.R
K = M.plan_constants()
L, BLOCK, CH, TILE = K["SCAN_LANE_ELEMS"], K["SCAN_BLOCK"], K["SCAN_CHUNK"], K["SCAN_TOTALS_TILE_DEFAULT"]
SIZES = [1, L - 1, L, L + 1, CH - 1, CH, CH + 1, 3 * CH + L + 1]
ONE, ZERO = limbs([1]).reshape(4), limbs([0]).reshape(4)
IDENT = {M.SUM: ZERO, M.PRODUCT: ONE}


def rand_words(rng, n):
    """any 256-bit words"""
    return np.frombuffer(rng.randbytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()


def with_edges(rng, n):
    a = rand_words(rng, n)
    for i, w in enumerate(EDGE_WORDS):
        a[(i * 37) % n if i % 2 else n - 1 - (i * 11) % n] = limbs([w])[0]
    return a


def combine(engine, op, a, b):
    return engine.fr_mul(a, b) if op == M.PRODUCT else engine.fr_add(a, b)


def relation(engine, a, op, exclusive, out, total):
    """one row, through fr_mul / fr_add alone: the first element, then out[k + 1] = out[k] o a[k (+ 1)], then the total"""
    n = len(a)
    canon = engine.fr_add(a, np.zeros_like(a))                       # a mod r
    assert np.array_equal(out[0], IDENT[op] if exclusive else canon[0])
    if n > 1:
        step = a[:-1] if exclusive else a[1:]
        assert np.array_equal(out[1:], combine(engine, op, out[:-1], step)), "out[k + 1] = out[k] o a[k]"
    last = combine(engine, op, out[-1:], a[-1:])[0] if exclusive else out[-1]
    assert np.array_equal(total, last), "the total"


def ratio_relation(engine, num, den, op, out, total):
    """one row with no zero denominator: out[0] is the identity and out[k + 1] den[k] = out[k] num[k] (product) or
    (out[k + 1] - out[k]) den[k] = num[k] (sum), the total as "out[len]" """
    assert np.array_equal(out[0], IDENT[op])
    nxt = np.concatenate([out[1:], total[None]])
    if op == M.PRODUCT:
        assert np.array_equal(engine.fr_mul(nxt, den), engine.fr_mul(out, num)), "out[k + 1] den[k] = out[k] num[k]"
    else:
        assert np.array_equal(engine.fr_mul(engine.fr_sub(nxt, out), den), engine.fr_add(num, np.zeros_like(num))), "(out[k + 1] - out[k]) den[k] = num[k]"


@pytest.mark.parametrize("n", SIZES)
def test_scan_sizes_against_the_model_and_the_relation(engine, n):
    rng = random.Random(0x5C0 + n)
    for m in (1, 3):
        a = np.stack([with_edges(rng, n) if j == 1 else rand_words(rng, n) for j in range(m)])
        for op in (M.SUM, M.PRODUCT):
            for exclusive in (False, True):
                out, total = engine.fr_scan(a, op, exclusive)
                assert out.shape == (m, n, 4) and total.shape == (m, 4)
                for j in range(m):
                    want, want_total = M.scan(ints(a[j]), op, exclusive)
                    assert np.array_equal(out[j], limbs(want)) and np.array_equal(total[j], limbs([want_total])[0]), (n, m, op, exclusive, j)
                    relation(engine, a[j], op, exclusive, out[j], total[j])


@pytest.mark.parametrize("n", SIZES)
def test_ratio_scan_sizes_against_the_model_and_the_relation(engine, n):
    rng = random.Random(0x5C1 + n)
    for m in (1, 3):
        num = np.stack([with_edges(rng, n) if j == 1 else rand_words(rng, n) for j in range(m)])
        den = np.stack([rand_words(rng, n) for j in range(m)])
        for j in range(m):
            assert all(v % R for v in ints(den[j]))
        for op in (M.SUM, M.PRODUCT):
            out, total, status = engine.fr_ratio_scan(num, den, op)
            assert not status.any()
            for j in range(m):
                want, want_total, _ = M.ratio_scan(ints(num[j]), ints(den[j]), op)
                assert np.array_equal(out[j], limbs(want)) and np.array_equal(total[j], limbs([want_total])[0]), (n, m, op, j)
                ratio_relation(engine, num[j], den[j], op, out[j], total[j])


def test_edge_words_as_denominators(engine):
    """0, r and 2 r are zero denominators; 1, r - 1, r + 1, p and 2^256 - 1 are not"""
    rng = random.Random(0x5C2)
    den = limbs(EDGE_WORDS)
    num = rand_words(rng, len(den))
    for op in (M.SUM, M.PRODUCT):
        out, total, status = engine.fr_ratio_scan(num, den, op)
        want, want_total, want_status = M.ratio_scan(ints(num), EDGE_WORDS, op)
        assert np.array_equal(out, limbs(want)) and np.array_equal(total, limbs([want_total])[0]) and status == want_status == 1


@pytest.mark.parametrize("totals_tile", [1, 2])
def test_the_tuned_forms_give_the_default_s_words(engine, totals_tile):
    """5 chunks + 1 element with ONE block: the stride walk of every phase, and at totals_tile 1 and 2 the carry across tiles"""
    n, m = 5 * CH + 1, 2
    rng = random.Random(0x5C3)
    a, num, den = (np.stack([rand_words(rng, n) for _ in range(m)]) for _ in range(3))
    for op in (M.SUM, M.PRODUCT):
        for exclusive in (False, True):
            base = engine.fr_scan(a, op, exclusive)
            got = engine.fr_scan(a, op, exclusive, max_blocks=1, totals_tile=totals_tile)
            assert all(np.array_equal(x, y) for x, y in zip(base, got)), (op, exclusive)
        base = engine.fr_ratio_scan(num, den, op)
        got = engine.fr_ratio_scan(num, den, op, max_blocks=1, totals_tile=totals_tile)
        assert all(np.array_equal(x, y) for x, y in zip(base, got)), op
    want, want_total = M.scan(ints(a[1]), M.PRODUCT, True)
    out, total = engine.fr_scan(a, M.PRODUCT, True, max_blocks=1, totals_tile=totals_tile)
    assert np.array_equal(out[1], limbs(want)) and np.array_equal(total[1], limbs([want_total])[0])
    out, total = engine.fr_scan(a, M.SUM, False, max_blocks=3, totals_tile=K["SCAN_TOTALS_TILE_MAX"])
    assert np.array_equal(out[0], limbs(M.scan(ints(a[0]), M.SUM)[0]))


PLACES = {"first of the array": 0, "last of lane 0": L - 1, "first of lane 1": L, "last of chunk 0": CH - 1, "first of chunk 1": CH, "last of the array": 3 * CH + L}


@pytest.mark.parametrize("at", list(PLACES))
def test_a_lone_zero(engine, at):
    """in `a` under the product, and in `den`: the words before it are untouched, the words after it are the model's, and status bit 0 is
    set in that row only"""
    n, k = 3 * CH + L + 1, PLACES[at]
    rng = random.Random(0x5C4 + k)
    a = np.stack([limbs([rng.randrange(1, R) for _ in range(n)]) for _ in range(3)])
    clean, clean_total = engine.fr_scan(a, M.PRODUCT)
    hit = a.copy()
    hit[1, k] = limbs([R])[0] if k % 2 else 0
    out, total = engine.fr_scan(hit, M.PRODUCT)
    assert np.array_equal(out[[0, 2]], clean[[0, 2]]) and np.array_equal(out[1, :k], clean[1, :k]) and not out[1, k:].any()
    assert np.array_equal(total[[0, 2]], clean_total[[0, 2]]) and not total[1].any()
    num = np.stack([limbs([rng.randrange(1, R) for _ in range(n)]) for _ in range(3)])
    for op in (M.SUM, M.PRODUCT):
        clean, clean_total, status = engine.fr_ratio_scan(num, a, op)
        assert not status.any()
        out, total, status = engine.fr_ratio_scan(num, hit, op)
        assert list(status) == [0, 1, 0]
        assert np.array_equal(out[[0, 2]], clean[[0, 2]]) and np.array_equal(total[[0, 2]], clean_total[[0, 2]])
        assert np.array_equal(out[1, :k + 1], clean[1, :k + 1]), "the zero's neighbours in the shared inversion are not disturbed"
        want, want_total, _ = M.ratio_scan(ints(num[1]), ints(hit[1]), op)
        assert np.array_equal(out[1], limbs(want)) and np.array_equal(total[1], limbs([want_total])[0])
        if op == M.PRODUCT:
            assert not out[1, k + 1:].any() and not total[1].any(), "a product row is 0 from there on"


def test_257_chunks_and_one(engine):
    """More chunk totals than a tile of the second level holds: the relation alone over the whole row, and the model at four sampled
    indices as direct prefix products"""
    n = (TILE + 1) * CH + 1
    rng = random.Random(0x5C5)
    num, den = rand_words(rng, n), rand_words(rng, n)
    out, total, status = engine.fr_ratio_scan(num, den, M.PRODUCT)
    assert status == 0
    ratio_relation(engine, num, den, M.PRODUCT, out, total)
    ni, di = ints(num), ints(den)
    at = [CH + 1, TILE * CH - 1, TILE * CH + 5, n - 1]
    pn = pd = 1
    want, k = [], 0
    for stop in at:
        while k < stop:
            pn, pd, k = pn * ni[k] % R, pd * di[k] % R, k + 1
        want.append(pn * pow(pd, -1, R) % R)
    assert np.array_equal(out[at], limbs(want))
    inc, inc_total = engine.fr_scan(den, M.PRODUCT)
    relation(engine, den, M.PRODUCT, False, inc, inc_total)
    assert np.array_equal(inc[n - 2], limbs([pd])[0])


def test_num_null_is_num_ones(engine):
    rng = random.Random(0x5C6)
    n = CH + L + 1
    den = np.stack([rand_words(rng, n) for _ in range(2)])
    den[1, 5] = 0
    ones = np.tile(ONE, (2, n, 1))
    for op in (M.SUM, M.PRODUCT):
        a, b = engine.fr_ratio_scan(None, den, op), engine.fr_ratio_scan(ones, den, op)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and list(a[2]) == [0, 1]
    out, total, _ = engine.fr_ratio_scan(None, den[0], M.PRODUCT)
    assert np.array_equal(engine.fr_mul(total[None], engine.fr_scan(den[0], M.PRODUCT)[1][None])[0], ONE), "the total is the inverse of the product"


def test_api_cumsum_and_cumprod(engine):
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0x5C7)
    vals = [rng.randrange(R) for _ in range(CH + 3)]
    a = api.Fr.from_ints(vals)
    assert ints(a.cumsum().v) == M.scan(vals, M.SUM)[0] and ints(a.cumprod().v) == M.scan(vals, M.PRODUCT)[0]
    assert ints(a.cumsum(exclusive=True).v) == M.scan(vals, M.SUM, True)[0] and ints(a.cumprod(exclusive=True).v) == M.scan(vals, M.PRODUCT, True)[0]
    assert len(api.Fr(np.zeros((0, 4), dtype=np.uint64)).cumprod()) == 0
