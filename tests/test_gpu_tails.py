"""GPU: fp_is_square and fp_inv on structured Montgomery REPRESENTATIVES, alone and in chosen wavefront compositions.

Both routines loop a number of times that depends on the word they iterate on, which is a = x 2^256 mod p of the value x passed, and both
leave their loops on a wavefront-wide vote.  tests/tail_model.py builds the representatives (small, sparse, one limb against p's eight,
the 507-step 2^253, zero) and says how many Jacobi steps and divsteps each needs; here they are passed as rep_to_value(a), laid out so
that a run of 64 is one wavefront under each kernel's own mapping of elements to lanes (tail_model.wavefronts), and every result is
compared with Python's big-integer power of the value.

What this cannot show.  The tests fix the input classes, not the path: which block or batch a wavefront left its loop at is not
observable from outside.  And no input is known that keeps safegcd's g alive into batches 19 and 20 (more than 540 divsteps; the
family's maximum is 524, 527 among 5000 random words), so those two batches only ever run idle here."""
import numpy as np
import pytest

import kzg_evals_model as E
import tail_model as T
from helpers import ints, limbs
from tail_model import P, R_ORDER, rep_to_value, run_of, wavefronts

pytestmark = pytest.mark.gpu
FAMILY = T.family()
STRUCTURED, BY_LIMBS = T.families()
CH = E.plan_constants()["EVALS_CHUNK"]


def by_jacobi(lo, hi=508):
    steps = T.jacobi_steps()
    return [a for a in FAMILY if lo <= steps[a] <= hi]


def by_divsteps(lo, hi=600):
    ds = T.divsteps()
    return [a for a in FAMILY if a and lo <= ds[a] <= hi]


def check_squares(engine, reps):
    """is_square and sqrt of the values whose representatives are `reps` against Euler's criterion on the value"""
    vals = [rep_to_value(a) for a in reps]
    a = limbs(vals)
    exp = np.array([1 if pow(v, (P - 1) // 2, P) in (0, 1) else 0 for v in vals], dtype=np.uint8)
    flags = engine.fp_is_square(a)
    bad = np.flatnonzero(flags != exp)
    assert bad.size == 0, f"{bad.size} flags differ, first at element {bad[0]}: representative {hex(reps[bad[0]])}, {T.jacobi_steps().get(reps[bad[0]])} steps"
    r, ok = engine.fp_sqrt(a)
    assert np.array_equal(ok, flags)
    assert all(y * y % P == v for v, y, e in zip(vals, ints(r), exp) if e)


def test_is_square_and_sqrt_by_representative(engine):
    assert len(by_jacobi(402)) >= 200 and (1 << 253) in FAMILY and 0 in FAMILY
    check_squares(engine, FAMILY)


ZEROS = [0] * 64
SQUARE_RUNS = ["64 lanes of 500 steps and more", "the 507-step lane among 63 of 254 steps", "64 one-limb representatives",
               "lane l on (l mod 8) + 1 limbs", "64 zeros", "zeros between slow lanes"]


def square_runs(name):
    slow = run_of(by_jacobi(500))
    return {
        "64 lanes of 500 steps and more": [slow],
        "the 507-step lane among 63 of 254 steps": [[1] * l + [1 << 253] + [1] * (63 - l) for l in (0, 31, 32, 63)],
        "64 one-limb representatives": [BY_LIMBS[1][:64]],
        "lane l on (l mod 8) + 1 limbs": [[BY_LIMBS[l % 8 + 1][l] for l in range(64)], [BY_LIMBS[(l + 3) % 8 + 1][64 + l] for l in range(64)]],
        "64 zeros": [ZEROS],
        "zeros between slow lanes": [[0 if l % 2 else a for l, a in enumerate(slow)], [a if l % 2 else 0 for l, a in enumerate(slow)]],
    }[name]


@pytest.mark.parametrize("name", SQUARE_RUNS)
def test_is_square_wavefront_compositions(engine, name):
    """k_fp_sqrt: thread t takes element t, so each run of 64 is one wavefront; runs alone in their launch and all in one"""
    runs = square_runs(name)
    assert len(by_jacobi(500)) >= 8 and all(len(r) == 64 for r in runs)
    for r in runs:
        check_squares(engine, wavefronts([r], "thread"))
    check_squares(engine, wavefronts(runs, "thread"))


@pytest.mark.parametrize("n", [1, 63, 64 + 1, 64 + 63, 3 * 64 + 1, 3 * 64 + 63, 4 * 64 + 1, 4 * 64 + 63])
def test_is_square_ragged_last_wavefront_of_slow_lanes(engine, n):
    """the lanes past n have left the kernel and must not vote: a last wavefront of 1 or 63 lanes, all of 500 steps and more, after whole
    wavefronts that finish in 254"""
    reps = wavefronts([[1] * 64] * (n // 64), "thread", tail=run_of(by_jacobi(500)[::-1], n % 64))
    assert len(reps) == n
    check_squares(engine, reps)


def inverses(vals):
    return limbs([pow(v, P - 2, P) for v in vals])


def check_inverses(engine, reps_thread, reps_pair=None):
    """fp_inv_batch on the "pair" layout, the hook's safegcd (op 4) and its Fermat twin (op 5) on the "thread" layout: pow(v, p - 2, p)"""
    vt = [rep_to_value(a) for a in reps_thread]
    vp = vt if reps_pair is None else [rep_to_value(a) for a in reps_pair]
    got = engine.fp_inv(limbs(vp))
    exp = inverses(vp)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"fp_inv_batch: {bad.size} differ, first at element {bad[0]} of {len(vp)}"
    a, exp = limbs(vt), inverses(vt)
    for op in (4, 5):
        got = engine.f29_hook(op, a, np.zeros_like(a))
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert bad.size == 0, f"f29_hook op {op}: {bad.size} differ, first at element {bad[0]} of {len(vt)}"


def test_inversion_by_representative(engine):
    assert len(by_divsteps(1, 510)) >= 300 and len(by_divsteps(511)) >= 300
    check_inverses(engine, FAMILY)


INVERSE_RUNS = ["all zeros: leaves before batch 17", "64 lanes within 510 divsteps: may leave before batch 18", "64 lanes of 511 divsteps and more",
                "one lane of 520 and more among 63 fast, lane 0", "one lane of 520 and more among 63 fast, lane 63", "one fast lane among 63 slow"]


def inverse_runs(name):
    fast, slow, slowest = by_divsteps(1, 510), by_divsteps(511), by_divsteps(520)
    assert len(fast) >= 192 and len(slow) >= 128 and slowest
    return {
        "all zeros: leaves before batch 17": [ZEROS],
        "64 lanes within 510 divsteps: may leave before batch 18": [run_of(fast), run_of(fast[64:]), run_of([0] + fast[128:])],
        "64 lanes of 511 divsteps and more": [run_of(slow), run_of(slow[64:])],
        "one lane of 520 and more among 63 fast, lane 0": [[slowest[0]] + run_of(fast, 63)],
        "one lane of 520 and more among 63 fast, lane 63": [run_of(fast[7:], 63) + [slowest[-1]]],
        "one fast lane among 63 slow": [run_of(slow, 20) + [fast[0]] + run_of(slow[20:], 43)],
    }[name]


@pytest.mark.parametrize("name", INVERSE_RUNS)
def test_inversion_wavefront_compositions(engine, name):
    """Each run of 64 is one wavefront-wide call of fp_inv: elements 64 w + l under the hook, elements 128 w + 2 l (and the odd ones, a
    second call) under fp_inv_batch"""
    runs = inverse_runs(name)
    assert all(len(r) == 64 for r in runs)
    for r in runs:
        check_inverses(engine, wavefronts([r], "thread"), wavefronts([r], "pair"))
    check_inverses(engine, wavefronts(runs, "thread"), wavefronts(runs, "pair"))


@pytest.mark.parametrize("n", [1, 63, 2 * 64 + 1, 2 * 64 + 63, 3 * 64 + 1, 3 * 64 + 63])
def test_inversion_ragged_last_wavefront_of_slow_lanes(engine, n):
    """whole fast wavefronts, then a last one whose live lanes all need 511 divsteps and more.  fp_inv_batch's wavefront covers 128
    elements (an odd n takes its scalar path, lane by lane over 2 t and 2 t + 1): everything past the last multiple of 128 is slow"""
    fast, slow = run_of(by_divsteps(1, 510)), by_divsteps(511)
    thread = wavefronts([fast] * (n // 64), "thread", tail=run_of(slow, n % 64))
    pair = wavefronts([fast] * (n // 128 * 2), "pair", tail=run_of(slow, n % 128))
    assert len(thread) == n == len(pair)
    check_inverses(engine, thread, pair)


def test_svdw_map_inversion_by_representative(engine, coracle):
    """k_svdw_map (g1.hip) carries its own copy of the inversion: it inverts d_i d_(i^1) with d = 1 - 16 u^4 (c1 = 4).  With u = 0 as
    the partner the product is d alone, so a target representative D is met by d = rep_to_value(D), u^4 = (1 - d) / 16: solvable where
    that is a non-zero square, since p = 3 mod 4 makes one of its two roots a square again.  Both lanes of a pair invert the same d, so 32
    pairs of targets within 510 divsteps are one wavefront that may leave safegcd early.  The map's own fp_is_square inputs (gx1, gx2)
    are cubics in the inverse: steering them needs cube roots, and 9 divides p - 1, so they are left to chance here.
    Of the 3666 non-zero targets 1819 are solvable, 777 of those within 510 divsteps (of the 1266 structured ones: 632 and 313)."""
    ds = T.divsteps()
    inv16, e = pow(16, P - 2, P), (P + 1) // 4
    solved = []
    for D in FAMILY:
        if not D:
            continue
        d = rep_to_value(D)
        w = (1 - d) * inv16 % P
        if w and pow(w, (P - 1) // 2, P) == 1:
            u = pow(pow(w, e, P), e, P)                         # w^e is the root of w that is a square; its root
            assert (1 - 16 * pow(u, 4, P)) % P == d
            solved.append((ds[D], u))
    assert len(solved) >= 0.4 * (len(FAMILY) - 1)
    fast = [u for k, u in solved if k <= 510]
    slow = [u for k, u in solved if k > 510]
    assert len(fast) >= 64 and len(slow) >= 32
    fast = fast[:len(fast) // 32 * 32]                          # whole wavefronts of fast pairs first, then the rest
    us = [x for u in fast + slow for x in (u, 0)]
    us += [slow[0], slow[1], 0, 0, fast[0]]                     # two live partners, two zeros, an odd length
    xy, st = engine.svdw_map(limbs(us))
    assert not st.any()
    assert np.array_equal(xy, coracle.svdw_map(limbs(us)))


FR = T.fr_sparse()


def test_fr_batch_inv_sparse_words_one_at_a_time(engine):
    """Fr is canonical: the word passed is the word the chunk's one Euclidean inversion (bn254_fr_euclid.hpp) runs on when it is the only
    element, or the only one that is not 1.  Arrays of length 1."""
    x = limbs(FR)
    exp = limbs([pow(v, R_ORDER - 2, R_ORDER) for v in FR])
    assert np.array_equal(engine.fr_inv(x), exp)
    for i in range(len(FR)):
        assert np.array_equal(engine.fr_batch_inv(x[i:i + 1]), exp[i:i + 1]), hex(FR[i])


@pytest.mark.parametrize("at", ["first", "last"])
def test_fr_batch_inv_sparse_word_in_a_chunk_of_ones(engine, at):
    """one full chunk, all ones but x at its first or last position: the chunk's product, the word inverted, is x"""
    x = limbs(FR)
    exp = limbs([pow(v, R_ORDER - 2, R_ORDER) for v in FR])
    k = 0 if at == "first" else CH - 1
    a = np.tile(limbs([1]), (CH, 1))
    want = a.copy()
    for i in range(len(FR)):
        a[k], want[k] = x[i], exp[i]
        assert np.array_equal(engine.fr_batch_inv(a), want), hex(FR[i])
