"""GPU: the carry-free core's routines on raw limbs (sylow_hip_f29_raw_hook_batch) against tools/f29_model.py, word for word, on the
vectors of tests/test_f29_model.py that sit on each stated bound plus a few thousand random in-bound ones.  Only vectors the model accepts
(no i32 / u32 / i64 value would wrap) go to the device."""
import random

import numpy as np
import pytest

import test_f29_model as T
from test_f29_model import B29, TOP, M

pytestmark = pytest.mark.gpu


def pack16(k):
    """four coefficients -> (k0, k1) for hook ops 10 / 12: two signed 16-bit halves each"""
    k = list(k) + [0] * (4 - len(k))
    lo = lambda a, b: np.int32(np.uint32((a & 0xFFFF) | ((b & 0xFFFF) << 16))).item()
    return lo(k[0], k[1]), lo(k[2], k[3])


def run(engine, op, cases, model, k0=0, k1=0):
    """cases: tuples of 9-limb operands; every case the model accepts goes to the device in one launch, the outputs must be identical"""
    ok, want = [], []
    for c in cases:
        try:
            want.append(model(*c))
        except M.Overflow:
            continue
        ok.append(c)
    assert ok, op
    arity = len(ok[0])
    ops = [np.array([c[j] for c in ok], dtype=np.int64).astype(np.int32) for j in range(arity)]
    got = engine.f29_raw(op, *ops, k0=k0, k1=k1)
    exp = np.array(want, dtype=np.int64).astype(np.int32)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (op, k0, k1, len(bad), ok[bad[0]], got[bad[0]].tolist(), exp[bad[0]].tolist())
    return len(ok)


def u32_as_i32(words):
    return [w - (1 << 32) if w >= 1 << 31 else w for w in words]


def test_norm_family(engine):
    rng = random.Random(11)
    assert run(engine, 0, [(a,) for a in T.bound_vectors(3 * B29, 3 << 28, rng, 1000)], M.norm) > 1000
    assert run(engine, 1, [(a,) for a in T.bound_vectors(B29 - 1, TOP, rng, 1000, nonneg=True)], M.norm_x8) > 1000
    vs = T.bound_vectors(B29 - 1, B29 - 1, rng, 20)
    pairs = [(a, b) for a in vs for b in vs] + [([-(B29 - 1)] * 9, [B29 - 1] * 9), ([B29 - 1] * 9, [-(B29 - 1)] * 9)]
    assert run(engine, 2, pairs, M.norm_sub3) == len(pairs)


def test_mul_inline_and_leaf(engine):
    cases = T.mul_cases(random.Random(12), n_random=400)
    assert run(engine, 3, cases, M.mul) == len(cases)
    assert run(engine, 4, cases, M.mul) == len(cases)            # f29_mul_leaf: the out-of-line form the hot kernels call


def test_sqr_and_dot2(engine):
    rng = random.Random(13)
    sq = [(a,) for a in T.sqr_cases(rng, n_random=1500)]
    assert run(engine, 5, sq, M.sqr) == len(sq)
    d2 = T.dot2_cases(rng, n_random=1500)
    assert run(engine, 6, d2, M.dot2) == len(d2)
    assert run(engine, 7, d2, M.dot2_ilp) == len(d2)


def test_reduce_from_edges(engine):
    """|limb| = 2^36 - 1, |top| = 2^31 - 1 and the rounding boundaries of the quotient estimate (a K off by one fails here)"""
    cases = T.reduce_cases(random.Random(14), n_random=2000)
    groups = {}
    for a, b, k0, k1 in cases:
        groups.setdefault((k0, k1), []).append((a, b))
    for (k0, k1), ab in groups.items():
        assert run(engine, 8, ab, lambda a, b: M.reduce_from(T.reduce_limbs(a, b, k0, k1)), k0, k1) == len(ab)


def test_linear_passes_at_call_site_coefficients(engine):
    """every CALL_SITES coefficient vector with at most four terms, operands at the site's limb bound in both sign patterns, plus
    random operands inside it; two-term vectors through f29_lin2 / norm_terms<2> as well"""
    rng = random.Random(15)
    launched = 0
    for key, row in T.CALL_SITES.items():
        if row is None or row[0] == "xi_lin":
            continue
        kind, lim, variants = row[:3]
        top = int((row[3] if len(row) > 3 else T.VMAX) * T.PT) + 1
        for kvec in variants:
            if len(kvec) > 4:
                continue
            cases = []
            for sign in (1, -1):
                cases.append(tuple(T.site_operands(lim, top, kvec, sign)))
            for _ in range(200):
                cases.append(tuple([rng.randint(-lim, lim) for _ in range(8)] + [rng.randint(-top, top)] for _ in kvec))
            pad = [c + ([0] * 9,) * (4 - len(kvec)) for c in cases]
            k4 = list(kvec) + [0] * (4 - len(kvec))
            if kind == "reduce":
                launched += run(engine, 10, pad, lambda *x: M.reduce_terms(list(x), k4), *pack16(kvec))
                if len(kvec) == 2:
                    launched += run(engine, 9, cases, lambda a, b: M.lin2(a, kvec[0], b, kvec[1]), *kvec)
            else:
                launched += run(engine, 12, pad, lambda *x: M.norm_terms(list(x), k4), *pack16(kvec))
                if len(kvec) == 2:
                    launched += run(engine, 11, cases, lambda a, b: M.norm_terms([a, b], list(kvec)), *kvec)
    assert launched > 5000


def test_xi_lin_at_its_bounds(engine):
    rng = random.Random(16)
    lim = (1 << 31) - 1
    for k, m in ((1, 1), (3, 2), (-1, 1), (1, 0), (6, 2)):
        top = ((1 << 31) - 1) // (10 * abs(k) + abs(m))
        low = min(lim, ((1 << 36) - 1) // (10 * abs(k) + abs(m)))
        cases = []
        for kind in ("pos", "neg", "alt", "tla"):
            for s in (1, -1):
                x0 = T.pattern(low, 0, kind, s)[:8] + [s * top]
                x1 = [-v for v in x0]
                cases += [(x0, x1, x0, x1), (x0, x0, x0, x0)]
        for _ in range(300):
            cases.append(tuple([rng.randint(-low, low) for _ in range(8)] + [rng.randint(-top // 2, top // 2)] for _ in range(4)))
        model = lambda x0, x1, y0, y1: sum(M.u2_xi_lin(x0, x1, y0, y1, k, m), [])
        assert run(engine, 13, cases, model, k, m) == len(cases)


def test_to_fp_and_from_fp(engine):
    rng = random.Random(17)
    cases = [(a,) for a in T.to_fp_cases(rng, n_random=2000)]
    assert run(engine, 14, cases, lambda a: u32_as_i32(M.to_fp(a)) + [0]) == len(cases)
    words = [M.int_to_words(x) for x in [0, 1, M.P - 1, M.P, (1 << 256) - 1, 1 << 255] + [rng.randrange(1 << 256) for _ in range(1000)]]
    cases = [(u32_as_i32(w) + [0],) for w in words]
    assert run(engine, 15, cases, lambda a: M.from_fp([x & 0xFFFFFFFF for x in a[:8]])) == len(cases)
