"""CPU: the host-side recoding and planning of sylow_hip_g2_msm (the g2_* functions of tools/msm_model.py mirror sylow_amd/csrc/msm_bucket.hpp under
the lane-pair policy of g2_msm.hpp, MOD_R = false).  The one place where G2 is not a copy of G1: the digits are those of k mod p itself."""
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import msm_model as M  # noqa: E402

BOUNDARY = [0, 1, 2, M.R - 1, M.R, M.R + 1, 2 * M.R, M.P - 1, M.P, M.P + 1, (1 << 254) - 1, (1 << 255) - 1, (1 << 256) - 1, 3 * M.P + 7]


def test_the_g2_scalar_is_fp_new_and_nothing_else():
    assert M.g2_reduce_scalar(M.P) == 0 and M.g2_reduce_scalar(M.P + 5) == 5 and M.g2_reduce_scalar(3 * M.P + 7) == 7
    # no mod-r step: r, r + 1, 2r and p - 1 stay what they are (a twist point of order 10069 sees them as r mod 10069, ...), where G1 folds them
    for k in (M.R - 1, M.R, M.R + 1, M.P - 1):
        assert M.g2_reduce_scalar(k) == k
    assert M.g2_reduce_scalar(2 * M.R) == 2 * M.R - M.P
    assert M.g2_reduce_scalar(M.R) != M.reduce_scalar(M.R) == 0
    assert M.R % 10069 != 0 and M.g2_reduce_scalar(M.R) % 10069 != 0
    assert M.g2_reduce_scalar((1 << 256) - 1) == ((1 << 256) - 1) % M.P


def test_g2_digits_are_those_of_k_mod_p():
    rng = random.Random(20261017)
    scalars = BOUNDARY + [rng.randrange(1 << 256) for _ in range(300)] + [M.P - 1 - (1 << j) for j in range(0, 253, 7)]
    for c in range(M.C_MIN, M.C_MAX + 1):
        half = 1 << (c - 1)
        for k in scalars:
            d = M.g2_recode(k, c)
            assert len(d) == M.windows(c)
            assert all(-half <= x <= half for x in d), (c, k)
            assert sum(x << (c * w) for w, x in enumerate(d)) == k % M.P, (c, k)


def test_no_carry_out_of_the_top_window_for_p_minus_1():
    """k mod p <= p - 1 < 2^254 and W c >= 255: recode() asserts that the carry out of the top window is zero; the top digit stays positive"""
    assert M.P < 1 << 254
    for c in range(M.C_MIN, M.C_MAX + 1):
        for k in (M.P - 1, M.P - 2, M.P - 1 - (1 << 200)):
            d = M.g2_recode(k, c)
            assert sum(x << (c * w) for w, x in enumerate(d)) == k
            assert 0 <= d[-1] <= 1 << (c - 1), (c, d[-1])
        # the largest value the top window can see: every lower window carries
        top = (M.P - 1) >> (c * (M.windows(c) - 1))
        assert top + 1 <= 1 << (c - 1), c


def test_g2_scratch_formula_and_plan():
    c = 16
    W, N = M.windows(c), M.windows(c) * M.buckets(c)
    nc = 1 << 20
    # per point: a record of 2 x 80 bytes + one 4-byte entry per window + one 216-byte partial per MSM_SEG entries (+ per bucket)
    assert M.g2_chunk_bytes(c, nc) == M._align(nc * 160) + M._align(W * nc * 4) + M._align((W * nc // 32 + 1 + N) * 216)
    assert M.g2_scratch_bytes(c, nc) == M.g2_fixed_bytes(c) + M.g2_chunk_bytes(c, nc)
    assert M.g2_scratch_bytes(c, nc) > M.scratch_bytes(c, nc)
    assert M.g2_plan(nc, c) == (nc, M.g2_scratch_bytes(c, nc))
    n = 4097
    for c in range(M.C_MIN, M.C_MAX + 1):
        for parts in (2, 7):
            budget = M.g2_scratch_bytes(c, n // parts)
            chunk, b = M.g2_plan(n, c, budget)
            assert n // parts <= chunk < n and b <= budget
            assert M.g2_scratch_bytes(c, chunk + 1) > budget or chunk + 1 > n
        assert M.g2_plan(n, c, M.g2_fixed_bytes(c)) is None
        assert M.g2_plan(0, c) == (0, M.g2_scratch_bytes(c, 0))


def test_g2_plan_and_scratch_are_monotone_in_the_chunk_size():
    for c in range(M.C_MIN, M.C_MAX + 1):
        sizes = [0, 1, 2, 31, 32, 33, 255, 256, 257, 1000, 4097, 1 << 16, (1 << 16) + 1, 1 << 20, 1 << 24]
        b = [M.g2_scratch_bytes(c, nc) for nc in sizes]
        assert all(x <= y for x, y in zip(b, b[1:])), c
        assert all(M.g2_chunk_bytes(c, nc) <= M.g2_chunk_bytes(c, nc + 1) for nc in range(0, 600)), c
        # a larger budget never plans a smaller chunk
        n = 1 << 18
        budgets = [M.g2_scratch_bytes(c, n // d) for d in (64, 16, 7, 3, 2, 1)]
        chunks = [M.g2_plan(n, c, bud)[0] for bud in budgets]
        assert chunks == sorted(chunks) and chunks[-1] == n, c


def test_the_model_mirrors_the_sources():
    csrc = os.path.join(ROOT, "sylow_amd", "csrc")
    src, shared = open(os.path.join(csrc, "g2_msm.hpp")).read(), open(os.path.join(csrc, "msm_bucket.hpp")).read()
    num = lambda name, text: int(re.search(r"\b" + name + r" = (?:\(size_t\))?(\d+)", text).group(1))
    # a lane pair per point: a bucket is LANES * 27 words, a prepared point LANES * 20
    assert num("LANES", src) == 2 and "PROJ_WORDS = PROJ_LANE_WORDS * G::LANES" in shared and "PT_WORDS = PT_LANE_WORDS * G::LANES" in shared
    assert num("LANES", src) * num("PROJ_LANE_WORDS", shared) == M.W54 and num("LANES", src) * num("PT_LANE_WORDS", shared) == M.G2_PT_WORDS
    assert num("MSM_SEG", shared) == M.MSM_SEG and num("MSM_RUN", shared) == M.MSM_RUN
    assert int(re.search(r"\bDEFAULT_MIN = \(size_t\)1 << (\d+)", src).group(1)) == M.G2_DEFAULT_MIN.bit_length() - 1
    assert num("WIDE_C", src) == M.G2_WIDE_C and int(re.search(r"\bWIDE_FROM = \(size_t\)1 << (\d+)", src).group(1)) == 16
    assert "return n >= WIDE_FROM ? WIDE_C : msm::default_window(n);" in src
    assert [M.g2_default_window(1 << lg) for lg in (10, 12, 14, 15, 16, 17, 18, 20, 24)] == [8, 8, 10, 10, 15, 15, 15, 15, 15]
    assert M.g2_default_window((1 << 16) - 1) == M.default_window((1 << 16) - 1) == 10
    assert re.search(r"\bMOD_R = false;", src)                                    # the digits of k mod p: no mod-r step on the twist
    assert "if (G::MOD_R) cond_sub_const" in shared and "msm_scalar<G>(k, ks, n, i);" in shared
    g1 = open(os.path.join(csrc, "msm.hip")).read()
    assert re.search(r"\bMOD_R = true;", g1) and "msm::tuned<msmh::G1Lane>" in g1 and "msm::tuned<plk::G2Pair>" in src
