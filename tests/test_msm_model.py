"""CPU: the host-side recoding and planning of sylow_hip_g1_msm (tools/msm_model.py mirrors sylow_amd/csrc/msm_bucket.hpp and the G1 policy of msm.hip)."""
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import msm_model as M  # noqa: E402

BOUNDARY = [0, 1, 2, M.R - 1, M.R, M.R + 1, M.P - 1, M.P, M.P + 1, 2 * M.R, (1 << 254) - 1, (1 << 255) + 12345, (1 << 256) - 1]


def test_reduce_scalar_is_fp_new_then_mod_r():
    assert M.reduce_scalar(M.P) == 0 and M.reduce_scalar(M.P + 5) == 5
    assert M.reduce_scalar(M.R) == 0 and M.reduce_scalar(M.P - 1) == (M.P - 1) - M.R
    k = (1 << 256) - 1
    assert M.reduce_scalar(k) == (k % M.P) % M.R != k % M.R          # straight mod r is wrong for k >= p


def test_signed_digits_reconstruct_the_scalar():
    rng = random.Random(20261015)
    scalars = [M.reduce_scalar(k) for k in BOUNDARY] + [rng.randrange(M.R) for _ in range(300)]
    scalars += [(1 << M.C_MAX * j) - 1 for j in range(1, 16)] + [M.R - 1 - (1 << j) for j in range(0, 250, 7)]
    for c in range(M.C_MIN, M.C_MAX + 1):
        half = 1 << (c - 1)
        for k in scalars:
            d = M.recode(k, c)
            assert len(d) == M.windows(c)
            assert all(-half <= x <= half for x in d), (c, k)
            assert sum(x << (c * w) for w, x in enumerate(d)) == k, (c, k)


def test_window_and_bucket_counts():
    want = {4: 64, 5: 51, 6: 43, 7: 37, 8: 32, 9: 29, 10: 26, 11: 24, 12: 22, 13: 20, 14: 19, 15: 17, 16: 16}
    for c, W in want.items():
        assert M.windows(c) == W and W * c >= 255 and (W - 1) * c < 255
        assert M.buckets(c) == 1 << (c - 1)
        assert M.additions_per_point(c) == W
    assert [M.default_window(1 << lg) for lg in (10, 12, 14, 16, 18, 20, 22)] == [8, 8, 10, 13, 15, 16, 16]
    assert M.default_window((1 << 20) - 1) == 15 and M.default_window(1 << 15) == 10
    # no default leaves a top window of fewer than 4 bits (a handful of buckets that every point of the window falls into)
    assert {c: M.top_bits(c) for c in range(8, 17)} == {8: 6, 9: 2, 10: 4, 11: 1, 12: 2, 13: 7, 14: 2, 15: 14, 16: 14}
    assert min(M.top_bits(M.default_window(1 << lg)) for lg in range(1, 40)) >= 4


def test_scratch_formula_and_plan():
    c = 16
    W, N = M.windows(c), M.windows(c) * M.buckets(c)
    # the per-point cost: F29 x, y in an 80-byte record + one 4-byte entry per window + one 108-byte partial per MSM_SEG entries (+ per bucket)
    nc = 1 << 20
    assert M.chunk_bytes(c, nc) == M._align(nc * 80) + M._align(W * nc * 4) + M._align((W * nc // 32 + 1 + N) * 108)
    assert M.scratch_bytes(c, nc) == M.fixed_bytes(c) + M.chunk_bytes(c, nc)
    assert 300 << 20 < M.scratch_bytes(c, nc) < 340 << 20
    # the default budget takes 2^20 points in one chunk; a small budget splits them, a tiny one leaves the bucket route
    assert M.plan(nc, c) == (nc, M.scratch_bytes(c, nc))
    n = 1 << 16
    c = M.default_window(n)
    budget = M.fixed_bytes(c) + M.chunk_bytes(c, n // 5)
    chunk, b = M.plan(n, c, budget)
    assert b <= budget < M.scratch_bytes(c, chunk + 1) and n // 5 <= chunk < n // 4
    assert M.plan(n, c, M.fixed_bytes(c)) is None
    for n in (1, 3, 255, 256, 1000):
        assert M.plan(n, 8) == (n, M.scratch_bytes(8, n))


def test_model_constants_match_the_kernel_unit():
    csrc = os.path.join(ROOT, "sylow_amd", "csrc")
    const = dict(re.findall(r"constexpr (?:int|size_t|bool) (\w+) = ([^,;]+)[,;]", open(os.path.join(csrc, "msm_bucket.hpp")).read()))
    assert int(const["MSM_SEG"]) == M.MSM_SEG and int(const["MSM_RUN"]) == M.MSM_RUN
    assert int(const["MSM_C_MIN"]) == M.C_MIN and int(const["MSM_C_MAX"]) == M.C_MAX
    assert const["MSM_DEFAULT_BUDGET"].strip() == "(size_t)1 << 30" and M.DEFAULT_BUDGET == 1 << 30
    # the G1 policy: one lane per point, so a bucket is LANES * 27 words and a prepared point LANES * 20; scalars reduced mod r
    g1 = dict(re.findall(r"constexpr (?:int|size_t|bool) (\w+) = ([^,;]+)[,;]", open(os.path.join(csrc, "msm.hip")).read()))
    assert g1["DEFAULT_MIN"].strip() == "(size_t)1 << 18" and M.DEFAULT_MIN == 1 << 18
    assert int(g1["LANES"]) == 1 and g1["MOD_R"].strip() == "true"
    assert int(g1["LANES"]) * int(const["PROJ_LANE_WORDS"]) == M.W27 and int(g1["LANES"]) * int(const["PT_LANE_WORDS"]) == M.PT_WORDS
    assert "PROJ_WORDS = PROJ_LANE_WORDS * G::LANES" in open(os.path.join(csrc, "msm_bucket.hpp")).read()
