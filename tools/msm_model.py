"""Model of the host-side recoding and planning of sylow_hip_g1_msm (sylow_amd/csrc/msm_bucket.hpp under the one-lane policy of msm.hip):
the signed c-bit digits of a scalar, the window / bucket counts, the chunk plan under a scratch budget and the scratch-byte formula.  Every
formula here mirrors the C++ one by one; tests/test_msm_model.py pins them, and tests/test_gpu_msm.py uses scratch_bytes to force chunking.
The g2_* functions are the same model for sylow_hip_g2_msm (the same header under the lane-pair policy of g2_msm.hpp): the digits are those
of k mod p itself (a twist point need not have order r), and a bucket and a prepared point are twice as wide (lane pairs);
tests/test_g2_msm_model.py pins them.

    python tools/msm_model.py            # prints the plan for n = 2^12 .. 2^24"""
import json
import sys

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001

MSM_SEG = 32          # entries per accumulation segment
MSM_RUN = 16          # buckets per lane in the running-sum reduction
C_MIN, C_MAX = 4, 16
SCAN_TILE = 1024
DEFAULT_BUDGET = 1 << 30
DEFAULT_MIN = 1 << 18
W27 = 27              # i32 words of a projective carry-free point
PT_WORDS = 20         # i32 words of a prepared affine point (x, y, padding to 80 bytes)


def reduce_scalar(k: int) -> int:
    """(k mod p) mod r: Fp::new first (k >= p as in the reference's Mul<&Fp>), then the group order."""
    return (k % P) % R


def windows(c: int) -> int:
    """W c >= 255 > log2(r) + 1: the carry out of the top window is always zero."""
    return -(-255 // c)


def buckets(c: int) -> int:
    return 1 << (c - 1)


def recode(k: int, c: int) -> list:
    """signed digits d_w in [-2^(c-1), 2^(c-1)] with sum d_w 2^(c w) = k (k < 2^254)"""
    assert 0 <= k < 1 << 254
    digits, carry = [], 0
    for w in range(windows(c)):
        d = ((k >> (w * c)) & ((1 << c) - 1)) + carry
        carry = 1 if d > 1 << (c - 1) else 0
        digits.append(d - (carry << c))
    assert carry == 0
    return digits


def top_bits(c: int) -> int:
    """bits of a scalar < 2^254 that the top window holds"""
    return 254 - c * (windows(c) - 1)


def default_window(n: int) -> int:
    """c0 = floor(log2 n) - 4 clamped to [8, 16]; of c0, c0 - 1, c0 + 1 (inside [8, 16]) the one with the widest top window, c0 on ties"""
    lg = max(n, 1).bit_length() - 1
    best = c0 = min(max(lg - 4, 8), C_MAX)
    for c in (c0 - 1, c0 + 1):
        if 8 <= c <= C_MAX and top_bits(c) > top_bits(best):
            best = c
    return best


def additions_per_point(c: int) -> int:
    """group additions a point costs in the accumulation (one per non-zero digit, at most one per window)"""
    return windows(c)


def _align(x: int) -> int:
    return (x + 255) & ~255


def seg_bound(W: int, N: int, nc: int) -> int:
    e = W * nc
    return e // MSM_SEG + 1 + min(N, e)


def fixed_bytes(c: int) -> int:
    W, B = windows(c), buckets(c)
    N, T = W * B, B // min(B, MSM_RUN)
    tiles = -(-N // SCAN_TILE)
    return (_align(N * 4) + _align(N * 8) + _align(N * 4) + _align(tiles * 8) + _align(8) + _align(N * W27 * 4) + _align(W * T * W27 * 4) +
            _align(W * W27 * 4))


def chunk_bytes(c: int, nc: int) -> int:
    W, N = windows(c), windows(c) * buckets(c)
    return _align(nc * PT_WORDS * 4) + _align(W * nc * 4) + _align(seg_bound(W, N, nc) * W27 * 4)


def scratch_bytes(c: int, nc: int) -> int:
    """the one lease of a call whose chunks hold nc points"""
    return fixed_bytes(c) + chunk_bytes(c, nc)


def plan(n: int, c: int, budget: int = DEFAULT_BUDGET):
    """(chunk size, lease bytes) of the bucket route, or None when not even a chunk of min(n, 256) points fits (small-n route)"""
    W = windows(c)
    nc = min(n, (1 << 31) // W)
    floor_nc = min(n, 256)
    if scratch_bytes(c, floor_nc) > budget:
        return None
    if scratch_bytes(c, nc) > budget:
        lo, hi = floor_nc, nc
        while lo < hi:
            mid = lo + (hi - lo + 1) // 2
            if scratch_bytes(c, mid) <= budget:
                lo = mid
            else:
                hi = mid - 1
        nc = lo
    return nc, scratch_bytes(c, nc)


# ---- G2 (the lane-pair policy of g2_msm.hpp): the same scalar side without the mod-r step, the same plan with lane-pair sizes ----
G2_DEFAULT_MIN = 1 << 16
G2_WIDE_FROM, G2_WIDE_C = 1 << 16, 15   # from this n on the default window is G2_WIDE_C (measured: DESIGN.md §4.3)
W54 = 54              # i32 words of a projective lane-pair point: 27 per lane
G2_PT_WORDS = 40      # i32 words of a prepared affine point: per lane x, y, padding to 80 bytes


def g2_reduce_scalar(k: int) -> int:
    """k mod p and nothing else: Fp::new.  The product is exact on the whole twist, whose points need not have order r."""
    return k % P


def g2_default_window(n: int) -> int:
    """the G1 rule below 2^16, c = 15 from there on (the sweep of c at 2^16 and 2^20 has it fastest at both)"""
    return G2_WIDE_C if n >= G2_WIDE_FROM else default_window(n)


def g2_recode(k: int, c: int) -> list:
    """the signed c-bit digits of k mod p: k mod p < 2^254 and W c >= 255 leave no carry out of the top window"""
    return recode(g2_reduce_scalar(k), c)


def g2_fixed_bytes(c: int) -> int:
    W, B = windows(c), buckets(c)
    N, T = W * B, B // min(B, MSM_RUN)
    tiles = -(-N // SCAN_TILE)
    return (_align(N * 4) + _align(N * 8) + _align(N * 4) + _align(tiles * 8) + _align(8) + _align(N * W54 * 4) + _align(W * T * W54 * 4) +
            _align(W * W54 * 4))


def g2_chunk_bytes(c: int, nc: int) -> int:
    W, N = windows(c), windows(c) * buckets(c)
    return _align(nc * G2_PT_WORDS * 4) + _align(W * nc * 4) + _align(seg_bound(W, N, nc) * W54 * 4)


def g2_scratch_bytes(c: int, nc: int) -> int:
    """the one lease of a G2 call whose chunks hold nc points"""
    return g2_fixed_bytes(c) + g2_chunk_bytes(c, nc)


def g2_plan(n: int, c: int, budget: int = DEFAULT_BUDGET):
    """(chunk size, lease bytes) of the G2 bucket route, or None when not even a chunk of min(n, 256) points fits (composed route)"""
    W = windows(c)
    nc = min(n, (1 << 31) // W)
    floor_nc = min(n, 256)
    if g2_scratch_bytes(c, floor_nc) > budget:
        return None
    if g2_scratch_bytes(c, nc) > budget:
        lo, hi = floor_nc, nc
        while lo < hi:
            mid = lo + (hi - lo + 1) // 2
            if g2_scratch_bytes(c, mid) <= budget:
                lo = mid
            else:
                hi = mid - 1
        nc = lo
    return nc, g2_scratch_bytes(c, nc)


if __name__ == "__main__":
    rows = []
    for lg in range(12, 25, 2):
        n = 1 << lg
        c = default_window(n)
        nc, b = plan(n, c)
        rows.append({"n": n, "c": c, "windows": windows(c), "buckets": buckets(c), "adds_per_point": additions_per_point(c),
                     "chunk": nc, "chunks": -(-n // nc), "scratch_MB": round(b / 2**20, 1)})
    json.dump(rows, sys.stdout, indent=1)
    print()
