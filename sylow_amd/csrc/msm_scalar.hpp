// msm_scalar.hpp -- the scalar side of the bucket method (Pippenger), shared by the G1 route (msm.hip) and the G2 route (g2_msm.hpp): the
// signed-digit recoding, the histogram, the flat scan, the counting-sort scatter, and the host-side plan and scratch formula.  Nothing here
// knows the point type: a unit states the words of its bucket and of its prepared point (msm::Plan's template arguments) and whether its
// scalars are reduced mod r on top of Fp::new (MOD_R: true where every point has order r, i.e. on E(Fp); false on the twist, whose points
// need not have order r -- there the digits are those of k mod p itself).  The build has no relocatable device code, so every kernel
// is a template on MOD_R and each unit instantiates, and launches, its own copy.
// tools/msm_model.py is the host-side model of the recoding, the plan and the scratch formula.
#pragma once
#include "host.hpp"

// The including unit defines the tuning constants at file scope BEFORE the include (msm.hip and g2_msm.hpp each keep their own, next to the
// kernels they tune): MSM_SEG (entries per accumulation segment), MSM_RUN (buckets per lane in the running-sum reduction), MSM_C_MAX, SCAN_ITEMS and
// SCAN_TILE (entries per scan thread and block).
namespace msm {
// ------------------------------------------------------------------ recode ----------
// scalar i as an Fp value (Fp::new: k >= p is reduced), and with MOD_R then mod the group order (every point of E(Fp) has order r) --
// k < 2^256 straight mod r would differ for k >= p
template <bool MOD_R>
BN_DEV void msm_scalar(u32 (&k)[8], const u64* ks, size_t n, size_t i) {
  load_scalar(k, ks, n, i);
  if (MOD_R) cond_sub_const(k, 0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u);   // r (k < p < 2r)
}
// bits [bit, bit + c) of k, c <= 16 (word index through selects: no dynamically indexed register array)
BN_DEV u32 msm_bits(const u32 (&k)[8], int bit, int c) {
  const int q = bit >> 5, s = bit & 31;
  u32 lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { lo = j == q ? k[j] : lo; hi = j == q + 1 ? k[j] : hi; }
  return (u32)((((u64)hi << 32) | lo) >> s) & ((1u << c) - 1u);
}
// the signed digit of window w given the carry out of window w - 1 (in / out): d in [-2^(c-1), 2^(c-1)]; k < 2^254 and W c >= 255 leave
// no carry out of the top window
BN_DEV int msm_digit(const u32 (&k)[8], int w, int c, int& carry) {
  int d = (int)msm_bits(k, w * c, c) + carry;
  carry = d > (1 << (c - 1));
  return d - (carry << c);
}
// atomicAdd(&ctr[key], 1) for every active lane with `on`, returning the old value, with the lanes of a wavefront that share a key served by ONE
// atomic (up to AGG_ROUNDS distinct keys per wavefront; the rest one atomic per lane).  Hot buckets -- every scalar equal, scalars from {0, 1},
// the few buckets of a narrow top window -- otherwise queue 64 atomics per wavefront on one address.  Call with the whole wavefront converged.
constexpr int AGG_ROUNDS = 4;
BN_DEV u32 agg_atomic_inc(u32* ctr, u32 key, bool on) {
  u32 pos = 0;
  bool done = !on;
#pragma unroll 1
  for (int r = 0; r < AGG_ROUNDS; ++r) {
    const unsigned long long act = __ballot(!done);
    if (!act) return pos;
    const int leader = __ffsll((long long)act) - 1;
    const u32 lk = (u32)__shfl((int)key, leader);
    const bool mine = !done && key == lk;
    const unsigned long long grp = __ballot(mine);
    u32 first = 0;
    if ((int)__lane_id() == leader) first = atomicAdd(&ctr[lk], (u32)__popcll(grp));
    first = (u32)__shfl((int)first, leader);
    if (mine) {
      pos = first + __builtin_amdgcn_mbcnt_hi((u32)(grp >> 32), __builtin_amdgcn_mbcnt_lo((u32)grp, 0u));
      done = true;
    }
  }
  if (!done) pos = atomicAdd(&ctr[key], 1u);
  return pos;
}
template <bool MOD_R>
__global__ void __launch_bounds__(BLOCK) k_msm_hist(const uint8_t* pinf, const u64* ks, size_t n, size_t base, size_t nc, int c, int W, u32* cnt) {
  const size_t t = TID;
  if (t >= nc) return;
  const size_t i = base + t;
  const bool skip = pinf && pinf[i];                    // stays in the loop: agg_atomic_inc wants the wavefront converged
  u32 k[8];
  msm_scalar<MOD_R>(k, ks, n, i);
  const size_t B = (size_t)1 << (c - 1);
  int carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int d = skip ? 0 : msm_digit(k, w, c, carry);
    (void)agg_atomic_inc(cnt, (u32)((size_t)w * B + (size_t)((d < 0 ? -d : d) - 1)), d != 0);
  }
}
template <bool MOD_R>
__global__ void __launch_bounds__(BLOCK) k_msm_scatter(const uint8_t* pinf, const u64* ks, size_t n, size_t base, size_t nc, int c, int W, u32* cursor, u32* idx) {
  const size_t t = TID;
  if (t >= nc) return;
  const size_t i = base + t;
  const bool skip = pinf && pinf[i];                    // stays in the loop: agg_atomic_inc wants the wavefront converged
  u32 k[8];
  msm_scalar<MOD_R>(k, ks, n, i);
  const size_t B = (size_t)1 << (c - 1);
  int carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int d = skip ? 0 : msm_digit(k, w, c, carry);
    const u32 pos = agg_atomic_inc(cursor, (u32)((size_t)w * B + (size_t)((d < 0 ? -d : d) - 1)), d != 0);
    if (d) idx[pos] = (u32)t | (d < 0 ? 0x80000000u : 0u);
  }
}
// ------------------------------------------------------------------ scan ----------
// exclusive scan of one tile of SCAN_TILE u64 values in place; returns the tile total (thread-uniform)
BN_DEV u64 tile_exscan(u64 (&v)[SCAN_ITEMS], u64* lds) {
  const int t = threadIdx.x;
  u64 s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) { const u64 x = v[j]; v[j] = s; s += x; }
  lds[t] = s;
  __syncthreads();
  for (int off = 1; off < BLOCK; off <<= 1) {
    const u64 x = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += x;
    __syncthreads();
  }
  const u64 before = lds[t] - s, total = lds[BLOCK - 1];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) v[j] += before;
  return total;
}
// counts -> packed (segments << 32 | entries), tile-exclusive scan into off, tile totals into tops
template <bool MOD_R>
__global__ void __launch_bounds__(BLOCK) k_msm_scan_tiles(const u32* cnt, size_t N, u64* off, u64* tops) {
  __shared__ u64 lds[BLOCK];
  const size_t b0 = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
  u64 v[SCAN_ITEMS];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const u64 e = b0 + j < N ? cnt[b0 + j] : 0;
    v[j] = ((e + MSM_SEG - 1) / MSM_SEG) << 32 | e;
  }
  const u64 total = tile_exscan(v, lds);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) if (b0 + j < N) off[b0 + j] = v[j];
  if (threadIdx.x == 0) tops[blockIdx.x] = total;
}
// one block: exclusive scan of the m <= SCAN_TILE tile totals in place, grand total into *meta
template <bool MOD_R>
__global__ void __launch_bounds__(BLOCK) k_msm_scan_tops(u64* tops, size_t m, u64* meta) {
  __shared__ u64 lds[BLOCK];
  const size_t b0 = (size_t)threadIdx.x * SCAN_ITEMS;
  u64 v[SCAN_ITEMS];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) v[j] = b0 + j < m ? tops[b0 + j] : 0;
  const u64 total = tile_exscan(v, lds);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) if (b0 + j < m) tops[b0 + j] = v[j];
  if (threadIdx.x == 0) *meta = total;
}
// tile offsets in; the scatter cursors (entry offsets) out
template <bool MOD_R>
__global__ void __launch_bounds__(BLOCK) k_msm_scan_add(u64* off, size_t N, const u64* tops, u32* cursor) {
  const size_t b = TID;
  if (b >= N) return;
  const u64 o = off[b] + tops[b / SCAN_TILE];
  off[b] = o;
  cursor[b] = (u32)o;
}

// ------------------------------------------------------------------ the plan of one call ----------
// (tools/msm_model.py mirrors every formula here.)  PROJ_WORDS: i32 words of one projective accumulator (a bucket, a segment partial, a
// reduction partial, a window sum); PT_WORDS: i32 words of one prepared point.
struct Plan {
  int c, W;
  size_t B, N, R, T, nc, seg_cap, bytes;
};
// bits of a scalar < 2^254 that the top window holds: few bits = few buckets that every point of that window falls into
inline int top_bits(int c) { return 254 - c * ((255 + c - 1) / c - 1); }
// c0 = floor(log2 n) - 4 clamped to [8, 16]; of c0, c0 - 1, c0 + 1 (inside [8, 16]) the one with the widest top window, c0 on ties
// (c0 = 12 -> 13, 14 -> 15: their top windows hold 2 bits, 13's and 15's 7 and 14)
inline int default_window(size_t n) {
  int lg = 0;
  while (lg < 62 && ((size_t)2 << lg) <= n) ++lg;
  const int c0 = lg - 4 < 8 ? 8 : (lg - 4 > MSM_C_MAX ? MSM_C_MAX : lg - 4);
  int best = c0;
  for (int c : {c0 - 1, c0 + 1})
    if (c >= 8 && c <= MSM_C_MAX && top_bits(c) > top_bits(best)) best = c;
  return best;
}
inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t seg_bound(int W, size_t N, size_t nc) { const size_t e = (size_t)W * nc; return e / MSM_SEG + 1 + (N < e ? N : e); }
// bytes of the fixed part (buckets, scan, reduction) and of a chunk of nc points
template <size_t PROJ_WORDS>
inline size_t fixed_bytes(int W, size_t N, size_t T) {
  const size_t tiles = (N + SCAN_TILE - 1) / SCAN_TILE;
  return align_up(N * 4) + align_up(N * 8) + align_up(N * 4) + align_up(tiles * 8) + align_up(8) + align_up(N * PROJ_WORDS * 4) + align_up((size_t)W * T * PROJ_WORDS * 4) +
         align_up((size_t)W * PROJ_WORDS * 4);
}
template <size_t PROJ_WORDS, size_t PT_WORDS>
inline size_t chunk_bytes(int W, size_t N, size_t nc) {
  return align_up(nc * PT_WORDS * 4) + align_up((size_t)W * nc * 4) + align_up(seg_bound(W, N, nc) * PROJ_WORDS * 4);
}
// the bucket route's plan for n points under `budget` bytes; false when not even a chunk of 256 points fits
template <size_t PROJ_WORDS, size_t PT_WORDS>
inline bool plan(size_t n, int c, size_t budget, Plan& p) {
  p.c = c; p.W = (255 + c - 1) / c; p.B = (size_t)1 << (c - 1); p.N = (size_t)p.W * p.B;
  p.R = p.B < (size_t)MSM_RUN ? p.B : (size_t)MSM_RUN; p.T = p.B / p.R;
  const size_t fixed = fixed_bytes<PROJ_WORDS>(p.W, p.N, p.T);
  size_t nc = n < ((size_t)1 << 31) / (size_t)p.W ? n : ((size_t)1 << 31) / (size_t)p.W;   // chunk-local indices and entry offsets stay below 2^31
  const size_t floor_nc = n < 256 ? n : 256;
  if (fixed + chunk_bytes<PROJ_WORDS, PT_WORDS>(p.W, p.N, floor_nc) > budget) return false;
  if (fixed + chunk_bytes<PROJ_WORDS, PT_WORDS>(p.W, p.N, nc) > budget) {      // largest chunk that fits (chunk_bytes is monotone in nc)
    size_t lo = floor_nc, hi = nc;
    while (lo < hi) {
      const size_t mid = lo + (hi - lo + 1) / 2;
      if (fixed + chunk_bytes<PROJ_WORDS, PT_WORDS>(p.W, p.N, mid) <= budget) lo = mid; else hi = mid - 1;
    }
    nc = lo;
  }
  p.nc = nc;
  p.seg_cap = seg_bound(p.W, p.N, nc);
  p.bytes = fixed + chunk_bytes<PROJ_WORDS, PT_WORDS>(p.W, p.N, nc);
  return true;
}
}  // namespace msm
