// msm.hip -- one large G1 multi-scalar multiplication Q = sum_i k_i P_i by the bucket method (Pippenger), on the carry-free core.
//
// Per chunk of points (one chunk unless the scratch budget is short; every chunk adds into the same buckets):
//   k_msm_prep       affine SoA -> carry-free (F29) x, y once per point, so that the W additions of a point convert nothing; one 80-byte
//                    record per point (x, y, 2 words of padding): a random gather is five 16-byte loads from two cache lines, not 18
//                    4-byte loads from 18 rows of an SoA array
//   k_msm_hist       scalar -> (k mod p) mod r -> W signed c-bit digits in [-2^(c-1), 2^(c-1)]; count[w][|d| - 1] += 1 (zero digits drop out)
//   k_msm_scan_*     ONE flat exclusive scan over all W * 2^(c-1) buckets of (segments << 32 | entries), segments = ceil(entries / MSM_SEG)
//   k_msm_scatter    the same digits again: index | sign << 31 into the bucket's slot range (a counting sort; order inside a bucket is free)
//   k_msm_seg        one lane per segment of <= MSM_SEG entries of one bucket: the complete addition (proj_add_lazy) with Z = 1 operands, in
//                    registers; a bucket of one segment adds straight into its bucket, longer buckets leave one partial per segment
//   k_msm_seg_join   one lane per bucket of 2 .. JOIN_LANE_MAX segments: bucket += its partials
//   k_msm_seg_join_wide  one BLOCK per bucket of more segments: the partials split over 256 threads, then a tree in LDS -- a hot bucket (all
//                    scalars equal, scalars from {0, 1}, the narrow top window) costs ns / 256 + 8 dependent additions, not ns
// Then once:
//   k_msm_bucket_reduce  running sums sum_m m B_m over MSM_RUN contiguous buckets per lane, corrected by (offset) x (range sum)
//   k_msm_window_sum     one block per window: the lanes' partials -> S_w
//   k_msm_combine        Horner over the windows (c doublings + one addition each), then affine
// tools/msm_model.py is the host-side model of the recoding, the plan and the scratch formula (tests/test_msm_model.py).
#include "host.hpp"

namespace {
constexpr int MSM_SEG = 32;            // entries per accumulation segment
constexpr u32 JOIN_LANE_MAX = 8;       // segments a bucket may have to be joined by one lane; more go to k_msm_seg_join_wide
constexpr int MSM_RUN = 16;            // buckets per lane in the running-sum reduction
constexpr int MSM_C_MIN = 4;           // window widths sylow_hip_g1_msm_tuned accepts
constexpr int MSM_C_MAX = 16;
constexpr int SCAN_ITEMS = 4, SCAN_TILE = BLOCK * SCAN_ITEMS;   // 1024 entries per scan block
constexpr size_t MSM_DEFAULT_BUDGET = (size_t)1 << 30;
constexpr size_t MSM_DEFAULT_MIN = (size_t)1 << 18;    // the smallest measured size the bucket route wins: 2^18 1.6 x, 2^17 0.28 x
constexpr size_t W27 = 27;             // words (i32) of a projective F29 point
constexpr size_t PT_WORDS = 20;        // words (i32) of a prepared affine point: x, y, padding to 80 bytes
}  // namespace

// ------------------------------------------------------------------ F29 point SoA --------------
BN_DEV F29 ld9(const i32* a, size_t stride, size_t i, int w0) {
  F29 r;
#pragma unroll
  for (int q = 0; q < 9; ++q) r.v[q] = a[(size_t)(w0 + q) * stride + i];
  return r;
}
BN_DEV void st9(i32* a, size_t stride, size_t i, int w0, const F29& x) {
#pragma unroll
  for (int q = 0; q < 9; ++q) a[(size_t)(w0 + q) * stride + i] = x.v[q];
}
BN_DEV G1W ldp(const i32* a, size_t stride, size_t i) { return G1W{ld9(a, stride, i, 0), ld9(a, stride, i, 9), ld9(a, stride, i, 18)}; }
BN_DEV void stp(i32* a, size_t stride, size_t i, const G1W& p) { st9(a, stride, i, 0, p.x); st9(a, stride, i, 9, p.y); st9(a, stride, i, 18, p.z); }
BN_DEV G1W msm_add(const G1W& a, const G1W& b) { return proj_add_lazy<OpsF29I>(a, b); }
BN_DEV G1W msm_dbl(const G1W& a) { return proj_double_lazy<OpsF29I>(a); }

// ------------------------------------------------------------------ recode ----------
// scalar i as (k mod p) mod r: Fp::new, then the group order (every point of E(Fp) has order r) -- k < 2^256 straight mod r would differ for k >= p
BN_DEV void msm_scalar(u32 (&k)[8], const u64* ks, size_t n, size_t i) {
  load_scalar(k, ks, n, i);
  cond_sub_const(k, 0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u);   // r (k < p < 2r)
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

__global__ void __launch_bounds__(BLOCK) k_msm_prep(const u64* pxy, size_t n, size_t base, size_t nc, int4* pts) {
  const size_t t = TID;
  if (t >= nc) return;
  const size_t i = base + t;
  const F29 x = f29_from_fp_reduced(load_fp(pxy, n, i, 0)), y = f29_from_fp_reduced(load_fp(pxy, n, i, 4));
  int4* d = pts + t * (PT_WORDS / 4);
  d[0] = make_int4(x.v[0], x.v[1], x.v[2], x.v[3]);
  d[1] = make_int4(x.v[4], x.v[5], x.v[6], x.v[7]);
  d[2] = make_int4(x.v[8], y.v[0], y.v[1], y.v[2]);
  d[3] = make_int4(y.v[3], y.v[4], y.v[5], y.v[6]);
  d[4] = make_int4(y.v[7], y.v[8], 0, 0);
}
// prepared point t as (x : +-y : 1)
BN_DEV G1W msm_point(const int4* __restrict__ pts, u32 t, bool neg) {
  const int4* s = pts + (size_t)t * (PT_WORDS / 4);
  const int4 a = s[0], b = s[1], c = s[2], d = s[3], e = s[4];
  G1W p{F29{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x}}, F29{{c.y, c.z, c.w, d.x, d.y, d.z, d.w, e.x, e.y}}, OpsF29::one()};
  if (neg) p.y = OpsF29::neg(p.y);
  return p;
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
__global__ void __launch_bounds__(BLOCK) k_msm_hist(const uint8_t* pinf, const u64* ks, size_t n, size_t base, size_t nc, int c, int W, u32* cnt) {
  const size_t t = TID;
  if (t >= nc) return;
  const size_t i = base + t;
  const bool skip = pinf && pinf[i];                    // stays in the loop: agg_atomic_inc wants the wavefront converged
  u32 k[8];
  msm_scalar(k, ks, n, i);
  const size_t B = (size_t)1 << (c - 1);
  int carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int d = skip ? 0 : msm_digit(k, w, c, carry);
    (void)agg_atomic_inc(cnt, (u32)((size_t)w * B + (size_t)((d < 0 ? -d : d) - 1)), d != 0);
  }
}
__global__ void __launch_bounds__(BLOCK) k_msm_scatter(const uint8_t* pinf, const u64* ks, size_t n, size_t base, size_t nc, int c, int W, u32* cursor, u32* idx) {
  const size_t t = TID;
  if (t >= nc) return;
  const size_t i = base + t;
  const bool skip = pinf && pinf[i];                    // stays in the loop: agg_atomic_inc wants the wavefront converged
  u32 k[8];
  msm_scalar(k, ks, n, i);
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
__global__ void __launch_bounds__(BLOCK) k_msm_scan_add(u64* off, size_t N, const u64* tops, u32* cursor) {
  const size_t b = TID;
  if (b >= N) return;
  const u64 o = off[b] + tops[b / SCAN_TILE];
  off[b] = o;
  cursor[b] = (u32)o;
}

// ------------------------------------------------------------------ bucket accumulation ----------
__global__ void __launch_bounds__(BLOCK) k_msm_bucket_init(i32* bk, size_t N) {
  const size_t b = TID;
  if (b >= N) return;
  stp(bk, N, b, proj_zero<OpsF29>());
}
// lane s = segment s of the flat segment order: its bucket is the last b with seg_off(b) <= s (empty buckets share the next one's offset)
__global__ void HEAVY_BOUNDS k_msm_seg(const u64* off, const u32* cnt, size_t N, const u64* meta, size_t seg_cap, const u32* idx, const int4* pts,
                                       i32* bk, i32* part) {
  const size_t s = TID;
  const u64 total = *meta;
  if (s >= (total >> 32) || s >= seg_cap) return;
  size_t lo = 0, hi = N - 1;                            // seg_off(0) = 0 <= s
  while (lo < hi) {
    const size_t mid = (lo + hi + 1) / 2;
    if ((off[mid] >> 32) <= s) lo = mid; else hi = mid - 1;
  }
  const size_t b = lo;
  const u64 o = off[b];
  const u32 e = cnt[b];
  const u32 j = (u32)(s - (o >> 32));
  const u32 first = (u32)o + j * MSM_SEG, last = min((u32)o + e, first + MSM_SEG);
  G1W acc = msm_point(pts, idx[first] & 0x7fffffffu, idx[first] >> 31);
#pragma unroll 1
  for (u32 q = first + 1; q < last; ++q) {
    const u32 u = idx[q];
    acc = msm_add(acc, msm_point(pts, u & 0x7fffffffu, u >> 31));
  }
  if (e <= MSM_SEG) stp(bk, N, b, msm_add(ldp(bk, N, b), acc));   // the bucket's only segment: this lane owns it
  else stp(part, seg_cap, s, acc);
}
__global__ void HEAVY_BOUNDS k_msm_seg_join(const u64* off, const u32* cnt, size_t N, size_t seg_cap, i32* bk, const i32* part) {
  const size_t b = TID;
  if (b >= N) return;
  const u32 e = cnt[b];
  if (e <= MSM_SEG || e > JOIN_LANE_MAX * MSM_SEG) return;
  const size_t s0 = (size_t)(off[b] >> 32), ns = (e + MSM_SEG - 1) / MSM_SEG;
  G1W acc = ldp(bk, N, b);
#pragma unroll 1
  for (size_t j = 0; j < ns; ++j) acc = msm_add(acc, ldp(part, seg_cap, s0 + j));
  stp(bk, N, b, acc);
}
// the BLOCK threads' points -> their sum, returned to every thread (a level per barrier; lds: W27 * BLOCK words, free again on return)
BN_DEV G1W block_sum(const G1W& mine, i32* lds) {
  const int t = threadIdx.x;
  stp(lds, BLOCK, t, mine);
  __syncthreads();
  for (int h = BLOCK / 2; h > 0; h >>= 1) {
    if (t < h) stp(lds, BLOCK, t, msm_add(ldp(lds, BLOCK, t), ldp(lds, BLOCK, t + h)));
    __syncthreads();
  }
  const G1W r = ldp(lds, BLOCK, 0);
  __syncthreads();
  return r;
}
// blocks stride over tiles of BLOCK buckets; each collects its tile's buckets of > JOIN_LANE_MAX segments and joins them one after the other,
// every one with all BLOCK threads
__global__ void __launch_bounds__(BLOCK) k_msm_seg_join_wide(const u64* off, const u32* cnt, size_t N, size_t seg_cap, i32* bk, const i32* part) {
  __shared__ i32 lds[W27 * BLOCK];
  __shared__ u32 heavy[BLOCK];
  __shared__ u32 n_heavy;
  const int t = threadIdx.x;
  for (size_t base = (size_t)blockIdx.x * BLOCK; base < N; base += (size_t)gridDim.x * BLOCK) {
    if (t == 0) n_heavy = 0;
    __syncthreads();
    if (base + t < N && cnt[base + t] > JOIN_LANE_MAX * MSM_SEG) heavy[atomicAdd(&n_heavy, 1u)] = (u32)t;
    __syncthreads();
    const u32 m = n_heavy;
    for (u32 h = 0; h < m; ++h) {
      const size_t b = base + heavy[h];
      const size_t s0 = (size_t)(off[b] >> 32), ns = (cnt[b] + MSM_SEG - 1) / MSM_SEG;
      G1W acc = proj_zero<OpsF29>();
#pragma unroll 1
      for (size_t j = t; j < ns; j += BLOCK) acc = msm_add(acc, ldp(part, seg_cap, s0 + j));
      acc = block_sum(acc, lds);
      if (t == 0) stp(bk, N, b, msm_add(ldp(bk, N, b), acc));
    }
    __syncthreads();                                    // every thread has read n_heavy before it is reset
  }
}

// ------------------------------------------------------------------ window reduction and combination ----------
// lane (w, t): buckets t R .. t R + R - 1 of window w (magnitudes t R + 1 .. t R + R).  Running sums from the top give sum_j (j + 1) B_j;
// adding t R times the range sum makes it sum_m m B_m.  Partial -> red[w T + t].
__global__ void HEAVY_BOUNDS k_msm_bucket_reduce(const i32* bk, size_t N, int W, size_t B, size_t R, i32* red) {
  const size_t T = B / R, g = TID;
  if (g >= (size_t)W * T) return;
  const size_t w = g / T, t = g % T, base = w * B + t * R;
  G1W run = proj_zero<OpsF29>(), acc = proj_zero<OpsF29>();
#pragma unroll 1
  for (size_t j = R; j-- > 0;) {
    run = msm_add(run, ldp(bk, N, base + j));
    acc = msm_add(acc, run);
  }
  const u32 m = (u32)(t * R);                           // < 2^15
  if (m) {
    G1W q = proj_zero<OpsF29>();
#pragma unroll 1
    for (int bit = 31 - __builtin_clz(m); bit >= 0; --bit) {
      q = msm_dbl(q);
      if ((m >> bit) & 1u) q = msm_add(q, run);
    }
    acc = msm_add(acc, q);
  }
  stp(red, (size_t)W * T, g, acc);
}
// block w: S_w = sum of the T partials of window w (serial per thread, then a tree in LDS)
__global__ void __launch_bounds__(BLOCK) k_msm_window_sum(const i32* red, int W, size_t T, i32* win) {
  __shared__ i32 lds[W27 * BLOCK];
  const size_t w = blockIdx.x, t = threadIdx.x, stride = (size_t)W * T;
  G1W acc = proj_zero<OpsF29>();
#pragma unroll 1
  for (size_t j = t; j < T; j += BLOCK) acc = msm_add(acc, ldp(red, stride, w * T + j));
  acc = block_sum(acc, lds);
  if (t == 0) stp(win, (size_t)W, w, acc);
}
__global__ void __launch_bounds__(64) k_msm_combine(const i32* win, int W, int c, u64* oxy, uint8_t* oinf) {
  if (threadIdx.x != 0) return;
  G1W acc = ldp(win, (size_t)W, (size_t)W - 1);
#pragma unroll 1
  for (int w = W - 2; w >= 0; --w) {
#pragma unroll 1
    for (int j = 0; j < c; ++j) acc = msm_dbl(acc);
    acc = msm_add(acc, ldp(win, (size_t)W, (size_t)w));
  }
  Fp x, y; bool inf;
  g1_to_affine(x, y, inf, G1P{f29_to_fp(acc.x), f29_to_fp(acc.y), f29_to_fp(acc.z)});
  store_fp(oxy, 1, 0, 0, x); store_fp(oxy, 1, 0, 4, y);
  oinf[0] = inf ? 1 : 0;
}

// ================================================================== host ======================
namespace {
// the plan of one call (tools/msm_model.py mirrors every formula here)
struct Plan {
  int c, W;
  size_t B, N, R, T, nc, seg_cap, bytes;
};
// bits of a scalar < 2^254 that the top window holds: few bits = few buckets that every point of that window falls into
int top_bits(int c) { return 254 - c * ((255 + c - 1) / c - 1); }
// c0 = floor(log2 n) - 4 clamped to [8, 16]; of c0, c0 - 1, c0 + 1 (inside [8, 16]) the one with the widest top window, c0 on ties
// (c0 = 12 -> 13, 14 -> 15: their top windows hold 2 bits, 13's and 15's 7 and 14)
int default_window(size_t n) {
  int lg = 0;
  while (lg < 62 && ((size_t)2 << lg) <= n) ++lg;
  const int c0 = lg - 4 < 8 ? 8 : (lg - 4 > MSM_C_MAX ? MSM_C_MAX : lg - 4);
  int best = c0;
  for (int c : {c0 - 1, c0 + 1})
    if (c >= 8 && c <= MSM_C_MAX && top_bits(c) > top_bits(best)) best = c;
  return best;
}
size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
size_t seg_bound(int W, size_t N, size_t nc) { const size_t e = (size_t)W * nc; return e / MSM_SEG + 1 + (N < e ? N : e); }
// bytes of the fixed part (buckets, scan, reduction) and of a chunk of nc points
size_t fixed_bytes(int W, size_t N, size_t T) {
  const size_t tiles = (N + SCAN_TILE - 1) / SCAN_TILE;
  return align_up(N * 4) + align_up(N * 8) + align_up(N * 4) + align_up(tiles * 8) + align_up(8) + align_up(N * W27 * 4) + align_up((size_t)W * T * W27 * 4) +
         align_up((size_t)W * W27 * 4);
}
size_t chunk_bytes(int W, size_t N, size_t nc) {
  return align_up(nc * PT_WORDS * 4) + align_up((size_t)W * nc * 4) + align_up(seg_bound(W, N, nc) * W27 * 4);
}
}  // namespace

namespace msmh {
// the bucket route's plan for n points under `budget` bytes; false when not even a chunk of 256 points fits
bool plan(size_t n, int c, size_t budget, Plan& p) {
  p.c = c; p.W = (255 + c - 1) / c; p.B = (size_t)1 << (c - 1); p.N = (size_t)p.W * p.B;
  p.R = p.B < (size_t)MSM_RUN ? p.B : (size_t)MSM_RUN; p.T = p.B / p.R;
  const size_t fixed = fixed_bytes(p.W, p.N, p.T);
  size_t nc = n < ((size_t)1 << 31) / (size_t)p.W ? n : ((size_t)1 << 31) / (size_t)p.W;   // chunk-local indices and entry offsets stay below 2^31
  const size_t floor_nc = n < 256 ? n : 256;
  if (fixed + chunk_bytes(p.W, p.N, floor_nc) > budget) return false;
  if (fixed + chunk_bytes(p.W, p.N, nc) > budget) {      // largest chunk that fits (chunk_bytes is monotone in nc)
    size_t lo = floor_nc, hi = nc;
    while (lo < hi) {
      const size_t mid = lo + (hi - lo + 1) / 2;
      if (fixed + chunk_bytes(p.W, p.N, mid) <= budget) lo = mid; else hi = mid - 1;
    }
    nc = lo;
  }
  p.nc = nc;
  p.seg_cap = seg_bound(p.W, p.N, nc);
  p.bytes = fixed + chunk_bytes(p.W, p.N, nc);
  return true;
}
int32_t bucket_route(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, const Plan& P, void* base, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  uint8_t* q = (uint8_t*)base;
  auto take = [&](size_t bytes) { void* r = q; q += align_up(bytes); return r; };
  const size_t tiles = (P.N + SCAN_TILE - 1) / SCAN_TILE;
  u32* cnt = (u32*)take(P.N * 4);
  u64* off = (u64*)take(P.N * 8);
  u32* cursor = (u32*)take(P.N * 4);
  u64* tops = (u64*)take(tiles * 8);
  u64* meta = (u64*)take(8);
  i32* bk = (i32*)take(P.N * W27 * 4);
  i32* red = (i32*)take((size_t)P.W * P.T * W27 * 4);
  i32* win = (i32*)take((size_t)P.W * W27 * 4);
  int4* pts = (int4*)take(P.nc * PT_WORDS * 4);
  u32* idx = (u32*)take((size_t)P.W * P.nc * 4);
  i32* part = (i32*)take(P.seg_cap * W27 * 4);
  const hipStream_t st = (hipStream_t)stream;
  k_msm_bucket_init<<<GRID(P.N)>>>(bk, P.N);
  for (size_t b0 = 0; b0 < n; b0 += P.nc) {
    const size_t nc = n - b0 < P.nc ? n - b0 : P.nc;
    HIPCHK(hipMemsetAsync(cnt, 0, P.N * 4, st));
    k_msm_prep<<<GRID(nc)>>>(p_xy, n, b0, nc, pts);
    k_msm_hist<<<GRID(nc)>>>(p_inf, k, n, b0, nc, P.c, P.W, cnt);
    k_msm_scan_tiles<<<dim3((unsigned)tiles), dim3(BLOCK), 0, st>>>(cnt, P.N, off, tops);
    k_msm_scan_tops<<<1, BLOCK, 0, st>>>(tops, tiles, meta);
    k_msm_scan_add<<<GRID(P.N)>>>(off, P.N, tops, cursor);
    k_msm_scatter<<<GRID(nc)>>>(p_inf, k, n, b0, nc, P.c, P.W, cursor, idx);
    // the segment count is only known on the device: launch its bound (seg_bound of THIS chunk), surplus lanes leave at once
    const size_t segs = seg_bound(P.W, P.N, nc);
    k_msm_seg<<<GRID(segs)>>>(off, cnt, P.N, meta, P.seg_cap, idx, pts, bk, part);
    k_msm_seg_join<<<GRID(P.N)>>>(off, cnt, P.N, P.seg_cap, bk, part);
    const size_t tiles_b = (P.N + BLOCK - 1) / BLOCK;
    k_msm_seg_join_wide<<<dim3((unsigned)(tiles_b < 1024 ? tiles_b : 1024)), dim3(BLOCK), 0, st>>>(off, cnt, P.N, P.seg_cap, bk, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return host::fail(e, "msm chunk launch");
  }
  k_msm_bucket_reduce<<<GRID((size_t)P.W * P.T)>>>(bk, P.N, P.W, P.B, P.R, red);
  k_msm_window_sum<<<dim3((unsigned)P.W), dim3(BLOCK), 0, st>>>(red, P.W, P.T, win);
  k_msm_combine<<<1, 64, 0, st>>>(win, P.W, P.c, out_xy, out_inf);
  LAUNCHED();
}
}  // namespace msmh

extern "C" {
int32_t sylow_hip_g1_msm_tuned(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, int32_t window, int64_t min_n_arg,
                               uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  ARGCHK(out_xy && out_inf && (n == 0 || (p_xy && k)));
  ARGCHK(window < 0 || (window >= MSM_C_MIN && window <= MSM_C_MAX));
  const size_t min_n = min_n_arg < 0 ? MSM_DEFAULT_MIN : (size_t)min_n_arg;
  if (n > 0 && n >= min_n) {
    const size_t lim = host::scratch_limit();
    Plan P;
    if (msmh::plan(n, window < 0 ? default_window(n) : window, lim ? lim : MSM_DEFAULT_BUDGET, P)) {
      host::Lease ws;
      int32_t rc = ws.acquire(P.bytes, (hipStream_t)stream);
      if (rc != SYLOW_HIP_OK) return rc;
      rc = msmh::bucket_route(p_xy, p_inf, k, n, P, ws.p, out_xy, out_inf, stream);
      return host::finish(rc, ws);
    }
  }
  // small n (or a budget below one chunk of the bucket route): a scalar multiplication per lane, then the batch sum
  if (!n) {
    host::Lease ws;
    int32_t rc = ws.acquire(12 * sizeof(u64), (hipStream_t)stream);
    if (rc != SYLOW_HIP_OK) return rc;
    rc = g1h::sum_tree((uint64_t*)ws.p, 0, out_xy, out_inf, 1, 0, 0, stream);
    return host::finish(rc, ws);
  }
  host::Lease ws;
  int32_t rc = ws.acquire(n * (8 * sizeof(u64) + 1) + 12 * n * sizeof(u64) + 256, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint64_t* acc = (uint64_t*)ws.p;
  uint64_t* xy = acc + 12 * n;
  uint8_t* inf = (uint8_t*)(xy + 8 * n);
  rc = sylow_hip_g1_scalar_mul_batch(p_xy, p_inf, k, xy, inf, n, stream);
  if (rc == SYLOW_HIP_OK) rc = g1h::sum(xy, inf, n, acc, out_xy, out_inf, 1, 0, 0, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_g1_msm(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  return sylow_hip_g1_msm_tuned(p_xy, p_inf, k, n, -1, -1, out_xy, out_inf, stream);
}
}  // extern "C"
