// g2_msm.hpp -- the ways of collapsing many G2 points into one: sum_i Q_i, n_jobs weighted sums, and one large multi-scalar multiplication
// Q = sum_i k_i Q_i by the bucket method (Pippenger) on LANE PAIRS (bn254_pair.hpp: lane l and lane 7 - l of a group of 8 each hold one Fp
// coordinate of every Fp2 value; a projective point is 27 VGPRs per lane).
//
// The scalar side is msm_scalar.hpp with MOD_R = false: the digits are those of k mod p itself.  A point of E(Fp) has order r, a point of the
// twist need not (the twist's group order is r times a cofactor), and the contract is that of sylow_hip_g2_scalar_mul_batch: the product is
// exact on the whole twist.  k mod p < 2^254 and W c >= 255 still leave no carry out of the top window.
//
// The point side keeps the structure of msm.hip with one lane PAIR wherever G1 has one lane.  Per chunk of points:
//   k_g2msm_prep          affine SoA -> carry-free form on the ISOMORPHIC twist E'' (g2q_to_iso, plk_group.hip) once per point: the two Fp scalings
//                         are paid once, and each of the W additions of a point then uses OpsW2I, where 3 b'' is one reduce pass and not a
//                         product leaf.  One record of 2 x 80 bytes per point (this lane's x, y, 2 words of padding): a lane of the pair
//                         gathers its own half with five 16-byte loads
//   k_g2msm_seg           one lane pair per segment of <= MSM_SEG entries of one bucket, accumulator in registers, Z = 1 operands
//   k_g2msm_seg_join      one lane pair per bucket of 2 .. JOIN_LANE_MAX segments
//   k_g2msm_seg_join_wide one BLOCK (128 lane pairs) per bucket of more segments, then a tree in LDS
// Then once:
//   k_g2msm_bucket_reduce running sums over MSM_RUN contiguous buckets per lane pair
//   k_g2msm_window_sum    one block per window
//   k_g2msm_combine       Horner over the windows on one lane pair, g2q_from_iso, ONE normalisation to canonical affine words + flag
// The complete formulas throughout: a doubling, an identity or a cancelling pair inside a bucket needs no special case.
// This file is the tail of the unit plk_group.hip (included at its end): the build has no relocatable device code, and the kernels here use that
// unit's G2 group law on lane pairs (OpsW2I, g2q_to_iso / g2q_from_iso, store_g2q_affine) and its segmented sum.
// tools/msm_model.py (g2_* functions) is the host-side model of the recoding, the plan and the scratch formula (tests/test_g2_msm_model.py).
#pragma once

namespace {
constexpr int MSM_SEG = 32;            // entries per accumulation segment
constexpr u32 JOIN_LANE_MAX = 8;       // segments a bucket may have to be joined by one lane pair; more go to k_g2msm_seg_join_wide
constexpr int MSM_RUN = 16;            // buckets per lane pair in the running-sum reduction
constexpr int MSM_C_MIN = 4;           // window widths sylow_hip_g2_msm_tuned accepts
constexpr int MSM_C_MAX = 16;
constexpr int SCAN_ITEMS = 4, SCAN_TILE = BLOCK * SCAN_ITEMS;   // 1024 entries per scan block
constexpr size_t MSM_DEFAULT_BUDGET = (size_t)1 << 30;
// the smallest measured size from which the bucket route beats sylow_hip_g2_scalar_mul_batch + the sum at every larger size:
// 2^16 1.5 x, 2^15 0.72 x
constexpr size_t G2_MSM_DEFAULT_MIN = (size_t)1 << 16;
constexpr size_t G2_MSM_WIDE_FROM = (size_t)1 << 16;   // from this n on the default window is G2_MSM_WIDE_C
constexpr int G2_MSM_WIDE_C = 15;
constexpr size_t W54 = 54;             // words (i32) of a projective lane-pair point: 27 per lane
constexpr size_t PT2_WORDS = 40;       // words (i32) of a prepared affine point: per lane x, y, padding to 80 bytes
constexpr int PAIRS = BLOCK / 2;       // lane pairs of a block
}  // namespace
#include "msm_scalar.hpp"              // the scalar side and the plan, shared with msm.hip: reads the constants above

using namespace msm;

namespace plk {
// ------------------------------------------------------------------ lane-pair point SoA --------------
// a [27][2 * count] i32: word q of element i, coordinate `odd`, at a[q * 2 count + 2 i + odd]
BN_DEV W2 ldw(const i32* a, size_t stride2, size_t slot, int w0) {
  W2 r;
#pragma unroll
  for (int q = 0; q < 9; ++q) r.c.v[q] = a[(size_t)(w0 + q) * stride2 + slot];
  return r;
}
BN_DEV void stw(i32* a, size_t stride2, size_t slot, int w0, const W2& x) {
#pragma unroll
  for (int q = 0; q < 9; ++q) a[(size_t)(w0 + q) * stride2 + slot] = x.c.v[q];
}
BN_DEV G2Q ldq(const i32* a, size_t count, size_t i, int odd) {
  const size_t s2 = 2 * count, slot = 2 * i + (size_t)odd;
  return G2Q{ldw(a, s2, slot, 0), ldw(a, s2, slot, 9), ldw(a, s2, slot, 18)};
}
BN_DEV void stq(i32* a, size_t count, size_t i, int odd, const G2Q& p) {
  const size_t s2 = 2 * count, slot = 2 * i + (size_t)odd;
  stw(a, s2, slot, 0, p.x); stw(a, s2, slot, 9, p.y); stw(a, s2, slot, 18, p.z);
}
BN_DEV G2Q msm2_add(const G2Q& a, const G2Q& b) { return proj_add_lazy<OpsW2I>(a, b); }      // on E''
BN_DEV G2Q msm2_dbl(const G2Q& a) { return proj_double_lazy<OpsW2I>(a); }

__global__ void __launch_bounds__(BLOCK) k_g2msm_prep(const u64* pxy, size_t n, size_t base, size_t nc, int4* pts) {
  const size_t g = TID, t = pair_index(g);
  const int odd = pair_role(g);
  if (t >= nc) return;
  const size_t i = base + t;
  const G2Q p = g2q_to_iso(G2Q{w2_from_s2(load_s2(pxy, n, i, 0, odd)), w2_from_s2(load_s2(pxy, n, i, 8, odd)), OpsW2::one()});
  const F29 &x = p.x.c, &y = p.y.c;
  int4* d = pts + t * (PT2_WORDS / 4) + (size_t)odd * (PT2_WORDS / 8);
  d[0] = make_int4(x.v[0], x.v[1], x.v[2], x.v[3]);
  d[1] = make_int4(x.v[4], x.v[5], x.v[6], x.v[7]);
  d[2] = make_int4(x.v[8], y.v[0], y.v[1], y.v[2]);
  d[3] = make_int4(y.v[3], y.v[4], y.v[5], y.v[6]);
  d[4] = make_int4(y.v[7], y.v[8], 0, 0);
}
// prepared point t as (x : +-y : 1) on E'', this lane's coordinates
BN_DEV G2Q msm2_point(const int4* __restrict__ pts, u32 t, bool neg, int odd) {
  const int4* s = pts + (size_t)t * (PT2_WORDS / 4) + (size_t)odd * (PT2_WORDS / 8);
  const int4 a = s[0], b = s[1], c = s[2], d = s[3], e = s[4];
  G2Q p{W2{F29{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x}}}, W2{F29{{c.y, c.z, c.w, d.x, d.y, d.z, d.w, e.x, e.y}}}, OpsW2::one()};
  if (neg) p.y = OpsW2::neg(p.y);
  return p;
}

// ------------------------------------------------------------------ bucket accumulation ----------
__global__ void __launch_bounds__(BLOCK) k_g2msm_bucket_init(i32* bk, size_t N) {
  const size_t g = TID, b = pair_index(g);
  const int odd = pair_role(g);
  if (b >= N) return;
  stq(bk, N, b, odd, proj_zero<OpsW2>());
}
// lane pair s = segment s of the flat segment order: its bucket is the last b with seg_off(b) <= s (empty buckets share the next one's offset)
__global__ void HEAVY_BOUNDS k_g2msm_seg(const u64* off, const u32* cnt, size_t N, const u64* meta, size_t seg_cap, const u32* idx, const int4* pts,
                                         i32* bk, i32* part) {
  const size_t g = TID, s = pair_index(g);
  const int odd = pair_role(g);
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
  G2Q acc = msm2_point(pts, idx[first] & 0x7fffffffu, idx[first] >> 31, odd);
#pragma unroll 1
  for (u32 q = first + 1; q < last; ++q) {
    const u32 u = idx[q];
    acc = msm2_add(acc, msm2_point(pts, u & 0x7fffffffu, u >> 31, odd));
  }
  if (e <= MSM_SEG) stq(bk, N, b, odd, msm2_add(ldq(bk, N, b, odd), acc));   // the bucket's only segment: this lane pair owns it
  else stq(part, seg_cap, s, odd, acc);
}
__global__ void HEAVY_BOUNDS k_g2msm_seg_join(const u64* off, const u32* cnt, size_t N, size_t seg_cap, i32* bk, const i32* part) {
  const size_t g = TID, b = pair_index(g);
  const int odd = pair_role(g);
  if (b >= N) return;
  const u32 e = cnt[b];
  if (e <= MSM_SEG || e > JOIN_LANE_MAX * MSM_SEG) return;
  const size_t s0 = (size_t)(off[b] >> 32), ns = (e + MSM_SEG - 1) / MSM_SEG;
  G2Q acc = ldq(bk, N, b, odd);
#pragma unroll 1
  for (size_t j = 0; j < ns; ++j) acc = msm2_add(acc, ldq(part, seg_cap, s0 + j, odd));
  stq(bk, N, b, odd, acc);
}
// the PAIRS lane pairs' points -> their sum, returned to every lane pair (a level per barrier; lds: W54 * PAIRS words, free again on return)
BN_DEV G2Q block_sum2(const G2Q& mine, i32* lds, u32 p, int odd) {
  stq(lds, PAIRS, p, odd, mine);
  __syncthreads();
  for (u32 h = PAIRS / 2; h > 0; h >>= 1) {
    if (p < h) stq(lds, PAIRS, p, odd, msm2_add(ldq(lds, PAIRS, p, odd), ldq(lds, PAIRS, p + h, odd)));
    __syncthreads();
  }
  const G2Q r = ldq(lds, PAIRS, 0, odd);
  __syncthreads();
  return r;
}
// blocks stride over tiles of BLOCK buckets; each collects its tile's buckets of > JOIN_LANE_MAX segments and joins them one after the other,
// every one with all PAIRS lane pairs
__global__ void __launch_bounds__(BLOCK) k_g2msm_seg_join_wide(const u64* off, const u32* cnt, size_t N, size_t seg_cap, i32* bk, const i32* part) {
  __shared__ i32 lds[W54 * PAIRS];
  __shared__ u32 heavy[BLOCK];
  __shared__ u32 n_heavy;
  const int t = threadIdx.x, odd = pair_role((u32)t);
  const u32 p = pair_index((u32)t);
  for (size_t base = (size_t)blockIdx.x * BLOCK; base < N; base += (size_t)gridDim.x * BLOCK) {
    if (t == 0) n_heavy = 0;
    __syncthreads();
    if (base + t < N && cnt[base + t] > JOIN_LANE_MAX * MSM_SEG) heavy[atomicAdd(&n_heavy, 1u)] = (u32)t;
    __syncthreads();
    const u32 m = n_heavy;
    for (u32 h = 0; h < m; ++h) {
      const size_t b = base + heavy[h];
      const size_t s0 = (size_t)(off[b] >> 32), ns = (cnt[b] + MSM_SEG - 1) / MSM_SEG;
      G2Q acc = proj_zero<OpsW2>();
#pragma unroll 1
      for (size_t j = p; j < ns; j += PAIRS) acc = msm2_add(acc, ldq(part, seg_cap, s0 + j, odd));
      acc = block_sum2(acc, lds, p, odd);
      if (p == 0) stq(bk, N, b, odd, msm2_add(ldq(bk, N, b, odd), acc));
    }
    __syncthreads();                                    // every thread has read n_heavy before it is reset
  }
}

// ------------------------------------------------------------------ window reduction and combination ----------
// lane pair (w, t): buckets t R .. t R + R - 1 of window w (magnitudes t R + 1 .. t R + R).  Running sums from the top give sum_j (j + 1) B_j;
// adding t R times the range sum makes it sum_m m B_m.  Partial -> red[w T + t].
// One wave per SIMD (no second argument to the launch bounds): three live points (run, acc, q or an operand: 81 VGPRs per lane) and an
// addition's temporaries do not fit in the 256 registers of HEAVY_BOUNDS without spilling, and W T lane pairs are a few hundred wavefronts.
__global__ void __launch_bounds__(BLOCK) k_g2msm_bucket_reduce(const i32* bk, size_t N, int W, size_t B, size_t R, i32* red) {
  const size_t T = B / R, g = pair_index(TID);
  const int odd = pair_role(TID);
  if (g >= (size_t)W * T) return;
  const size_t w = g / T, t = g % T, base = w * B + t * R;
  G2Q run = proj_zero<OpsW2>(), acc = proj_zero<OpsW2>();
#pragma unroll 1
  for (size_t j = R; j-- > 0;) {
    run = msm2_add(run, ldq(bk, N, base + j, odd));
    acc = msm2_add(acc, run);
  }
  const u32 m = (u32)(t * R);                           // < 2^15
  if (m) {
    G2Q q = proj_zero<OpsW2>();
#pragma unroll 1
    for (int bit = 31 - __builtin_clz(m); bit >= 0; --bit) {
      q = msm2_dbl(q);
      if ((m >> bit) & 1u) q = msm2_add(q, run);
    }
    acc = msm2_add(acc, q);
  }
  stq(red, (size_t)W * T, g, odd, acc);
}
// block w: S_w = sum of the T partials of window w (serial per lane pair, then a tree in LDS)
__global__ void __launch_bounds__(BLOCK) k_g2msm_window_sum(const i32* red, int W, size_t T, i32* win) {
  __shared__ i32 lds[W54 * PAIRS];
  const size_t w = blockIdx.x, count = (size_t)W * T;
  const u32 p = pair_index((u32)threadIdx.x);
  const int odd = pair_role((u32)threadIdx.x);
  G2Q acc = proj_zero<OpsW2>();
#pragma unroll 1
  for (size_t j = p; j < T; j += PAIRS) acc = msm2_add(acc, ldq(red, count, w * T + j, odd));
  acc = block_sum2(acc, lds, p, odd);
  if (p == 0) stq(win, (size_t)W, w, odd, acc);
}
__global__ void __launch_bounds__(64) k_g2msm_combine(const i32* win, int W, int c, u64* oxy, uint8_t* oinf) {
  if (pair_index((u32)threadIdx.x) != 0) return;       // one lane pair: lanes 0 and 7
  const int odd = pair_role((u32)threadIdx.x);
  G2Q acc = ldq(win, (size_t)W, (size_t)W - 1, odd);
#pragma unroll 1
  for (int w = W - 2; w >= 0; --w) {
#pragma unroll 1
    for (int j = 0; j < c; ++j) acc = msm2_dbl(acc);
    acc = msm2_add(acc, ldq(win, (size_t)W, (size_t)w, odd));
  }
  store_g2q_affine(oxy, oinf, 1, 0, odd, g2q_from_iso(acc));
}
}  // namespace plk

// ================================================================== host ======================
namespace g2msmh {
// The default window: the rule of sylow_hip_g1_msm below 2^16, c = 15 from there on.  The sweep of c at 2^16 and 2^20 has
// c = 15 fastest at both sizes, and the G1 rule's c = 13 for 2^16 and 2^17 3.6 x slower than it: the 7-bit top window of c = 13 puts every
// point of that window into 64 buckets of ONE tile, which k_g2msm_seg_join_wide joins one after the other.
int g2_default_window(size_t n) { return n >= G2_MSM_WIDE_FROM ? G2_MSM_WIDE_C : default_window(n); }
bool plan(size_t n, int c, size_t budget, Plan& p) { return msm::plan<W54, PT2_WORDS>(n, c, budget, p); }
int32_t bucket_route(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, const Plan& P, void* base, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  uint8_t* q = (uint8_t*)base;
  auto take = [&](size_t bytes) { void* r = q; q += align_up(bytes); return r; };
  const size_t tiles = (P.N + SCAN_TILE - 1) / SCAN_TILE;
  u32* cnt = (u32*)take(P.N * 4);
  u64* off = (u64*)take(P.N * 8);
  u32* cursor = (u32*)take(P.N * 4);
  u64* tops = (u64*)take(tiles * 8);
  u64* meta = (u64*)take(8);
  i32* bk = (i32*)take(P.N * W54 * 4);
  i32* red = (i32*)take((size_t)P.W * P.T * W54 * 4);
  i32* win = (i32*)take((size_t)P.W * W54 * 4);
  int4* pts = (int4*)take(P.nc * PT2_WORDS * 4);
  u32* idx = (u32*)take((size_t)P.W * P.nc * 4);
  i32* part = (i32*)take(P.seg_cap * W54 * 4);
  const hipStream_t st = (hipStream_t)stream;
  plk::k_g2msm_bucket_init<<<GRID(2 * P.N)>>>(bk, P.N);
  for (size_t b0 = 0; b0 < n; b0 += P.nc) {
    const size_t nc = n - b0 < P.nc ? n - b0 : P.nc;
    HIPCHK(hipMemsetAsync(cnt, 0, P.N * 4, st));
    plk::k_g2msm_prep<<<GRID(2 * nc)>>>(p_xy, n, b0, nc, pts);
    k_msm_hist<false><<<GRID(nc)>>>(p_inf, k, n, b0, nc, P.c, P.W, cnt);
    k_msm_scan_tiles<false><<<dim3((unsigned)tiles), dim3(BLOCK), 0, st>>>(cnt, P.N, off, tops);
    k_msm_scan_tops<false><<<1, BLOCK, 0, st>>>(tops, tiles, meta);
    k_msm_scan_add<false><<<GRID(P.N)>>>(off, P.N, tops, cursor);
    k_msm_scatter<false><<<GRID(nc)>>>(p_inf, k, n, b0, nc, P.c, P.W, cursor, idx);
    // the segment count is only known on the device: launch its bound (seg_bound of THIS chunk), surplus lane pairs leave at once
    const size_t segs = seg_bound(P.W, P.N, nc);
    plk::k_g2msm_seg<<<GRID(2 * segs)>>>(off, cnt, P.N, meta, P.seg_cap, idx, pts, bk, part);
    plk::k_g2msm_seg_join<<<GRID(2 * P.N)>>>(off, cnt, P.N, P.seg_cap, bk, part);
    const size_t tiles_b = (P.N + BLOCK - 1) / BLOCK;
    plk::k_g2msm_seg_join_wide<<<dim3((unsigned)(tiles_b < 1024 ? tiles_b : 1024)), dim3(BLOCK), 0, st>>>(off, cnt, P.N, P.seg_cap, bk, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return host::fail(e, "g2 msm chunk launch");
  }
  plk::k_g2msm_bucket_reduce<<<GRID(2 * (size_t)P.W * P.T)>>>(bk, P.N, P.W, P.B, P.R, red);
  plk::k_g2msm_window_sum<<<dim3((unsigned)P.W), dim3(BLOCK), 0, st>>>(red, P.W, P.T, win);
  plk::k_g2msm_combine<<<1, 64, 0, st>>>(win, P.W, P.c, out_xy, out_inf);
  LAUNCHED();
}
// k_i Q_i per lane pair (exact on the whole twist), then the segmented sum: n_seg sums of c terms each, term-major
int32_t composed(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n_seg, size_t c, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  const size_t n = n_seg * c, acc_words = plkh::g2_sum_scratch_words(n_seg, c);
  host::Lease ws;
  int32_t rc = ws.acquire((acc_words + 16 * n) * sizeof(u64) + n + 256, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint64_t* acc = (uint64_t*)ws.p;
  uint64_t* xy = acc + acc_words;
  uint8_t* inf = (uint8_t*)(xy + 16 * n);
  if (n) rc = sylow_hip_g2_scalar_mul_batch(p_xy, p_inf, k, xy, inf, n, stream);
  if (rc == SYLOW_HIP_OK) rc = plkh::g2_sum(xy, inf, n_seg, c, acc, out_xy, out_inf, stream);
  return host::finish(rc, ws);
}
}  // namespace g2msmh

extern "C" {
int32_t sylow_hip_g2_sum_batch(const uint64_t* q_xy, const uint8_t* q_inf, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  ARGCHK(out_xy && out_inf && (n == 0 || q_xy));
  host::Lease ws;
  int32_t rc = ws.acquire(plkh::g2_sum_scratch_words(1, n) * sizeof(u64) + 256, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  rc = plkh::g2_sum(q_xy, q_inf, 1, n, (uint64_t*)ws.p, out_xy, out_inf, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_g2_lincomb_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, uint64_t* out_xy, uint8_t* out_inf,
                                   size_t n_jobs, size_t n_terms, void* stream) {
  ARGCHK(out_xy && out_inf && (n_jobs * n_terms == 0 || (p_xy && k)));
  if (!n_jobs) return SYLOW_HIP_OK;
  return g2msmh::composed(p_xy, p_inf, k, n_jobs, n_terms, out_xy, out_inf, stream);
}
int32_t sylow_hip_g2_msm_tuned(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, int32_t window, int64_t min_n_arg,
                               uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  ARGCHK(out_xy && out_inf && (n == 0 || (p_xy && k)));
  ARGCHK(window < 0 || (window >= MSM_C_MIN && window <= MSM_C_MAX));
  const size_t min_n = min_n_arg < 0 ? G2_MSM_DEFAULT_MIN : (size_t)min_n_arg;
  if (n > 0 && n >= min_n) {
    const size_t lim = host::scratch_limit();
    Plan P;
    if (g2msmh::plan(n, window < 0 ? g2msmh::g2_default_window(n) : window, lim ? lim : MSM_DEFAULT_BUDGET, P)) {
      host::Lease ws;
      int32_t rc = ws.acquire(P.bytes, (hipStream_t)stream);
      if (rc != SYLOW_HIP_OK) return rc;
      rc = g2msmh::bucket_route(p_xy, p_inf, k, n, P, ws.p, out_xy, out_inf, stream);
      return host::finish(rc, ws);
    }
  }
  // small n (or a budget below one chunk of the bucket route): a scalar multiplication per lane pair, then the segmented sum with one segment
  return g2msmh::composed(p_xy, p_inf, k, 1, n, out_xy, out_inf, stream);
}
int32_t sylow_hip_g2_msm(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  return sylow_hip_g2_msm_tuned(p_xy, p_inf, k, n, -1, -1, out_xy, out_inf, stream);
}
}  // extern "C"
