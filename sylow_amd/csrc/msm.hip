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
// The scalar side (recoding, histogram, scan, scatter) and the plan live in msm_scalar.hpp, shared with the G2 route (g2_msm.hpp).
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
#include "msm_scalar.hpp"              // the scalar side and the plan, shared with g2_msm.hpp: reads the constants above

using namespace msm;

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
namespace msmh {
typedef msm::Plan Plan;
bool plan(size_t n, int c, size_t budget, Plan& p) { return msm::plan<W27, PT_WORDS>(n, c, budget, p); }
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
    k_msm_hist<true><<<GRID(nc)>>>(p_inf, k, n, b0, nc, P.c, P.W, cnt);
    k_msm_scan_tiles<true><<<dim3((unsigned)tiles), dim3(BLOCK), 0, st>>>(cnt, P.N, off, tops);
    k_msm_scan_tops<true><<<1, BLOCK, 0, st>>>(tops, tiles, meta);
    k_msm_scan_add<true><<<GRID(P.N)>>>(off, P.N, tops, cursor);
    k_msm_scatter<true><<<GRID(nc)>>>(p_inf, k, n, b0, nc, P.c, P.W, cursor, idx);
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
