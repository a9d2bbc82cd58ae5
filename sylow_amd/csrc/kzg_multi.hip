// kzg_multi.hip -- many KZG polynomials opened at one point under ONE folded proof (include/sylow_hip.h, "KZG, folded openings"): the m
//   polynomials fall into G groups of consecutive polynomials, group g is opened at z_g and folded under gamma_g.  New here: the grouped linear
//   combination over Fr, out_g = sum_j w_j a_j (k_fr_lincomb: one launch, unreduced multiply-accumulates), the powers gamma_g^i, and the small
//   kernels around them.  The quotient, the commitments and the pairing check are the library's own stream-ordered calls, as they stand.
// Tiles, grids, the flush length, scratch and the chunks of the combined commitments: kzg_multi_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_acc.hpp"
#include "bn254_fr_block.hpp"
#include "kzg_multi_plan.hpp"

namespace kzgm {
using namespace kzgm_plan;
static_assert(KZGM_BLOCK == BLOCK, "the kernels run blocks of BLOCK lanes");
constexpr int T = (int)KZGM_LINCOMB_TILE, FL = KZGM_LINCOMB_FLUSH;

// group_start on its way to the device: `count` offsets from the launch's own arguments to dst
struct Offsets {
  u64 v[KZGM_OFFSET_ARGS];
};
__global__ void __launch_bounds__(BLOCK) k_kzgm_offsets(Offsets o, u64* dst, size_t count) {
  if (threadIdx.x < count) dst[threadIdx.x] = o.v[threadIdx.x];
}

// out_g[k] = sum_{j = gs[g] .. gs[g+1] - 1} w_j a_j[k] mod r for a [m][4][len], w [4][m], out [G][4][len]; an empty group stores zeros.
// Block (x, y) takes the tiles x, x + gridDim.x, ... of the groups y, y + gridDim.y, ...; lane t owns column k = tile T + t.  The polynomials
// of the group go by in rounds of FL: FL lanes bring the round's weights to canonical form and stage them in LDS (ONE fetch per block and
// term; every lane then reads the same LDS word, a broadcast), each lane adds its FL products a_j[k] w_j into 16 limbs UNREDUCED and folds
// them with one fr_reduce_wide.  THE BOUND (bn254_fr_acc.hpp): both factors are canonical -- a_j[k] is ANY word and is reduced at the load,
// the weights when they are staged -- and a round starts from a residue below r, so the accumulator stays below r + 16 r^2 < 2^512.
// The next term's four words are in flight while the current product is formed.  Every lane of a block sees the same group and the same
// rounds, so the barriers are reached by whole blocks.  Every index is size_t; no read leaves a [m][4][len], w [4][m] or gs [G + 1] because
// gs is non-decreasing and ends at m (checked on the host before anything is enqueued).
__global__ void __launch_bounds__(BLOCK) k_fr_lincomb(const u64* a, size_t len, size_t m, const u64* w, const u64* gs, size_t G, size_t tiles, u64* out) {
  __shared__ u32 wl[FL][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t g = blockIdx.y; g < G; g += gridDim.y) {
    const size_t j0 = gs[g], j1 = gs[g + 1];
    u64* o = out + g * 4 * len;
#pragma unroll 1
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
      const size_t k = tile * T + (size_t)t;
      const bool live = k < len;
      Fp res = fr_zero();
#pragma unroll 1
      for (size_t jb = j0; jb < j1; jb += FL) {
        const int cnt = j1 - jb < (size_t)FL ? (int)(j1 - jb) : FL;
        __syncthreads();                                      // the round before has read its weights
        if (t < cnt) lds_put(wl, t, fr_reduce_plain(load_plain(w, m, jb + (size_t)t, 0)));
        __syncthreads();
        if (live) {
          u32 acc[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] = i < 8 ? res.v[i] : 0;
          Fp nxt = load_plain(a + jb * 4 * len, len, k, 0);
#pragma unroll 1
          for (int i = 0; i < cnt; ++i) {
            const Fp cur = fr_reduce_plain(nxt);
            if (i + 1 < cnt) nxt = load_plain(a + (jb + (size_t)i + 1) * 4 * len, len, k, 0);
            mul_acc(acc, cur, lds_get(wl, i));
          }
          res = fr_reduce_wide(acc);
        }
      }
      if (live) store_plain(o, len, k, 0, res);
    }
  }
}

// the group of polynomial j < m = gs[G]: the g with gs[g] <= j < gs[g + 1] (empty groups are stepped over)
BN_DEV size_t group_of(const u64* gs, size_t G, size_t j) {
  size_t lo = 0, hi = G;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (gs[mid + 1] <= j) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// One lane per polynomial j of group g, i = j - gs[g]: pow_out_j = gamma_g^i (0^0 = 1) and z_out_j = z_g as it lies; either output may be
// NULL.  SQUARE-AND-MULTIPLY on i, not a walk along the group: the lanes stay independent and a lane runs at most 2 log2(i) products, where a
// walk is serial in the length of the group (65536 products in a row for one group of 2^16).
__global__ void __launch_bounds__(BLOCK) k_kzgm_group_powers(const u64* gamma, const u64* z, const u64* gs, size_t G, size_t m, u64* pow_out, u64* z_out) {
#pragma unroll 1
  for (size_t j = TID; j < m; j += (size_t)gridDim.x * BLOCK) {
    const size_t g = group_of(gs, G, j);
    if (z_out) store_plain(z_out, m, j, 0, load_plain(z, G, g, 0));
    if (!pow_out) continue;
    Fp b = fr_reduce_plain(load_plain(gamma, G, g, 0)), p = fr_one();
#pragma unroll 1
    for (size_t i = j - gs[g]; i; i >>= 1) {
      if (i & 1) p = fr_mul(p, b);
      if (i >> 1) b = fr_mul(b, b);
    }
    store_plain(pow_out, m, j, 0, p);
  }
}
// y_F,g = sum_j pow_j y_j mod r, a block per group: the lanes stride over the group, then a tree over LDS.  A modular sum: the order of the
// terms does not show in the words.  pow is canonical (k_kzgm_group_powers); y is any word, reduced at the load.
__global__ void __launch_bounds__(BLOCK) k_kzgm_fold_values(const u64* y, const u64* pow, size_t m, const u64* gs, size_t G, u64* yf) {
  __shared__ u32 part[BLOCK][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t g = blockIdx.x; g < G; g += gridDim.x) {
    const size_t j1 = gs[g + 1];
    Fp s = fr_zero();
#pragma unroll 1
    for (size_t j = gs[g] + (size_t)t; j < j1; j += BLOCK) s = fr_add(s, fr_mul(fr_reduce_plain(load_plain(y, m, j, 0)), load_plain(pow, m, j, 0)));
    s = block_sum(s, part);                                   // ends on a barrier: part is free for the next group
    if (t == 0) store_plain(yf, G, g, 0, s);
  }
}
// The padded layout of `n_seg` groups from g0 on, `c` slots each, term-major (slot k of group g0 + s at index k n_seg + s, what
// g1h::sum_segments reads; n_seg = 1 is a plain array of c pairs, what sylow_hip_g1_msm reads): a slot inside its group holds (C_j, its flag,
// pow_j), a slot past the group's end the flagged identity (0, 1) and the scalar 0.
__global__ void __launch_bounds__(BLOCK) k_kzgm_combine_prep(const u64* c_xy, const uint8_t* c_inf, size_t m, const u64* pow, const u64* gs, size_t g0, size_t n_seg,
                                                            size_t c, u64* sc, u64* bases, uint8_t* flags) {
  const size_t n = n_seg * c;
#pragma unroll 1
  for (size_t i = TID; i < n; i += (size_t)gridDim.x * BLOCK) {
    const size_t k = i / n_seg, s = i - k * n_seg, g = g0 + s;
    const bool real = k < gs[g + 1] - gs[g];
    const size_t j = real ? gs[g] + k : 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) bases[(size_t)w * n + i] = real ? c_xy[(size_t)w * m + j] : (w == 4 ? 1 : 0);
#pragma unroll
    for (int w = 0; w < 4; ++w) sc[(size_t)w * n + i] = real ? pow[(size_t)w * m + j] : 0;
    flags[i] = real ? (c_inf && c_inf[j] ? 1 : 0) : 1;
  }
}
// n points of an [8][n] array + flags to the columns col0 .. col0 + n - 1 of out [8][stride] + flags
__global__ void __launch_bounds__(BLOCK) k_kzgm_put_points(const u64* src, const uint8_t* src_inf, size_t n, u64* out_xy, uint8_t* out_inf, size_t stride, size_t col0) {
  const size_t j = TID;
  if (j >= n) return;
#pragma unroll
  for (int w = 0; w < 8; ++w) out_xy[(size_t)w * stride + col0 + j] = src[(size_t)w * n + j];
  out_inf[col0 + j] = src_inf[j];
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
// group_start -> dst [G + 1] on the device, through kernel arguments (kzg_multi_plan.hpp): the host array is free when this returns
static int32_t put_offsets(const uint64_t* group_start, size_t G, u64* dst, hipStream_t st) {
  const size_t total = offset_words(G);
  for (size_t at = 0; at < total; at += KZGM_OFFSET_ARGS) {
    Offsets o;
    const size_t count = total - at < KZGM_OFFSET_ARGS ? total - at : KZGM_OFFSET_ARGS;
    for (size_t i = 0; i < KZGM_OFFSET_ARGS; ++i) o.v[i] = i < count ? group_start[at + i] : 0;
    k_kzgm_offsets<<<dim3(1), dim3(BLOCK), 0, st>>>(o, dst + at, count);
  }
  LAUNCHED();
}
static void lincomb_launch(const u64* a, size_t len, size_t m, const u64* w, const u64* gs, size_t G, u64* out, hipStream_t st) {
  k_fr_lincomb<<<dim3((unsigned)lincomb_grid_x(len), (unsigned)lincomb_grid_y(G)), dim3(BLOCK), 0, st>>>(a, len, m, w, gs, G, lincomb_tiles(len), out);
}
static void powers_launch(const u64* gamma, const u64* z, const u64* gs, size_t G, size_t m, u64* pow_out, u64* z_out, hipStream_t st) {
  k_kzgm_group_powers<<<dim3((unsigned)lane_grid(m)), dim3(BLOCK), 0, st>>>(gamma, z, gs, G, m, pow_out, z_out);
}
static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

// The prover's common part once the y_j are written: the powers and z spread to the polynomials are in ws; F = the folded polynomials (or
// the folded values) into ws.  Layout of ws: kzgm_plan::open_layout
struct OpenScratch {
  u64 *gs, *pow, *zs, *f, *yf;
  OpenScratch(const host::Lease& ws, const OpenLayout& l) : gs(ws.at<u64>(l.gs)), pow(ws.at<u64>(l.pow)), zs(ws.at<u64>(l.zs)), f(ws.at<u64>(l.f)), yf(ws.at<u64>(l.yf)) {}
};
static int32_t open_setup(host::Lease& ws, const uint64_t* group_start, size_t len, size_t m, size_t G, const uint64_t* z, const uint64_t* gamma, hipStream_t st) {
  const OpenLayout l = open_layout(len, m, G);
  if (l.bytes == SAT) {
    snprintf(sylow_g_err, sizeof(sylow_g_err), "bad argument: the scratch of %zu groups of %zu terms does not fit size_t", G, len);
    return SYLOW_HIP_E_ARG;
  }
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  const OpenScratch s(ws, l);
  rc = put_offsets(group_start, G, s.gs, st);
  if (rc == SYLOW_HIP_OK) powers_launch(gamma, z, s.gs, G, m, s.pow, s.zs, st);
  return rc;
}

// C_F and y_F of the verifier; gs and pow are on the device already
static int32_t combine(const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* y, size_t m, const uint64_t* group_start, const u64* gs, const u64* pow, size_t G,
                       uint64_t* cf_xy, uint8_t* cf_inf, uint64_t* yf, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  k_kzgm_fold_values<<<dim3((unsigned)group_grid(G)), dim3(BLOCK), 0, st>>>(y, pow, m, gs, G, yf);
  const size_t lim = host::scratch_limit(), budget = lim ? lim : msmh::default_budget(), msm_min = msmh::g1_default_min();
  int32_t rc = SYLOW_HIP_OK;
  for (size_t g0 = 0; g0 < G && rc == SYLOW_HIP_OK;) {
    const CombineChunk ch = combine_chunk(group_start, G, g0, msm_min, budget);
    const size_t n_seg = ch.g_end - g0;
    const size_t n = n_seg * ch.terms, w_acc = ch.route == Route::SEGMENTS ? g1h::sum_segments_scratch_words(n_seg, ch.terms) : 0;
    const bool direct = ch.route == Route::SEGMENTS && n_seg == G;      // one chunk: the segmented sum writes [8][G] itself
    host::Lease ws;
    const ChunkLayout l = chunk_layout(n, n_seg, w_acc);
    rc = ws.acquire(l.bytes, st);
    if (rc != SYLOW_HIP_OK) return rc;
    u64 *sc = ws.at<u64>(l.sc), *bases = ws.at<u64>(l.bases), *prod = ws.at<u64>(l.prod), *acc = ws.at<u64>(l.acc), *part = ws.at<u64>(l.part);
    uint8_t *flags = ws.at<uint8_t>(l.flags), *prod_inf = ws.at<uint8_t>(l.prod_inf), *part_inf = ws.at<uint8_t>(l.part_inf);
    k_kzgm_combine_prep<<<dim3((unsigned)lane_grid(n)), dim3(BLOCK), 0, st>>>(c_xy, c_inf, m, pow, gs, g0, n_seg, ch.terms, sc, bases, flags);
    if (ch.route == Route::MSM) {
      rc = sylow_hip_g1_msm(bases, flags, sc, n, part, part_inf, stream);
    } else {
      rc = sylow_hip_g1_scalar_mul_batch(bases, flags, sc, prod, prod_inf, n, stream);
      if (rc == SYLOW_HIP_OK) rc = direct ? g1h::sum_segments(prod, prod_inf, n_seg, ch.terms, acc, cf_xy, cf_inf, stream)
                                          : g1h::sum_segments(prod, prod_inf, n_seg, ch.terms, acc, part, part_inf, stream);
    }
    if (rc == SYLOW_HIP_OK && !direct) k_kzgm_put_points<<<GRID(n_seg)>>>(part, part_inf, n_seg, cf_xy, cf_inf, G, g0);
    rc = host::finish(rc, ws);
    g0 = ch.g_end;
  }
  return rc;
}
// gs and pow into a fresh lease, then combine
static int32_t combine_call(const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* y, size_t m, const uint64_t* group_start, size_t G, const uint64_t* gamma,
                            uint64_t* cf_xy, uint8_t* cf_inf, uint64_t* yf, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const CombineLayout l = combine_layout(m, G);
  const size_t words = words_of(l.bytes);
  ARGCHK(words <= SAT / sizeof(u64));
  host::Lease ws;
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *gs = ws.at<u64>(l.gs), *pow = ws.at<u64>(l.pow);
  rc = put_offsets(group_start, G, gs, st);
  if (rc == SYLOW_HIP_OK) {
    powers_launch(gamma, nullptr, gs, G, m, pow, nullptr, st);
    rc = combine(c_xy, c_inf, y, m, group_start, gs, pow, G, cf_xy, cf_inf, yf, stream);
  }
  return host::finish(rc, ws);
}
}  // namespace kzgm

#define GROUPCHK(gs, G, m) ARGCHK(kzgm_plan::groups_ok(gs, G, m))

extern "C" {
int32_t sylow_hip_fr_lincomb_batch(const uint64_t* a, size_t len, size_t m, const uint64_t* weights, const uint64_t* group_start, size_t G, uint64_t* out,
                                   void* stream) {
  using namespace kzgm;
  ARGCHK(len > 0); if (!m || !G) return SYLOW_HIP_OK;
  ARGCHK(a && weights && group_start && out);
  GROUPCHK(group_start, G, m);
  ARGCHK(m <= SAT / (4 * sizeof(u64)) / len && G <= SAT / (4 * sizeof(u64)) / len);
  ARGCHK(!ranges_overlap(a, 4 * sizeof(u64) * len * m, out, 4 * sizeof(u64) * len * G));
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  int32_t rc = ws.acquire(offset_bytes(G), st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* gs = ws.at<u64>(0);
  rc = put_offsets(group_start, G, gs, st);
  if (rc == SYLOW_HIP_OK) lincomb_launch(a, len, m, weights, gs, G, out, st);
  return host::finish(rc, ws);
}
int32_t sylow_hip_fr_group_powers_batch(const uint64_t* gamma, const uint64_t* group_start, size_t G, size_t m, uint64_t* out, void* stream) {
  using namespace kzgm;
  if (!m || !G) return SYLOW_HIP_OK;
  ARGCHK(gamma && group_start && out);
  GROUPCHK(group_start, G, m);
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  int32_t rc = ws.acquire(offset_bytes(G), st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* gs = ws.at<u64>(0);
  rc = put_offsets(group_start, G, gs, st);
  if (rc == SYLOW_HIP_OK) powers_launch(gamma, nullptr, gs, G, m, out, nullptr, st);
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_open_multi_batch(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, const uint64_t* group_start, size_t G,
                                       const uint64_t* z, const uint64_t* gamma, uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  using namespace kzgm;
  ARGCHK(len > 0); if (!m || !G) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && coeffs && group_start && z && gamma && y_out && pi_xy && pi_inf);
  GROUPCHK(group_start, G, m);
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  int32_t rc = open_setup(ws, group_start, len, m, G, z, gamma, st);
  if (rc != SYLOW_HIP_OK) return rc;
  const OpenScratch s(ws, open_layout(len, m, G));
  rc = sylow_hip_kzg_quotient_batch(coeffs, len, m, s.zs, nullptr, y_out, stream);                 // y_j = f_j(z_g): evaluation only
  if (rc == SYLOW_HIP_OK) {
    lincomb_launch(coeffs, len, m, s.pow, s.gs, G, s.f, st);
    rc = sylow_hip_kzg_open_batch(srs_g1_xy, s.f, len, G, z, s.yf, pi_xy, pi_inf, stream);         // the quotient of F_g at z_g and its commitment
  }
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_open_multi_evals_batch(const uint64_t* srs_lagrange_xy, const uint64_t* evals, int32_t log_n, size_t m, const uint64_t* group_start,
                                             size_t G, const uint64_t* z, const uint64_t* gamma, uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  using namespace kzgm;
  ARGCHK(log_n >= 0 && log_n <= 28); if (!m || !G) return SYLOW_HIP_OK;
  ARGCHK(srs_lagrange_xy && evals && group_start && z && gamma && y_out && pi_xy && pi_inf);
  GROUPCHK(group_start, G, m);
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)1 << log_n;
  host::Lease ws;
  int32_t rc = open_setup(ws, group_start, n, m, G, z, gamma, st);
  if (rc != SYLOW_HIP_OK) return rc;
  const OpenScratch s(ws, open_layout(n, m, G));
  rc = sylow_hip_kzg_quotient_evals_batch(evals, log_n, m, s.zs, nullptr, y_out, stream);          // barycentric evaluation alone
  if (rc == SYLOW_HIP_OK) {
    lincomb_launch(evals, n, m, s.pow, s.gs, G, s.f, st);                                          // the values of F_g: the fold is linear
    rc = sylow_hip_kzg_open_evals_batch(srs_lagrange_xy, s.f, log_n, G, z, s.yf, pi_xy, pi_inf, stream);
  }
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_combine_openings_batch(const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* y, size_t m, const uint64_t* group_start, size_t G,
                                             const uint64_t* gamma, uint64_t* cf_xy, uint8_t* cf_inf, uint64_t* yf, void* stream) {
  if (!m || !G) return SYLOW_HIP_OK;
  ARGCHK(c_xy && y && group_start && gamma && cf_xy && cf_inf && yf);
  GROUPCHK(group_start, G, m);
  return kzgm::combine_call(c_xy, c_inf, y, m, group_start, G, gamma, cf_xy, cf_inf, yf, stream);
}
int32_t sylow_hip_kzg_verify_multi_batch(const uint64_t* tau_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* y, size_t m,
                                         const uint64_t* group_start, size_t G, const uint64_t* z, const uint64_t* gamma, const uint64_t* pi_xy,
                                         const uint8_t* pi_inf, uint8_t* ok, void* stream) {
  using namespace kzgm;
  if (!m || !G) return SYLOW_HIP_OK;
  ARGCHK(tau_g2_xy && c_xy && y && group_start && z && gamma && pi_xy && ok);
  GROUPCHK(group_start, G, m);
  const VerifyLayout l = verify_layout(G);
  const size_t words = words_of(l.bytes);
  ARGCHK(words <= SAT / sizeof(u64));
  host::Lease ws;
  int32_t rc = ws.acquire(l.bytes, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *cf = ws.at<u64>(l.cf), *yf = ws.at<u64>(l.yf);
  uint8_t* cf_inf = ws.at<uint8_t>(l.cf_inf);
  rc = combine_call(c_xy, c_inf, y, m, group_start, G, gamma, cf, cf_inf, yf, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_kzg_verify_batch(tau_g2_xy, cf, cf_inf, z, yf, pi_xy, pi_inf, ok, G, stream);
  return host::finish(rc, ws);
}
}  // extern "C"
