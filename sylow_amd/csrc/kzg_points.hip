// kzg_points.hip -- ONE KZG polynomial opened at SEVERAL points under one proof (include/sylow_hip_kzg_points.h).  For the points z_0 .. z_{k-1} of
//   a polynomial f, Z = prod (X - z_i), a_i = 1 / prod_{l != i} (z_i - z_l) and q_i = (f - f(z_i)) / (X - z_i):
//     f div Z = sum_i a_i q_i,     f mod Z = sum_i f(z_i) a_i Z / (X - z_i),
//   so the k Horner scans of kzg_prove.hip run INDEPENDENTLY and are folded under the weights before anything is stored.  New here: the
//   weights (denominators, then sylow_hip_fr_batch_inv: inv(0) = 0, so a repeated point drops out), the totals and carry passes over
//   (polynomial, point, chunk) items, the chunk kernel that walks the k points inside the block and stores the quotient ONCE, the verifier's
//   Fr half (Z and f mod Z as coefficients) and the small kernels that lay out its G2 sum and its pair list.  The commitment, the G2 sum, the
//   G1 difference and the pairing products are the library's own stream-ordered calls, as they stand.
// Items, grids, scratch and the chunks of the G2 half: kzg_points_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "kzg_scan_dev.hpp"
#include "kzg_points_plan.hpp"
#include "../../include/sylow_hip_kzg_points.h"

namespace kzgpt {
using namespace kzg_scan;
using namespace kzgpt_plan;
static_assert(KZGPT_BLOCK == BLOCK, "the kernels run blocks of BLOCK lanes");
static_assert(KZGPT_MAX_POINTS == SYLOW_HIP_KZG_POINTS_MAX, "the header states the plan's limit");
constexpr int RB = KZGPT_ROW_BLOCK, MAXK = (int)KZGPT_MAX_POINTS;

// element i of an Fr SoA array of stride n, mod r
BN_DEV Fp elem(const u64* a, size_t n, size_t i) { return fr_reduce_plain(load_plain(a, n, i, 0)); }

// ---- the weights -----------------------------------------------------------------------------------------------------------------------
// One lane per (row, point) pair: den_{j,i} = prod_{l != i} (z_{j,i} - z_{j,l}) mod r, the empty product of k = 1 being 1.  z, den: [4][mk].
__global__ void __launch_bounds__(BLOCK) k_kzgpt_denominators(const u64* zs, size_t k, size_t mk, u64* den) {
#pragma unroll 1
  for (size_t idx = TID; idx < mk; idx += (size_t)gridDim.x * BLOCK) {
    const size_t row0 = idx / k * k, i = idx - row0;
    const Fp zi = elem(zs, mk, idx);
    Fp d = fr_one();
#pragma unroll 1
    for (size_t l = 0; l < k; ++l)
      if (l != i) d = fr_mul(d, fr_sub(zi, elem(zs, mk, row0 + l)));
    store_plain(den, mk, idx, 0, d);
  }
}
// One lane per row: distinct_j = 1 iff no denominator of the row is 0, which is iff its k points are distinct mod r
__global__ void __launch_bounds__(BLOCK) k_kzgpt_distinct(const u64* den, size_t k, size_t m, uint8_t* distinct) {
#pragma unroll 1
  for (size_t j = TID; j < m; j += (size_t)gridDim.x * BLOCK) {
    bool ok = true;
#pragma unroll 1
    for (size_t i = 0; i < k; ++i) ok = ok && !fp_is_zero(load_plain(den, m * k, j * k + i, 0));
    distinct[j] = ok ? 1 : 0;
  }
}

// ---- the quotient ----------------------------------------------------------------------------------------------------------------------
// Pass 1 over (row, chunk) items, row = (polynomial j, point i) = j k + i: the chunk's value at its own base with a zero carry,
// T = sum_{e < CH} f_{c CH + e} z^e, into totals [4][items] at item = row chunks + c.  k_kzg_quot_totals of kzg_prove.hip with the polynomial of
// a row being row / k.
__global__ void __launch_bounds__(BLOCK) k_kzgpt_totals(const u64* coeffs, size_t len, size_t chunks, size_t items, const u64* zs, size_t k, size_t mk, u64* totals) {
  __shared__ u32 pw[LOG_BLOCK][8], part[BLOCK][8];
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t row = it / chunks, c = it - row * chunks;
    const u64* f = coeffs + row / k * 4 * len;
    const Fp z = elem(zs, mk, row);
    block_powers<LOG_L>(z, pw);
    const Fp v = lane_value(f, len, c * CH + (size_t)threadIdx.x * L, z);
    const Fp s = block_suffix<false>(v, pw, part, live_lanes(len, c));     // its first barrier publishes pw, its last one frees part and pw
    if (threadIdx.x == 0) store_plain(totals, items, it, 0, s);
  }
}
// The carry level, a block per row: H_c = T_c + z^CH H_{c + 1}, H_chunks = 0, walked from the top in tiles of BLOCK chunks.  carries [4][items]:
// slot c receives H_{c + 1}, the carry INTO chunk c.  y != NULL: H_0 = f(z) goes there.  The rows are independent: this is the single-point
// carry pass over m k rows.
__global__ void __launch_bounds__(BLOCK) k_kzgpt_carry(const u64* totals, size_t chunks, size_t items, const u64* zs, size_t mk, u64* carries, u64* y) {
  __shared__ u32 pw[LOG_BLOCK][8], part[BLOCK][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t row = blockIdx.x; row < mk; row += gridDim.x) {
    block_powers<LOG_L + LOG_BLOCK>(elem(zs, mk, row), pw);                  // pw[s] = z^(CH 2^s)
    __syncthreads();
    Fp run = fr_zero();
#pragma unroll 1
    for (size_t tile = (chunks + BLOCK - 1) / BLOCK; tile-- > 0;) {
      const size_t c = tile * BLOCK + t;
      Fp v = c < chunks ? load_plain(totals, items, row * chunks + c, 0) : fr_zero();
      if (t == BLOCK - 1 && c + 1 < chunks) v = fr_add(v, fr_mul(run, lds_get(pw, 0)));
      const size_t left = chunks - tile * BLOCK;
      const Fp s = block_suffix<true>(v, pw, part, left >= (size_t)BLOCK ? BLOCK : (int)left);
      if (c >= 1 && c < chunks) store_plain(carries, items, row * chunks + c - 1, 0, s);
      run = lds_get(part, 0);
      __syncthreads();                                       // every lane has read part[0] before the next tile overwrites it
    }
    if (y && t == 0) store_plain(y, mk, row, 0, run);
    __syncthreads();                                         // pw is free for the next row
  }
}
// The chunk of polynomial j, for ALL its k points -- the only launch after the weights when every polynomial is one chunk (carries == NULL).
// Per point i: lane values, the carry into the chunk through the top lane, the block scan, then each lane walks its L coefficients from the
// value above it, h_e = f_e + z_i h_{e + 1}, and adds a_i h_e into its accumulator of q_{e - 1}.  After the last point the lane stores its
// accumulators: the quotient is written once and no [m k][len] array exists.  The lane that owns the top coefficient writes q_{len - 1} = 0,
// lane 0 of chunk 0 writes y_i = h_0 per point.  q == NULL: evaluation only.  The L accumulators stay in registers (the walk is unrolled so
// that their indices are constants).  q must not overlap coeffs: other blocks still read what this one writes.
__global__ void __launch_bounds__(BLOCK) k_kzgpt_chunk(const u64* coeffs, size_t len, size_t chunks, size_t items, const u64* zs, const u64* ws, size_t k, size_t mk,
                                                       const u64* carries, u64* q, u64* y) {
  __shared__ u32 pw[LOG_BLOCK][8], part[BLOCK][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t j = it / chunks, c = it - j * chunks, a = c * CH + (size_t)t * L;
    const u64* f = coeffs + j * 4 * len;
    const int live = live_lanes(len, c);
    const bool carried = carries && c + 1 < chunks;           // block-uniform; such a chunk is full: its top lane owns coefficients
    Fp acc[L];
#pragma unroll
    for (int e = 0; e < L; ++e) acc[e] = fr_zero();
#pragma unroll 1
    for (size_t i = 0; i < k; ++i) {
      const size_t row = j * k + i;
      const Fp z = elem(zs, mk, row);
      block_powers<LOG_L>(z, pw);
      Fp v = lane_value(f, len, a, z);
      Fp cin = fr_zero();
      if (carried) {
        __syncthreads();                                     // pw[0] = z^L is published
        if (t == BLOCK - 1) {
          cin = load_plain(carries, mk * chunks, row * chunks + c, 0);
          v = fr_add(v, fr_mul(cin, lds_get(pw, 0)));
        }
      }
      const Fp s = block_suffix<true>(v, pw, part, live);
      if (y && c == 0 && t == 0) store_plain(y, mk, row, 0, s);
      if (q && a < len) {
        const Fp w = load_plain(ws, mk, row, 0);             // canonical: sylow_hip_fr_batch_inv wrote it
        Fp h = t + 1 < live ? lds_get(part, t + 1) : cin;    // h_{a + L}: the scan's value at the next lane, the chunk's carry above the top lane
#pragma unroll
        for (int e = L - 1; e >= 0; --e) {
          const size_t x = a + e;
          if (x < len) {
            h = fr_add(fr_mul(h, z), coeff(f, len, x));
            if (x) acc[e] = fr_add(acc[e], fr_mul(h, w));
          }
        }
      }
      __syncthreads();                                       // part and pw are free for the next point
    }
    if (q && a < len) {
      u64* qj = q + j * 4 * len;
#pragma unroll
      for (int e = L - 1; e >= 0; --e) {
        const size_t x = a + e;
        if (x >= len) continue;
        if (x == len - 1) store_plain(qj, len, x, 0, fr_zero());
        if (x) store_plain(qj, len, x - 1, 0, acc[e]);
      }
    }
  }
}

// ---- the verifier's Fr half ------------------------------------------------------------------------------------------------------------
// ONE wavefront per row, lane i on point i.  Z = prod (X - z_l) grows by one factor per step in LDS: lane t holds coefficient t, the leading 1 is
// implied.  Then every lane divides Z by (X - z_i) synthetically, b_{k-1} = 1, b_{e-1} = Z_e + z_i b_e, all lanes on the same e, and
// R_e = sum_i y_i a_i b_e is a tree over LDS: 2 k^2 products per row.  zs, ys, ws: [4][nk], ws canonical; zpoly [n][4][k+1], rpoly [n][4][k].
__global__ void __launch_bounds__(RB) k_kzgpt_polys(const u64* zs, const u64* ys, const u64* ws, size_t k, size_t n, u64* zpoly, u64* rpoly) {
  __shared__ u32 zl[MAXK][8], zc[MAXK][8], part[RB][8];
  const int t = threadIdx.x, kk = (int)k;
  const size_t nk = n * k;
#pragma unroll 1
  for (size_t row = blockIdx.x; row < n; row += gridDim.x) {
    const bool on = t < kk;
    const Fp zi = on ? elem(zs, nk, row * k + t) : fr_zero();
    if (on) lds_put(zl, t, zi);
    Fp cur = fr_zero();                                      // coefficient t of the product so far (below its leading 1)
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < kk; ++l) {                           // times (X - z_l): new_t = old_{t-1} - z_l old_t, old_l = 1
      if (t <= l) {
        const Fp below = t ? lds_get(zc, t - 1) : fr_zero();
        const Fp here = t == l ? fr_one() : cur;
        cur = fr_sub(below, fr_mul(lds_get(zl, l), here));
      }
      __syncthreads();                                       // every lane has read zc of the step before
      if (t <= l) lds_put(zc, t, cur);
      __syncthreads();
    }
    u64* zo = zpoly + row * 4 * (k + 1);
    if (on) store_plain(zo, k + 1, t, 0, cur);
    if (t == 0) store_plain(zo, k + 1, k, 0, fr_one());
    const Fp ci = on ? fr_mul(elem(ys, nk, row * k + t), load_plain(ws, nk, row * k + t, 0)) : fr_zero();
    Fp b = fr_one();
    u64* ro = rpoly + row * 4 * k;
#pragma unroll 1
    for (int e = kk - 1; e >= 0; --e) {
      lds_put(part, t, on ? fr_mul(ci, b) : fr_zero());
      __syncthreads();
#pragma unroll 1
      for (int off = RB / 2; off > 0; off >>= 1) {
        if (t < off) lds_put(part, t, fr_add(lds_get(part, t), lds_get(part, t + off)));
        __syncthreads();
      }
      if (t == 0) store_plain(ro, k, e, 0, lds_get(part, 0));
      if (on && e) b = fr_add(lds_get(zc, e), fr_mul(zi, b));
      __syncthreads();                                       // part is free for the next coefficient, zc and zl for the next row after the last
    }
  }
}

// ---- the verifier's small kernels ------------------------------------------------------------------------------------------------------
// The G2 sum of `rows` rows from j0 on, term-major (term i of row j0 + j at index i rows + j, what sylow_hip_g2_lincomb_batch reads): the
// scalar Z_{j0 + j, i} and the replicated base srs_g2[i], i <= k
__global__ void __launch_bounds__(BLOCK) k_kzgpt_g2_prep(const u64* zpoly, const u64* srs_g2, size_t k, size_t j0, size_t rows, u64* sc, u64* bases) {
  const size_t n = rows * (k + 1);
#pragma unroll 1
  for (size_t idx = TID; idx < n; idx += (size_t)gridDim.x * BLOCK) {
    const size_t i = idx / rows, j = idx - i * rows;
    store_plain(sc, n, idx, 0, load_plain(zpoly + (j0 + j) * 4 * (k + 1), k + 1, i, 0));
#pragma unroll
    for (int w = 0; w < 16; ++w) bases[(size_t)w * n + idx] = srs_g2[(size_t)w * (k + 1) + i];
  }
}
// rows G2 points of a [16][rows] array + flags to the columns j0 .. j0 + rows - 1 of out [16][n] + flags
__global__ void __launch_bounds__(BLOCK) k_kzgpt_put_g2(const u64* src, const uint8_t* src_inf, size_t rows, u64* out_xy, uint8_t* out_inf, size_t n, size_t j0) {
#pragma unroll 1
  for (size_t j = TID; j < rows; j += (size_t)gridDim.x * BLOCK) {
#pragma unroll
    for (int w = 0; w < 16; ++w) out_xy[(size_t)w * n + j0 + j] = src[(size_t)w * rows + j];
    out_inf[j0 + j] = src_inf[j];
  }
}
// The pair list of the n rows, SoA of stride 2n, and pair_offsets [n + 1]: pair 2j = (F_j, G2gen), pair 2j + 1 = (-pi_j, Z_j(tau) G2gen).  F and
// Z(tau) G2gen are canonical words of the library's own calls; pi is the caller's, its coordinate words reduced like Fp::new on the way.
__global__ void __launch_bounds__(BLOCK) k_kzgpt_pairs(const u64* f_xy, const uint8_t* f_inf, const u64* pi_xy, const uint8_t* pi_inf, const u64* zg_xy,
                                                       const uint8_t* zg_inf, size_t n, u64* p_xy, uint8_t* p_inf, u64* q_xy, uint8_t* q_inf, u64* offs) {
  const size_t s = 2 * n;
#pragma unroll 1
  for (size_t j = TID; j < n; j += (size_t)gridDim.x * BLOCK) {
#pragma unroll
    for (int w = 0; w < 8; ++w) p_xy[(size_t)w * s + 2 * j] = f_xy[(size_t)w * n + j];
    p_inf[2 * j] = f_inf[j];
    store_fp(p_xy, s, 2 * j + 1, 0, load_fp(pi_xy, n, j, 0));
    store_fp(p_xy, s, 2 * j + 1, 4, fp_neg(load_fp(pi_xy, n, j, 4)));
    p_inf[2 * j + 1] = pi_inf && pi_inf[j] ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) store_fp(q_xy, s, 2 * j, 4 * c, fp_const(C_G2_GEN[c]));
    q_inf[2 * j] = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) q_xy[(size_t)w * s + 2 * j + 1] = zg_xy[(size_t)w * n + j];
    q_inf[2 * j + 1] = zg_inf[j];
    offs[j] = 2 * j;
    if (j == n - 1) offs[n] = s;
  }
}
__global__ void __launch_bounds__(BLOCK) k_kzgpt_flags(const uint8_t* is_one, const uint8_t* distinct, size_t n, uint8_t* ok) {
#pragma unroll 1
  for (size_t j = TID; j < n; j += (size_t)gridDim.x * BLOCK) ok[j] = is_one[j] && distinct[j] ? 1 : 0;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
static dim3 lanes(size_t n) { return dim3((unsigned)lane_grid(n)); }
static dim3 blocks(size_t items) { return dim3((unsigned)block_grid(items)); }
static bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}
// den [4][mk] (scratch), a_out [4][mk], distinct_out [m] or NULL
static int32_t weights(const uint64_t* z, size_t k, size_t m, u64* den, uint64_t* a_out, uint8_t* distinct_out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t mk = m * k;
  k_kzgpt_denominators<<<lanes(mk), dim3(BLOCK), 0, st>>>(z, k, mk, den);
  const int32_t rc = sylow_hip_fr_batch_inv(den, a_out, mk, stream);
  if (rc == SYLOW_HIP_OK && distinct_out) k_kzgpt_distinct<<<lanes(m), dim3(BLOCK), 0, st>>>(den, k, m, distinct_out);
  return rc;
}
static int32_t quotient(const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z, size_t k, uint64_t* q_out, uint64_t* y_out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t mk = m * k, n_chunks = chunks(len), s_items = scan_items(len, m, k), c_items = chunk_items(len, m);
  host::Lease ws;
  const PointsQuotLayout l = points_quot_layout(len, m, k);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *den = ws.at<u64>(l.den), *a = ws.at<u64>(l.a), *totals = ws.at<u64>(l.totals), *carries = ws.at<u64>(l.carries);
  if (q_out) rc = weights(z, k, m, den, a, nullptr, stream);
  if (rc == SYLOW_HIP_OK) {
    if (!carry_levels(len)) {
      k_kzgpt_chunk<<<blocks(c_items), dim3(BLOCK), 0, st>>>(coeffs, len, n_chunks, c_items, z, a, k, mk, nullptr, q_out, y_out);
    } else {
      k_kzgpt_totals<<<blocks(s_items), dim3(BLOCK), 0, st>>>(coeffs, len, n_chunks, s_items, z, k, mk, totals);
      k_kzgpt_carry<<<blocks(mk), dim3(BLOCK), 0, st>>>(totals, n_chunks, s_items, z, mk, carries, y_out);
      if (q_out) k_kzgpt_chunk<<<blocks(c_items), dim3(BLOCK), 0, st>>>(coeffs, len, n_chunks, c_items, z, a, k, mk, carries, q_out, nullptr);
    }
  }
  return host::finish(rc, ws);
}
static int32_t polys(const uint64_t* z, const uint64_t* y, size_t k, size_t n, uint64_t* zpoly, uint64_t* rpoly, uint8_t* distinct, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  const PolysLayout l = polys_layout(n, k);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *den = ws.at<u64>(l.den), *a = ws.at<u64>(l.a);
  rc = weights(z, k, n, den, a, distinct, stream);
  if (rc == SYLOW_HIP_OK) k_kzgpt_polys<<<blocks(n), dim3(RB), 0, st>>>(z, y, a, k, n, zpoly, rpoly);
  return host::finish(rc, ws);
}
}  // namespace kzgpt

extern "C" {
int32_t sylow_hip_kzg_points_weights_batch(const uint64_t* z, size_t k, size_t m, uint64_t* a_out, uint8_t* distinct_out, void* stream) {
  using namespace kzgpt;
  ARGCHK(points_ok(k)); if (!m) return SYLOW_HIP_OK;
  ARGCHK(z && a_out);
  ARGCHK(weights_scratch_words(m, k) <= SAT / sizeof(u64));
  host::Lease ws;
  int32_t rc = ws.acquire(weights_scratch_bytes(m, k), (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  rc = weights(z, k, m, ws.at<u64>(0), a_out, distinct_out, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_quotient_points_batch(const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z, size_t k, uint64_t* q_out, uint64_t* y_out,
                                            void* stream) {
  using namespace kzgpt;
  ARGCHK(len > 0 && points_ok(k)); if (!m) return SYLOW_HIP_OK;
  ARGCHK(coeffs && z && (q_out || y_out));
  ARGCHK(poly_bytes(len, m) != SAT && quot_scratch_words(len, m, k) <= SAT / sizeof(u64));
  ARGCHK(!q_out || !ranges_overlap(coeffs, q_out, poly_bytes(len, m)));      // other blocks still read what this one writes
  return quotient(coeffs, len, m, z, k, q_out, y_out, stream);
}
int32_t sylow_hip_kzg_open_points_batch(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z, size_t k, uint64_t* y_out,
                                        uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  using namespace kzgpt;
  ARGCHK(len > 0 && points_ok(k)); if (!m) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && coeffs && z && y_out && pi_xy && pi_inf);
  ARGCHK(poly_bytes(len, m) != SAT && quot_scratch_words(len, m, k) <= SAT / sizeof(u64));
  host::Lease ws;
  int32_t rc = ws.acquire(poly_bytes(len, m), (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint64_t* q = ws.at<uint64_t>(0);
  rc = quotient(coeffs, len, m, z, k, q, y_out, stream);
  if (rc == SYLOW_HIP_OK) rc = kzgph::commit_canonical(srs_g1_xy, q, len, m, pi_xy, pi_inf, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_points_polys_batch(const uint64_t* z, const uint64_t* y, size_t k, size_t n, uint64_t* zpoly_out, uint64_t* rpoly_out, uint8_t* distinct_out,
                                         void* stream) {
  using namespace kzgpt;
  ARGCHK(points_ok(k)); if (!n) return SYLOW_HIP_OK;
  ARGCHK(z && y && zpoly_out && rpoly_out && distinct_out);
  ARGCHK(polys_scratch_words(n, k) <= SAT / sizeof(u64) && mul_sat(mul_sat(32, n), k + 1) != SAT);
  return polys(z, y, k, n, zpoly_out, rpoly_out, distinct_out, stream);
}
int32_t sylow_hip_kzg_verify_points_batch(const uint64_t* srs_g1_xy, const uint64_t* srs_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z,
                                          const uint64_t* y, size_t k, size_t n, const uint64_t* pi_xy, const uint8_t* pi_inf, uint8_t* ok, void* stream) {
  using namespace kzgpt;
  ARGCHK(points_ok(k)); if (!n) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && srs_g2_xy && c_xy && z && y && pi_xy && ok);
  const hipStream_t st = (hipStream_t)stream;
  const size_t lim = host::scratch_limit(), rows = g2_rows_per_chunk(n, k, lim ? lim : msmh::default_budget());
  const VerifyLayout v = verify_layout(n, k, rows);
  const size_t bytes = v.bytes;
  ARGCHK(bytes != SAT && polys_scratch_words(n, k) <= SAT / sizeof(u64));
  host::Lease ws;
  int32_t rc = ws.acquire(bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  const auto W = [&](size_t off) { return ws.at<u64>(off); };
  const auto B = [&](size_t off) { return ws.at<uint8_t>(off); };
  const bool direct = rows == n;                              // one chunk: the G2 sum writes [16][n] itself
  rc = polys(z, y, k, n, W(v.z), W(v.r), B(v.distinct), stream);
  if (rc == SYLOW_HIP_OK) rc = kzgph::commit_canonical(srs_g1_xy, W(v.r), k, n, W(v.rc), B(v.rc_inf), stream);      // R(tau) G1gen
  for (size_t j0 = 0; j0 < n && rc == SYLOW_HIP_OK; j0 += rows) {                                                        // Z(tau) G2gen
    const size_t rc_rows = n - j0 < rows ? n - j0 : rows;
    k_kzgpt_g2_prep<<<lanes(rc_rows * (k + 1)), dim3(BLOCK), 0, st>>>(W(v.z), srs_g2_xy, k, j0, rc_rows, W(v.sc), W(v.bases));
    rc = direct ? sylow_hip_g2_lincomb_batch(W(v.bases), nullptr, W(v.sc), W(v.zg), B(v.zg_inf), n, k + 1, stream)
                : sylow_hip_g2_lincomb_batch(W(v.bases), nullptr, W(v.sc), W(v.part), B(v.part_inf), rc_rows, k + 1, stream);
    if (rc == SYLOW_HIP_OK && !direct) k_kzgpt_put_g2<<<lanes(rc_rows), dim3(BLOCK), 0, st>>>(W(v.part), B(v.part_inf), rc_rows, W(v.zg), B(v.zg_inf), n, j0);
  }
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_sub_batch(c_xy, c_inf, W(v.rc), B(v.rc_inf), W(v.f), B(v.f_inf), n, stream);      // F = C - R(tau) G1gen
  if (rc == SYLOW_HIP_OK) {
    k_kzgpt_pairs<<<lanes(n), dim3(BLOCK), 0, st>>>(W(v.f), B(v.f_inf), pi_xy, pi_inf, W(v.zg), B(v.zg_inf), n, W(v.p), B(v.p_inf), W(v.q), B(v.q_inf),
                                                   W(v.offs));
    rc = sylow_hip_multi_pairing_batch(W(v.p), B(v.p_inf), W(v.q), B(v.q_inf), W(v.offs), n, 2 * n, /*skip_infinity=*/1, nullptr, B(v.is_one), stream);
  }
  if (rc == SYLOW_HIP_OK) k_kzgpt_flags<<<lanes(n), dim3(BLOCK), 0, st>>>(B(v.is_one), B(v.distinct), n, ok);
  return host::finish(rc, ws);
}
}  // extern "C"
