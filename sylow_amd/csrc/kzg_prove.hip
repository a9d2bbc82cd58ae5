// kzg_prove.hip -- the prover's half of KZG on BN254 under ONE SRS (include/sylow_hip.h, "KZG, the prover's side"): the quotient
//   q(X) = (f(X) - f(z)) / (X - z) and y = f(z) for m polynomials, as a scan in Fr (the new kernels of this unit); the commitment
//   sum_k f_k srs_k of m polynomials, composed from the library's own stream-ordered calls; and the opening (y, pi = commit(q)); the
//   commitment from values on a radix-2 domain is the inverse transform of ntt.hip in front of the same commitment.
// Geometry and routes: kzg_prove_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "kzg_scan_dev.hpp"

namespace kzgp {
using namespace kzg_scan;      // the scan's device routines and its geometry (kzg_prove_plan.hpp), shared with kzg_points.hip

// Pass 1 of a polynomial of several chunks: the chunk's value at its own base with a zero carry, T_c = sum_{i < CH} f_{c CH + i} z^i, into
// totals [4][items] at item = j chunks + c.  The grid is walked with a stride of whole blocks: every lane of a block sees the same items.
__global__ void __launch_bounds__(BLOCK) k_kzg_quot_totals(const u64* coeffs, size_t len, size_t chunks, size_t items, const u64* zs, size_t m, u64* totals) {
  __shared__ u32 pw[LOG_BLOCK][8], part[BLOCK][8];
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t j = it / chunks, c = it - j * chunks;
    const u64* f = coeffs + j * 4 * len;
    const Fp z = fr_reduce_plain(load_plain(zs, m, j, 0));
    block_powers<LOG_L>(z, pw);
    const Fp v = lane_value(f, len, c * CH + (size_t)threadIdx.x * L, z);
    const Fp s = block_suffix<false>(v, pw, part, live_lanes(len, c));     // its first barrier publishes pw, its last one frees part and pw
    if (threadIdx.x == 0) store_plain(totals, items, it, 0, s);
  }
}
// The carry level, a block per polynomial: H_c = T_c + z^CH H_{c + 1}, H_chunks = 0, walked from the top in tiles of BLOCK chunks; the running
// carry enters a tile through its top lane.  carries [4][items]: slot c receives H_{c + 1}, the carry INTO chunk c (the top chunk's is zero and
// its slot is never read).  y != NULL: H_0 = f(z) goes there -- the evaluation-only call ends here.
__global__ void __launch_bounds__(BLOCK) k_kzg_quot_carry(const u64* totals, size_t chunks, size_t items, const u64* zs, size_t m, u64* carries, u64* y) {
  __shared__ u32 pw[LOG_BLOCK][8], part[BLOCK][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t j = blockIdx.x; j < m; j += gridDim.x) {
    block_powers<LOG_L + LOG_BLOCK>(fr_reduce_plain(load_plain(zs, m, j, 0)), pw);       // pw[s] = z^(CH 2^s)
    __syncthreads();
    Fp run = fr_zero();
#pragma unroll 1
    for (size_t tile = (chunks + BLOCK - 1) / BLOCK; tile-- > 0;) {
      const size_t c = tile * BLOCK + t;
      Fp v = c < chunks ? load_plain(totals, items, j * chunks + c, 0) : fr_zero();
      if (t == BLOCK - 1 && c + 1 < chunks) v = fr_add(v, fr_mul(run, lds_get(pw, 0)));
      const size_t left = chunks - tile * BLOCK;
      const Fp s = block_suffix<true>(v, pw, part, left >= (size_t)BLOCK ? BLOCK : (int)left);
      if (c >= 1 && c < chunks) store_plain(carries, items, j * chunks + c - 1, 0, s);
      run = lds_get(part, 0);
      __syncthreads();                                       // every lane has read part[0] before the next tile overwrites it
    }
    if (y && t == 0) store_plain(y, m, j, 0, run);
  }
}
// The chunk itself -- the ONLY launch when every polynomial is one chunk (carries == NULL): lane values, the carry into the chunk through
// the top lane, the block scan, then each lane walks its L coefficients from the value above it, h_k = f_k + z h_{k + 1}, and stores h_k as
// q_{k - 1}; the lane that owns the top coefficient writes q_{len - 1} = 0, lane 0 of chunk 0 writes y = h_0.  q == NULL: evaluation only.
// The coefficients are read twice (the second time mostly from cache) instead of held: 8 more registers per coefficient would halve the
// occupancy.  q must not overlap coeffs: other blocks still read what this one writes.
__global__ void __launch_bounds__(BLOCK) k_kzg_quot_chunk(const u64* coeffs, size_t len, size_t chunks, size_t items, const u64* zs, size_t m, const u64* carries,
                                                          u64* q, u64* y) {
  __shared__ u32 pw[LOG_BLOCK][8], part[BLOCK][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t j = it / chunks, c = it - j * chunks, a = c * CH + (size_t)t * L;
    const u64* f = coeffs + j * 4 * len;
    const Fp z = fr_reduce_plain(load_plain(zs, m, j, 0));
    block_powers<LOG_L>(z, pw);
    Fp v = lane_value(f, len, a, z);
    const bool carried = carries && c + 1 < chunks;           // block-uniform; such a chunk is full: its top lane owns coefficients
    Fp cin = fr_zero();
    if (carried) {
      __syncthreads();                                       // pw[0] = z^L is published
      if (t == BLOCK - 1) {
        cin = load_plain(carries, items, it, 0);
        v = fr_add(v, fr_mul(cin, lds_get(pw, 0)));
      }
    }
    const int live = live_lanes(len, c);
    const Fp s = block_suffix<true>(v, pw, part, live);
    if (y && c == 0 && t == 0) store_plain(y, m, j, 0, s);
    if (q && a < len) {
      u64* qj = q + j * 4 * len;
      Fp h = t + 1 < live ? lds_get(part, t + 1) : cin;      // h_{a + L}: the scan's value at the next lane, the chunk's carry above the top lane
#pragma unroll 1
      for (int i = L - 1; i >= 0; --i) {
        const size_t k = a + i;
        if (k >= len) continue;
        if (k == len - 1) store_plain(qj, len, k, 0, fr_zero());
        h = fr_add(fr_mul(h, z), coeff(f, len, k));
        if (k) store_plain(qj, len, k - 1, 0, h);
      }
    }
    __syncthreads();                                         // part and pw are free for the next item
  }
}

// ---- the commitment's small kernels ----------------------------------------------------------------------------------------------------
// src [4][n] -> dst [4][n] mod r (the bucket route: sylow_hip_g1_msm reduces its scalars like Fp::new FIRST, which is another value for a
// word >= p; the KZG block's scalars are taken mod r)
__global__ void __launch_bounds__(BLOCK) k_kzg_reduce_scalars(const u64* src, u64* dst, size_t n) {
  const size_t i = TID;
  if (i < n) store_plain(dst, n, i, 0, fr_reduce_plain(load_plain(src, n, i, 0)));
}
// The short route's pairs, term-major: pair k mc + j holds f_{j0 + j, k} mod r and srs_k, for the mc polynomials from j0 on
__global__ void __launch_bounds__(BLOCK) k_kzg_commit_prep(const u64* srs, const u64* coeffs, size_t len, size_t j0, size_t mc, u64* sc, u64* bases) {
  const size_t i = TID, n = mc * len;
  if (i >= n) return;
  const size_t k = i / mc, j = i - k * mc;
  store_plain(sc, n, i, 0, coeff(coeffs + (j0 + j) * 4 * len, len, k));
#pragma unroll
  for (int w = 0; w < 8; ++w) bases[(size_t)w * n + i] = srs[(size_t)w * len + k];
}
// n points, word w of point j at src[w sw + j sj], to columns j0 .. j0 + n - 1 of out [8][m] + flags
__global__ void __launch_bounds__(BLOCK) k_kzg_gather_points(const u64* src, const uint8_t* src_inf, size_t sw, size_t sj, size_t n, u64* out_xy, uint8_t* out_inf,
                                                             size_t m, size_t j0) {
  const size_t j = TID;
  if (j >= n) return;
#pragma unroll
  for (int w = 0; w < 8; ++w) out_xy[(size_t)w * m + j0 + j] = src[(size_t)w * sw + j * sj];
  out_inf[j0 + j] = src_inf[j];
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
static int32_t quotient(const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z, uint64_t* q_out, uint64_t* y_out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t chunks = quot_chunks(len), items = quot_items(len, m);
  if (!quot_carry_levels(len)) {
    k_kzg_quot_chunk<<<dim3((unsigned)quot_grid(items)), dim3(BLOCK), 0, st>>>(coeffs, len, chunks, items, z, m, nullptr, q_out, y_out);
    LAUNCHED();
  }
  host::Lease ws;
  const QuotLayout l = quot_layout(len, m);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *totals = ws.at<u64>(l.totals), *carries = ws.at<u64>(l.carries);
  k_kzg_quot_totals<<<dim3((unsigned)quot_grid(items)), dim3(BLOCK), 0, st>>>(coeffs, len, chunks, items, z, m, totals);
  k_kzg_quot_carry<<<dim3((unsigned)quot_grid(m)), dim3(BLOCK), 0, st>>>(totals, chunks, items, z, m, carries, q_out ? nullptr : y_out);
  if (q_out) k_kzg_quot_chunk<<<dim3((unsigned)quot_grid(items)), dim3(BLOCK), 0, st>>>(coeffs, len, chunks, items, z, m, carries, q_out, y_out);
  return host::finish(SYLOW_HIP_OK, ws);
}

// one sylow_hip_g1_msm_tuned per polynomial into scratch, then one gather.  canonical: the coefficients are known to be below r (the opening's
// quotients), so polynomial j is passed as it lies
static int32_t commit_msm_each(const uint64_t* srs, const uint64_t* coeffs, size_t len, size_t m, bool canonical, int32_t window, int64_t min_n,
                               uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  const MsmEachLayout l = msm_each_layout(len, m, canonical);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *pts = ws.at<u64>(l.pts), *sc = ws.at<u64>(l.sc);
  uint8_t* inf = ws.at<uint8_t>(l.inf);
  for (size_t j = 0; j < m && rc == SYLOW_HIP_OK; ++j) {
    const u64* k = coeffs + j * 4 * len;
    if (!canonical) {
      k_kzg_reduce_scalars<<<GRID(len)>>>(k, sc, len);
      k = sc;
    }
    rc = sylow_hip_g1_msm_tuned(srs, nullptr, k, len, window, min_n, pts + 8 * j, inf + j, stream);
  }
  if (rc == SYLOW_HIP_OK) k_kzg_gather_points<<<GRID(m)>>>(pts, inf, 1, 8, m, out_xy, out_inf, m, 0);
  return host::finish(rc, ws);
}
static int32_t commit_short(const uint64_t* srs, const uint64_t* coeffs, size_t len, size_t m, size_t per_chunk, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t last = m % per_chunk;                         // a shorter last chunk may cut its segments into more slices
  const size_t w_a = g1h::sum_segments_scratch_words(per_chunk, len), w_b = last ? g1h::sum_segments_scratch_words(last, len) : 0, w_acc = w_a > w_b ? w_a : w_b;
  const bool direct = per_chunk == m;                        // one chunk: the segmented sum writes [8][m] itself
  host::Lease ws;
  const ShortLayout l = short_layout(len, per_chunk, w_acc, direct);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *sc = ws.at<u64>(l.sc), *bases = ws.at<u64>(l.bases), *prod = ws.at<u64>(l.prod), *acc = ws.at<u64>(l.acc), *part = ws.at<u64>(l.part);
  uint8_t *prod_inf = ws.at<uint8_t>(l.prod_inf), *part_inf = ws.at<uint8_t>(l.part_inf);
  for (size_t j0 = 0; j0 < m && rc == SYLOW_HIP_OK; j0 += per_chunk) {
    const size_t mc = m - j0 < per_chunk ? m - j0 : per_chunk, nc = mc * len;
    k_kzg_commit_prep<<<GRID(nc)>>>(srs, coeffs, len, j0, mc, sc, bases);
    rc = sylow_hip_g1_scalar_mul_batch(bases, nullptr, sc, prod, prod_inf, nc, stream);
    if (rc != SYLOW_HIP_OK) break;
    if (direct) {
      rc = g1h::sum_segments(prod, prod_inf, mc, len, acc, out_xy, out_inf, stream);
    } else {
      rc = g1h::sum_segments(prod, prod_inf, mc, len, acc, part, part_inf, stream);
      if (rc == SYLOW_HIP_OK) k_kzg_gather_points<<<GRID(mc)>>>(part, part_inf, mc, 1, mc, out_xy, out_inf, m, j0);
    }
  }
  return host::finish(rc, ws);
}
static int32_t commit(const uint64_t* srs, const uint64_t* coeffs, size_t len, size_t m, bool canonical, int32_t window, int64_t min_len,
                      uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  const size_t lim = host::scratch_limit();
  const CommitPlan plan = commit_plan(len, m, min_len < 0 ? msmh::g1_default_min() : (size_t)min_len, lim ? lim : msmh::default_budget());
  switch (plan.route) {
    case Route::BUCKET: return commit_msm_each(srs, coeffs, len, m, canonical, window, 0, out_xy, out_inf, stream);
    case Route::MSM_EACH: return commit_msm_each(srs, coeffs, len, m, canonical, -1, -1, out_xy, out_inf, stream);
    case Route::SHORT: break;
  }
  return commit_short(srs, coeffs, len, m, plan.polys_per_chunk, out_xy, out_inf, stream);
}
}  // namespace kzgp
int32_t kzgph::commit_canonical(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  return kzgp::commit(srs_g1_xy, coeffs, len, m, /*canonical=*/true, -1, -1, out_xy, out_inf, stream);
}

extern "C" {
int32_t sylow_hip_kzg_quotient_batch(const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z, uint64_t* q_out, uint64_t* y_out, void* stream) {
  ARGCHK(len > 0); if (!m) return SYLOW_HIP_OK;
  ARGCHK(coeffs && z && (q_out || y_out));
  return kzgp::quotient(coeffs, len, m, z, q_out, y_out, stream);
}
int32_t sylow_hip_kzg_commit_batch_tuned(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, int32_t window, int64_t min_len,
                                         uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  ARGCHK(len > 0 && msmh::window_ok(window)); if (!m) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && coeffs && out_xy && out_inf);
  return kzgp::commit(srs_g1_xy, coeffs, len, m, /*canonical=*/false, window, min_len, out_xy, out_inf, stream);
}
int32_t sylow_hip_kzg_commit_batch(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  return sylow_hip_kzg_commit_batch_tuned(srs_g1_xy, coeffs, len, m, -1, -1, out_xy, out_inf, stream);
}
int32_t sylow_hip_kzg_open_batch(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z,
                                 uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  ARGCHK(len > 0); if (!m) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && coeffs && z && y_out && pi_xy && pi_inf);
  host::Lease ws;
  int32_t rc = ws.acquire(kzg_plan::coeffs_bytes(len, m), (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint64_t* q = ws.at<uint64_t>(0);
  rc = kzgp::quotient(coeffs, len, m, z, q, y_out, stream);
  if (rc == SYLOW_HIP_OK) rc = kzgp::commit(srs_g1_xy, q, len, m, /*canonical=*/true, -1, -1, pi_xy, pi_inf, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_commit_evals_batch(const uint64_t* srs_g1_xy, const uint64_t* evals, int32_t log_n, size_t m, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  ARGCHK(log_n >= 0 && log_n <= 28); if (!m) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && evals && out_xy && out_inf);
  const size_t len = (size_t)1 << log_n;
  ARGCHK(m <= (size_t)-1 / (4 * sizeof(u64)) / len);
  host::Lease ws;
  int32_t rc = ws.acquire(kzg_plan::coeffs_bytes(len, m), (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint64_t* f = ws.at<uint64_t>(0);
  rc = sylow_hip_fr_ntt_batch(evals, log_n, m, /*inverse=*/1, nullptr, f, stream);      // the coefficients, canonical
  if (rc == SYLOW_HIP_OK) rc = kzgp::commit(srs_g1_xy, f, len, m, /*canonical=*/true, -1, -1, out_xy, out_inf, stream);
  return host::finish(rc, ws);
}
}  // extern "C"
