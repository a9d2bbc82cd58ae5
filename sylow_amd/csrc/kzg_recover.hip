// kzg_recover.hip -- a KZG polynomial of degree below n / 2 from ANY HALF of the c cells of its domain of n = c l points
//   (include/sylow_hip_kzg_recover.h).  With M the missing cells of a row, v = w^l and s = 5:
//   Z = prod_(i in M) (X^l - v^i) is a polynomial in X^l -- c values zd on the domain, c values zc on the coset s <w>, never n of either;
//   t = y zd (missing cells become 0), P = INTT(t) = f Z, e = NTT_s(P), q = e / zc, f = INTT_s(q); the upper half of f is the check.
// Per call: the constants, the table of v, the vanishing values, ONE sylow_hip_fr_batch_inv of m c elements, the mask product, three
// transforms with the division in place between them, the status reduction, and a fourth transform where the caller wants every cell.
// Rows that miss too many cells take no branch: their zd is zero, so is everything after it.
// Items, staging, grids and scratch: kzg_recover_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_dev.hpp"
#include "kzg_recover_plan.hpp"
#include "../../include/sylow_hip_kzg_recover.h"

namespace kzrc {
using namespace kzg_recover_plan;
static_assert(RECOVER_BLOCK == BLOCK && RECOVER_WAVES * RECOVER_WAVE == BLOCK, "the kernels run blocks of BLOCK lanes, waves of 64");
static_assert(SYLOW_HIP_KZG_RECOVER_LOG_C_MAX == RECOVER_LOG_C_MAX && SYLOW_HIP_KZG_RECOVER_LOG_N_MAX == RECOVER_LOG_N_MAX, "the header's bounds are the plan's");
static_assert(RECOVER_LOG_N_MAX <= ntt_plan::NTT_LOG_N_MAX, "the domains of the transform");
static_assert(VANISH_CHUNK == BLOCK, "a staging round takes one mask byte per lane");

// consts: s as the transforms read their shift, then s^l by log_l squarings -- one lane, once per call
__global__ void __launch_bounds__(BLOCK) k_recover_consts(int log_l, u64* consts) {
  if (TID) return;
  Fp s = fp_from_limbs((u32)RECOVER_COSET_SHIFT, 0, 0, 0, 0, 0, 0, 0);
  store_plain(consts + CONST_SHIFT, 1, 0, 0, s);
#pragma unroll 1
  for (int i = 0; i < log_l; ++i) s = fr_mul(s, s);
  store_plain(consts + CONST_SL, 1, 0, 0, s);
}

// Item (row, block of the row), 2^vanish_split_log adjacent lanes per k < c: zd[k] = prod_(i in M) (v^k - v^i) and
// zc[k] = prod_(i in M) (s^l v^k - v^i).  The block counts the row's missing cells first (the count is the status: too many, and the row is
// zd = 0, zc = 1 without a product); then the mask is walked in rounds of VANISH_CHUNK indices, the missing roots of a round compacted into
// LDS -- a ballot inside the wave, the waves' counts through LDS -- and lane `sub` of a k runs its two chains over the roots sub,
// sub + lanes, ... of the list; the partial products of a k meet through shuffles.  zd, zc: element (row, k) at z_row_off + k, words
// `stride` apart.
__global__ void __launch_bounds__(BLOCK) k_recover_vanish(const uint8_t* present, const u64* roots, const u64* consts, int log_c, size_t m, size_t items, u64* zd,
                                                          u64* zc, int packed, uint8_t* status) {
  __shared__ u32 list[VANISH_CHUNK][8];
  __shared__ u32 waves[RECOVER_WAVES];
  static_assert(sizeof(list) + sizeof(waves) == vanish_lds_bytes(), "the plan prices this LDS");
  const size_t c = elems(log_c), stride = z_word_stride(log_c, m, packed != 0);
  const int t = threadIdx.x, lane = t & (RECOVER_WAVE - 1), wv = t / RECOVER_WAVE;
  const Fp sl = load_plain(consts + CONST_SL, 1, 0, 0);
#pragma unroll 1
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const size_t row = vanish_row(item, log_c), k = vanish_k0(item, log_c) + vanish_lane_k(t, log_c);
    const u32 sub = (u32)vanish_lane_sub(t, log_c), split = 1u << vanish_split_log(log_c);
    const uint8_t* pr = present + row * c;
    u32 cnt = 0;
#pragma unroll 1
    for (size_t i = t; i < c; i += BLOCK) cnt += pr[i] ? 0u : 1u;
#pragma unroll
    for (int off = RECOVER_WAVE / 2; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) waves[wv] = cnt;
    __syncthreads();
    u32 missing = 0;
#pragma unroll
    for (int w = 0; w < RECOVER_WAVES; ++w) missing += waves[w];
    __syncthreads();                                          // the counts are read: the rounds reuse the slots
    const bool live = k < c, refused = missing > max_missing(log_c);      // refused: the same in every lane of the block
    if (vanish_k0(item, log_c) == 0 && t == 0) status[row] = refused ? 1 : 0;
    Fp pd = refused ? fr_zero() : fr_one(), pc = fr_one();
    if (!refused && missing) {
      const Fp a = live ? fr_root_from_half_table(roots, log_c, k) : fr_one(), b = fr_mul(sl, a);
#pragma unroll 1
      for (size_t round = 0; round < vanish_rounds(log_c); ++round) {
        const size_t i = round * VANISH_CHUNK + t;
        const bool miss = i < c && !pr[i];
        const unsigned long long bal = __ballot(miss);
        if (lane == 0) waves[wv] = (u32)__popcll(bal);
        __syncthreads();
        u32 base = 0, staged = 0;
#pragma unroll
        for (int w = 0; w < RECOVER_WAVES; ++w) {
          base += w < wv ? waves[w] : 0u;
          staged += waves[w];
        }
        if (miss) lds_put(list, (int)(base + (u32)__popcll(bal & (((unsigned long long)1 << lane) - 1))), fr_root_from_half_table(roots, log_c, i));
        __syncthreads();
#pragma unroll 1
        for (u32 j = sub; j < staged; j += split) {
          const Fp x = lds_get(list, (int)j);
          pd = fr_mul(pd, fr_sub(a, x));
          pc = fr_mul(pc, fr_sub(b, x));
        }
        __syncthreads();                                      // the list and the counts are free for the next round
      }
#pragma unroll 1
      for (int off = 1; off < (int)split; off <<= 1) {        // the lanes of a k are adjacent in one wave: every lane of it holds the product
        pd = fr_mul(pd, shfl_xor_fp(pd, off));
        pc = fr_mul(pc, shfl_xor_fp(pc, off));
      }
    }
    if (live && sub == 0) {
      store_plain(zd + z_row_off(row, log_c, packed != 0), stride, k, 0, pd);
      store_plain(zc + z_row_off(row, log_c, packed != 0), stride, k, 0, pc);
    }
  }
}

// t[r][i + c j] = y[r][i + c j] zd[r][i] over the m n elements, consecutive lanes on consecutive words; words of y >= r are reduced by the
// product, and those of a cell with zd = 0 are not read at all
__global__ void __launch_bounds__(BLOCK) k_recover_mask_mul(const u64* y, const u64* zd, u64* out, int log_c, int log_l, size_t m, size_t total) {
  const size_t n = elems(log_n(log_c, log_l)), stride = z_word_stride(log_c, m, true), lanes = (size_t)gridDim.x * BLOCK;
#pragma unroll 1
  for (size_t t = TID; t < total; t += lanes) {
    const size_t row = elem_row(t, log_c, log_l), col = elem_col(t, log_c, log_l);
    const Fp z = load_plain(zd + z_row_off(row, log_c, true), stride, elem_cell(col, log_c), 0);
    Fp v = fr_zero();
    if (!fp_is_zero(z)) v = fr_mul(load_plain(y + row * FR_WORDS * n, n, col, 0), z);
    store_plain(out + row * FR_WORDS * n, n, col, 0, v);
  }
}
// e[r][t] <- e[r][t] zci[r][t mod c], in place; e is canonical (a transform wrote it)
__global__ void __launch_bounds__(BLOCK) k_recover_div(u64* e, const u64* zci, int log_c, int log_l, size_t m, size_t total) {
  const size_t n = elems(log_n(log_c, log_l)), stride = z_word_stride(log_c, m, true), lanes = (size_t)gridDim.x * BLOCK;
#pragma unroll 1
  for (size_t t = TID; t < total; t += lanes) {
    const size_t row = elem_row(t, log_c, log_l), col = elem_col(t, log_c, log_l);
    const Fp z = load_plain(zci + z_row_off(row, log_c, true), stride, elem_cell(col, log_c), 0);
    store_plain(e + row * FR_WORDS * n, n, col, 0, fr_mul(load_plain(e + row * FR_WORDS * n, n, col, 0), z));
  }
}
// Item (row, chunk of the upper half): the OR of the words of the chunk's coefficients, a ballot per wave, the waves through LDS, and the
// block's first lane ORs a set bit into the row's flag word.  flags: u32 [m], cleared before the launch.
__global__ void __launch_bounds__(BLOCK) k_recover_status(const u64* coeffs, int log_c, int log_l, size_t items, u32* flags) {
  __shared__ u32 waves[RECOVER_WAVES];
  static_assert(sizeof(waves) == status_lds_bytes(), "the plan prices this LDS");
  const size_t n = elems(log_n(log_c, log_l)), half = status_half(log_c, log_l), chunks = status_row_chunks(log_c, log_l);
  const int t = threadIdx.x, lane = t & (RECOVER_WAVE - 1), wv = t / RECOVER_WAVE;
#pragma unroll 1
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const size_t row = item / chunks, base = (item - row * chunks) * STATUS_CHUNK + t;
    const u64* upper = coeffs + row * FR_WORDS * n + half;
    u64 acc = 0;
#pragma unroll
    for (int e = 0; e < STATUS_LANE_ELEMS; ++e) {
      const size_t k = base + (size_t)e * BLOCK;
      if (k < half) {
#pragma unroll
        for (int w = 0; w < (int)FR_WORDS; ++w) acc |= upper[(size_t)w * n + k];
      }
    }
    const bool any = __ballot(acc != 0) != 0;
    if (lane == 0) waves[wv] = any ? 1u : 0u;
    __syncthreads();
    if (t == 0) {
      u32 a = 0;
#pragma unroll
      for (int w = 0; w < RECOVER_WAVES; ++w) a |= waves[w];
      if (a) atomicOr(flags + row, 1u);
    }
    __syncthreads();                                          // the slots are free for the next item
  }
}
// a set flag is status 2; 0 and 1 stay as the vanishing kernel wrote them (a row of status 1 is all zero and never sets its flag)
__global__ void __launch_bounds__(BLOCK) k_recover_status_close(const u32* flags, uint8_t* status, size_t m) {
#pragma unroll 1
  for (size_t j = TID; j < m; j += (size_t)gridDim.x * BLOCK)
    if (flags[j]) status[j] = 2;
}

// the constants, the roots and the vanishing values: consts [CONST_WORDS], roots [root_words(log_c)], both scratch
static int32_t vanish(const uint8_t* present, int log_c, int log_l, size_t m, u64* consts, u64* roots, u64* zd, u64* zc, bool packed, uint8_t* status, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  k_recover_consts<<<dim3(1), dim3(RECOVER_WAVE), 0, st>>>(log_l, consts);
  if (log_c >= 1) {
    const int32_t rc = ntth::build_table(log_c, roots, stream);
    if (rc != SYLOW_HIP_OK) return rc;
  }
  k_recover_vanish<<<dim3((unsigned)vanish_grid(log_c, m)), dim3(BLOCK), 0, st>>>(present, roots, consts, log_c, m, vanish_items(log_c, m), zd, zc, packed ? 1 : 0, status);
  LAUNCHED();
}
static int32_t recover(const uint64_t* y, const uint8_t* present, int log_c, int log_l, size_t m, uint64_t* coeffs_out, uint64_t* y_out, uint8_t* status_out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const int L = log_n(log_c, log_l);
  host::Lease ws;
  const RecoverLayout l = recover_layout(log_c, log_l, m);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *consts = ws.at<u64>(l.v.consts), *roots = ws.at<u64>(l.v.roots), *zd = ws.at<u64>(l.zd), *zc = ws.at<u64>(l.zc), *zci = ws.at<u64>(l.zci);
  u32* flags = ws.at<u32>(l.flags);
  u64* buf = ws.at<u64>(l.buf);
  const u64* shift = consts + CONST_SHIFT;
  const size_t total = elem_items(log_c, log_l, m);
  const dim3 eg((unsigned)elem_grid(log_c, log_l, m));
  if (hipMemsetAsync(flags, 0, flag_words(m) * sizeof(u64), st) != hipSuccess) rc = host::fail(hipGetLastError(), "clearing the flags");
  if (rc == SYLOW_HIP_OK) rc = vanish(present, log_c, log_l, m, consts, roots, zd, zc, /*packed=*/true, status_out, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_fr_batch_inv(zc, zci, inv_elems(log_c, m), stream);
  if (rc == SYLOW_HIP_OK) {
    k_recover_mask_mul<<<eg, dim3(BLOCK), 0, st>>>(y, zd, buf, log_c, log_l, m, total);
    rc = sylow_hip_fr_ntt_batch(buf, L, m, /*inverse=*/1, nullptr, coeffs_out, stream);                  // P = f Z
  }
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_fr_ntt_batch(coeffs_out, L, m, /*inverse=*/0, shift, buf, stream);   // its values on the coset
  if (rc == SYLOW_HIP_OK) {
    k_recover_div<<<eg, dim3(BLOCK), 0, st>>>(buf, zci, log_c, log_l, m, total);
    rc = sylow_hip_fr_ntt_batch(buf, L, m, /*inverse=*/1, shift, coeffs_out, stream);                    // f from its coset values
  }
  if (rc == SYLOW_HIP_OK) {
    k_recover_status<<<dim3((unsigned)status_grid(log_c, log_l, m)), dim3(BLOCK), 0, st>>>(coeffs_out, log_c, log_l, status_items(log_c, log_l, m), flags);
    k_recover_status_close<<<dim3((unsigned)status_close_grid(m)), dim3(BLOCK), 0, st>>>(flags, status_out, m);
    if (y_out) rc = sylow_hip_fr_ntt_batch(coeffs_out, L, m, /*inverse=*/0, nullptr, y_out, stream);
  }
  return host::finish(rc, ws);
}
}  // namespace kzrc

extern "C" {
int32_t sylow_hip_kzg_recover_vanish_batch(const uint8_t* present, int32_t log_c, int32_t log_l, size_t m, uint64_t* zd_out, uint64_t* zc_out, uint8_t* status_out,
                                           void* stream) {
  using namespace kzg_recover_plan;
  ARGCHK(logs_ok(log_c, log_l));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(present && zd_out && zc_out && status_out);
  const size_t pb = present_bytes(log_c, m), zb = z_bytes(log_c, m), sb = status_bytes(m);
  ARGCHK(pb != SAT && zb != SAT);
  const host::Range in[1] = {{(uintptr_t)present, pb}};
  const host::Range out[3] = {{(uintptr_t)zd_out, zb}, {(uintptr_t)zc_out, zb}, {(uintptr_t)status_out, sb}};
  ARGCHK(host::outputs_disjoint(in, out, disjoint));
  host::Lease ws;
  const VanishLayout l = vanish_layout(log_c);
  int32_t rc = ws.acquire(l.bytes, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  rc = kzrc::vanish(present, log_c, log_l, m, ws.at<u64>(l.consts), ws.at<u64>(l.roots), zd_out, zc_out, /*packed=*/false, status_out, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_recover_batch(const uint64_t* y, const uint8_t* present, int32_t log_c, int32_t log_l, size_t m, uint64_t* coeffs_out, uint64_t* y_out,
                                    uint8_t* status_out, void* stream) {
  using namespace kzg_recover_plan;
  ARGCHK(logs_ok(log_c, log_l));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(y && present && coeffs_out && status_out);
  const size_t fb = fr_bytes(log_c, log_l, m), pb = present_bytes(log_c, m), sb = status_bytes(m);
  ARGCHK(fb != SAT && pb != SAT && scratch_ok(recover_scratch_bytes(log_c, log_l, m)));
  const host::Range in[2] = {{(uintptr_t)y, fb}, {(uintptr_t)present, pb}};
  const host::Range out[3] = {{(uintptr_t)coeffs_out, fb}, {(uintptr_t)y_out, fb}, {(uintptr_t)status_out, sb}};      // y_out may be NULL: it is skipped
  ARGCHK(host::outputs_disjoint(in, out, disjoint));
  return kzrc::recover(y, present, log_c, log_l, m, coeffs_out, y_out, status_out, stream);
}
}  // extern "C"
