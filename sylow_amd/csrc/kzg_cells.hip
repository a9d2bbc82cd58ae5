// kzg_cells.hip -- many cells of many KZG blobs checked as ONE boolean over shared commitments (include/sylow_hip_kzg_cells.h).  Row k is
//   (cell i_k < c, commitment b_k < n_com, l values, proof pi_k, weight r_k), R_k the interpolant of its values, v = w^l:
//   e( sum_b W_b C_b - A(tau) G1gen + sum_k (r_k v^(i_k)) pi_k , G2gen ) e( -sum_k r_k pi_k , tau^l G2gen ) == 1,
//   W_b = sum_(k: b_k = b) r_k,   A = sum_k r_k R_k -- every sum taken in Fr before anything touches the curve.
// The Fr half: one launch per row, the rows grouped by key on the device (counts, starts, a permutation), W as a keyed sum, and A by
// columns -- S_i[j] = sum_(k: i_k = i) r_k val_k[j] by a keyed multiply-accumulate, ONE inverse transform of c arrays of l points, a Horner
// fold over i -- or by rows through the interpolation of kzg_cosets.hip and the linear combination of kzg_multi.hip.  The curve half is
// the library's own stream-ordered calls, as they stand.
// Route, keys, teams, staging, slices, chunks, grids and scratch: kzg_cells_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_acc.hpp"
#include "bn254_fr_dev.hpp"
#include "bn254_fr_roots.hpp"
#include "kzg_cells_plan.hpp"
#include "../../include/sylow_hip_kzg_cells.h"
#include "../../include/sylow_hip_kzg_cosets.h"

namespace kzce {
using namespace kzg_cells_plan;
static_assert(CELLS_BLOCK == BLOCK && (1 << CELLS_BLOCK_LOG) == BLOCK, "the kernels run blocks of BLOCK lanes");
static_assert(SYLOW_HIP_KZG_CELLS_LOG_N_MAX == CELLS_LOG_N_MAX, "the header's bound is the plan's");
static_assert(CELLS_LOG_N_MAX <= SYLOW_HIP_KZG_COSETS_LOG_N_MAX && CELLS_LOG_N_MAX <= ntt_plan::NTT_LOG_N_MAX, "the domains of the calls the fold makes");
typedef unsigned long long ull;
static_assert(sizeof(ull) == sizeof(u64), "the atomics take the counts as they are");

// One row per lane: the range test, the weight mod r, r v^i, the row's keys and their counts.  A row takes part when it is in range and
// its weight is not 0 mod r; one that is out of range with a live weight clears the flag (every such lane stores the same 0).
// r_out, rz_out [4][rows]; keys [entries]; cnt [n_keys], cleared before the launch; in_range [1], set before the launch.
__global__ void __launch_bounds__(BLOCK) k_cells_rows(const u64* idx, const u64* com_idx, const u64* weights, const u64* roots, int log_c, size_t rows, size_t n_com,
                                                      int route, u64* r_out, u64* rz_out, u64* keys, u64* cnt, uint8_t* in_range_flag) {
  const size_t lanes = (size_t)gridDim.x * BLOCK, none = n_keys(route, log_c, n_com), com0 = cell_keys(route, log_c), ce = cell_entries(route, rows);
#pragma unroll 1
  for (size_t k = TID; k < rows; k += lanes) {
    const u64 id = idx[k], cb = com_idx[k];
    const bool inside = in_range(id, log_c) && cb < n_com;
    const Fp w = fr_reduce_plain(load_plain(weights, rows, k, 0));
    const bool zero = fp_is_zero(w), part = inside && !zero;
    if (!inside && !zero) in_range_flag[0] = 0;
    store_plain(r_out, rows, k, 0, part ? w : fr_zero());
    store_plain(rz_out, rows, k, 0, part ? fr_mul(w, fr_root_from_half_table(roots, log_c, (size_t)id)) : fr_zero());
    if (route == ROUTE_COLUMNS) {
      keys[k] = part ? id : none;
      if (part) atomicAdd((ull*)cnt + id, 1ull);
    }
    keys[ce + k] = part ? com0 + cb : none;
    if (part) atomicAdd((ull*)cnt + com0 + cb, 1ull);
  }
}
// ONE block: start[i] = the sum of cnt below i for i <= n (the last is the number of grouped entries), next[i] = start[i], the cursors of
// the scatter.  Rounds of BLOCK counts, an inclusive scan of a round in LDS, the carry in a register that every lane holds.
__global__ void __launch_bounds__(BLOCK) k_cells_scan(const u64* cnt, size_t n, u64* start, u64* next) {
  __shared__ u64 part[BLOCK];
  const int t = threadIdx.x;
  u64 carry = 0;
#pragma unroll 1
  for (size_t round = 0; round < scan_rounds(n); ++round) {
    const size_t i = round * BLOCK + (size_t)t;
    const u64 v = i < n ? cnt[i] : 0;
    part[t] = v;
    __syncthreads();
#pragma unroll 1
    for (int off = 1; off < BLOCK; off <<= 1) {
      const u64 a = t >= off ? part[t - off] : 0;
      __syncthreads();
      part[t] += a;
      __syncthreads();
    }
    if (i < n) start[i] = next[i] = carry + part[t] - v;
    carry += part[BLOCK - 1];
    __syncthreads();                                          // the slots are free for the next round
  }
  if (t == 0) start[n] = carry;
}
// perm[cursor of the entry's key] = the entry's row.  THE ORDER INSIDE A GROUP IS WHATEVER THE ATOMICS GIVE: every sum over a group is
// exact in Fr, so no word of any output depends on it.
__global__ void __launch_bounds__(BLOCK) k_cells_scatter(const u64* keys, size_t total, size_t none, int route, size_t rows, u64* next, u64* perm) {
  const size_t lanes = (size_t)gridDim.x * BLOCK;
#pragma unroll 1
  for (size_t e = TID; e < total; e += lanes) {
    const u64 key = keys[e];
    if (key < none) perm[atomicAdd((ull*)next + key, 1ull)] = entry_row(e, route, rows);
  }
}

// The keyed multiply-accumulate over items (slice, tile of BLOCK flattened (key, column) pairs): lane t owns column `col` of key `key` and
// walks the slice of the key's group through the permutation.  The lanes of a key are a team; a group goes by in rounds of `stage` rows:
// the team's first lanes bring the round's row numbers and canonical weights (r_out) into the team's LDS slots, then every lane adds its
// products val[row][col] r_row UNREDUCED and folds before the accumulator could hold more than MAC_FLUSH of them.  THE BOUND
// (bn254_fr_acc.hpp): both factors are canonical -- a value is ANY word and is reduced at the load, r_out is canonical -- and a fold leaves a
// residue below r, so the accumulator stays below r + 16 r^2 < 2^512.  VALS = false: the factor is 1 (the sums W_b of the weights).
// The teams of a block have groups of different lengths: the block runs the rounds of its longest slice, so the barriers are reached by
// whole blocks.  A key without a row stores zeros.  Element (key, col) of slice s: out + s slice_words + key key_stride + col, words
// word_stride apart.
template <bool VALS>
__global__ void __launch_bounds__(BLOCK) k_cells_mac(const u64* vals, const u64* r, const u64* perm, const u64* start, size_t keys, int log_cols, size_t rows,
                                                     size_t tiles, size_t slices, size_t items, u64* out, size_t slice_w, size_t key_stride, size_t word_stride) {
  __shared__ u32 wl[BLOCK][8];
  __shared__ u64 rl[BLOCK];
  __shared__ ull longest;
  static_assert(sizeof(wl) + sizeof(rl) + sizeof(longest) == mac_lds_bytes(), "the plan prices this LDS");
  const int t = threadIdx.x, q = mac_team_lane(t, log_cols), slot0 = mac_slot(t, log_cols), stage = 1 << mac_stage_log(log_cols);
  const size_t cols = elems(log_cols);
#pragma unroll 1
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const size_t s = mac_slice(item, tiles), flat = mac_tile(item, tiles) * BLOCK + (size_t)t, key = mac_key(flat, log_cols), col = mac_col(flat, log_cols);
    const bool live = key < keys;
    size_t g0 = 0, g1 = 0;
    if (live) {
      const size_t b = start[key], len = start[key + 1] - b;
      g0 = b + slice_begin(len, s, slices);
      g1 = b + slice_begin(len, s + 1, slices);
    }
    if (t == 0) longest = 0;
    __syncthreads();
    if (q == 0 && g1 > g0) atomicMax(&longest, (ull)(g1 - g0));
    __syncthreads();
    const size_t most = longest;
    u32 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
    int pending = 0;
#pragma unroll 1
    for (size_t base = 0; base < most; base += (size_t)stage) {
      __syncthreads();                                        // the round before has read its slots
      if (q < stage && g0 + base + (size_t)q < g1) {
        const u64 row = perm[g0 + base + (size_t)q];
        rl[slot0 + q] = row;
        lds_put(wl, slot0 + q, load_plain(r, rows, row, 0));
      }
      __syncthreads();
      if (live && g0 + base < g1) {
        const int cnt = g1 - (g0 + base) < (size_t)stage ? (int)(g1 - (g0 + base)) : stage;
#pragma unroll 1
        for (int i = 0; i < cnt; ++i) {
          const Fp v = VALS ? fr_reduce_plain(load_plain(vals + (size_t)rl[slot0 + i] * FR_WORDS * cols, cols, col, 0)) : fr_one();
          mul_acc(acc, v, lds_get(wl, slot0 + i));
        }
        pending += cnt;
        if (mac_folds(pending, log_cols)) {
          const Fp f = fr_reduce_wide(acc);
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] = i < 8 ? f.v[i] : 0;
          pending = 0;
        }
      }
    }
    if (live) store_plain(out + s * slice_w + key * key_stride, word_stride, col, 0, fr_reduce_wide(acc));
    __syncthreads();                                          // `longest` is read: the next item resets it
  }
}
// element (key, col): the sum over the slices, into the array the next step reads
__global__ void __launch_bounds__(BLOCK) k_cells_join(const u64* part, size_t keys, int log_cols, size_t slices, size_t slice_w, size_t key_stride, size_t word_stride,
                                                      u64* out) {
  const size_t lanes = (size_t)gridDim.x * BLOCK, total = mac_flat(keys, log_cols);
#pragma unroll 1
  for (size_t flat = TID; flat < total; flat += lanes) {
    const size_t off = mac_key(flat, log_cols) * key_stride, col = mac_col(flat, log_cols);
    Fp a = load_plain(part + off, word_stride, col, 0);
#pragma unroll 1
    for (size_t s = 1; s < slices; ++s) a = fr_add(a, load_plain(part + s * slice_w + off, word_stride, col, 0));
    store_plain(out + off, word_stride, col, 0, a);
  }
}
// Item (t, lane q of 2^horner_lanes_log adjacent lanes): Horner over the chunk's a_i[t] from the top with g = w^(-t), times g^(the chunk's
// first i); the lanes of a t meet through shuffles and lane 0 stores A[t].  a [c][4][l] canonical (the transform wrote it); out [4][l].
// A wave holds whole items-of-a-t, and a wave past the last item holds none.
__global__ void __launch_bounds__(BLOCK) k_cells_horner(const u64* a, int log_c, int log_l, size_t items, u64* out) {
  const size_t l = elems(log_l), lanes = (size_t)gridDim.x * BLOCK, chunk = horner_chunk(log_c);
  // w_n by ntt_plan::root_squarings squarings, spelt out: behind a function the compiler closes this loop with the opposite branch
  Fp w = fp_from_limbs(BN_FR_ROOT28);
#pragma unroll 1
  for (int i = 0; i < ntt_plan::root_squarings(log_n(log_c, log_l)); ++i) w = fr_mul(w, w);
#pragma unroll 1
  for (size_t item = TID; item < items; item += lanes) {
    const size_t t = horner_t(item, log_c), q = horner_q(item, log_c), i0 = horner_first(q, log_c);
    const Fp g = fr_pow(w, horner_g_exp(t, log_c, log_l));
    Fp acc = fr_zero();
#pragma unroll 1
    for (size_t k = chunk; k-- > 0;) acc = fr_add(fr_mul(acc, g), load_plain(a + (i0 + k) * FR_WORDS * l, l, t, 0));
    acc = fr_mul(acc, fr_pow(w, horner_join_exp(t, q, log_c, log_l)));
#pragma unroll 1
    for (int off = 1; off < (1 << horner_lanes_log(log_c)); off <<= 1) acc = fr_add(acc, shfl_xor_fp(acc, off));
    if (q == 0) store_plain(out, l, t, 0, acc);
  }
}
// the n_com + rows terms of ONE multi-scalar multiplication: (W_b, C_b) then (r_k v^(i_k), pi_k), words and flags as given
__global__ void __launch_bounds__(BLOCK) k_cells_concat(const u64* w, const u64* cxy, const uint8_t* cinf, const u64* rz, const u64* pxy, const uint8_t* pinf,
                                                        size_t n_com, size_t rows, u64* sc, u64* bases, uint8_t* binf) {
  const size_t lanes = (size_t)gridDim.x * BLOCK, total = n_com + rows;
#pragma unroll 1
  for (size_t i = TID; i < total; i += lanes) {
    const bool com = i < n_com;
    const size_t j = com ? i : i - n_com, n = com ? n_com : rows;
    const u64 *s = com ? w : rz, *b = com ? cxy : pxy;
    const uint8_t* f = com ? cinf : pinf;
#pragma unroll
    for (int k = 0; k < (int)FR_WORDS; ++k) sc[(size_t)k * total + i] = s[(size_t)k * n + j];
#pragma unroll
    for (int k = 0; k < (int)G1_WORDS; ++k) bases[(size_t)k * total + i] = b[(size_t)k * n + j];
    binf[i] = (f && f[j]) ? 1 : 0;
  }
}
// The two pairs as one SoA pair list of stride 2: lane 0 writes (F, G2gen), lane 1 writes (-P, tau^l G2gen).
__global__ void __launch_bounds__(64) k_cells_pairs(const u64* f, const uint8_t* finf, const u64* p, const uint8_t* pinf_in, const u64* tau, u64* pxy, uint8_t* pinf,
                                                    u64* qxy, uint8_t* qinf) {
  const size_t i = TID;
  if (i >= 2) return;
  if (i == 0) store_closing_pair(0, load_fp(f, 1, 0, 0), load_fp(f, 1, 0, 4), finf[0] != 0, tau, pxy, pinf, qxy, qinf);
  else store_closing_pair(1, load_fp(p, 1, 0, 0), load_fp(p, 1, 0, 4), pinf_in[0] != 0, tau, pxy, pinf, qxy, qinf);
}
// is_one <- [Gt is the identity] AND the range flag; the flag itself where the caller wants it
__global__ void __launch_bounds__(64) k_cells_close(const uint8_t* one, const uint8_t* flag, uint8_t* is_one, uint8_t* in_range_out) {
  if (TID) return;
  if (is_one) is_one[0] = one[0] && flag[0] ? 1 : 0;
  if (in_range_out) in_range_out[0] = flag[0] ? 1 : 0;
}

template <bool VALS>
static void mac(const u64* vals, const u64* r, const u64* perm, const u64* start, size_t keys, int log_cols, size_t rows, long long max_blocks, u64* part, u64* out,
                size_t key_stride, size_t word_stride, hipStream_t st) {
  const size_t slices = mac_slices(keys, log_cols, rows), sw = slice_words(keys, log_cols);
  k_cells_mac<VALS><<<dim3((unsigned)mac_grid(keys, log_cols, slices, max_blocks)), dim3(BLOCK), 0, st>>>(
      vals, r, perm, start, keys, log_cols, rows, mac_tiles(keys, log_cols), slices, mac_items(keys, log_cols, slices), joins(slices) ? part : out, sw, key_stride, word_stride);
  if (joins(slices))
    k_cells_join<<<dim3((unsigned)join_grid(keys, log_cols, max_blocks)), dim3(BLOCK), 0, st>>>(part, keys, log_cols, slices, sw, key_stride, word_stride, out);
}

// the Fr half; rows > 0, the arguments checked
static int32_t fold(const uint64_t* idx, const uint64_t* com_idx, const uint64_t* vals, const uint64_t* weights, int log_c, int log_l, size_t rows, size_t n_com,
                    int route, long long max_blocks, uint64_t* w_out, uint64_t* a_out, uint64_t* r_out, uint64_t* rz_out, uint8_t* in_range_out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t nk = n_keys(route, log_c, n_com), ne = entries(route, rows), l = elems(log_l), c = elems(log_c);
  host::Lease ws;
  const FoldLayout lay = fold_layout(route, log_c, log_l, rows, n_com);
  int32_t rc = ws.acquire(lay.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *roots = ws.at<u64>(lay.roots), *keys = ws.at<u64>(lay.keys), *perm = ws.at<u64>(lay.perm), *cnt = ws.at<u64>(lay.cnt), *start = ws.at<u64>(lay.start),
      *next = ws.at<u64>(lay.next), *wpart = ws.at<u64>(lay.wpart), *body = ws.at<u64>(lay.body);
  if (hipMemsetAsync(in_range_out, 1, 1, st) != hipSuccess) rc = host::fail(hipGetLastError(), "setting the range flag");
  if (rc == SYLOW_HIP_OK && nk && hipMemsetAsync(cnt, 0, nk * sizeof(u64), st) != hipSuccess) rc = host::fail(hipGetLastError(), "clearing the counts");
  if (rc == SYLOW_HIP_OK && log_c >= 1) rc = ntth::build_table(log_c, roots, stream);
  if (rc != SYLOW_HIP_OK) return host::finish(rc, ws);
  k_cells_rows<<<dim3((unsigned)rows_grid(rows, max_blocks)), dim3(BLOCK), 0, st>>>(idx, com_idx, weights, roots, log_c, rows, n_com, route, r_out, rz_out, keys, cnt,
                                                                                   in_range_out);
  k_cells_scan<<<dim3(1), dim3(BLOCK), 0, st>>>(cnt, nk, start, next);
  k_cells_scatter<<<dim3((unsigned)scatter_grid(route, rows, max_blocks)), dim3(BLOCK), 0, st>>>(keys, ne, nk, route, rows, next, perm);
  if (n_com) mac<false>(nullptr, r_out, perm, start + cell_keys(route, log_c), n_com, 0, rows, max_blocks, wpart, w_out, w_key_stride(), w_word_stride(n_com), st);
  if (route == ROUTE_COLUMNS) {
    u64 *S = body, *a = ws.at<u64>(lay.a), *spart = ws.at<u64>(lay.spart);
    mac<true>(vals, r_out, perm, start, c, log_l, rows, max_blocks, spart, S, s_key_stride(log_l), s_word_stride(log_l), st);
    rc = sylow_hip_fr_ntt_batch(S, log_l, c, /*inverse=*/1, nullptr, a, stream);
    if (rc == SYLOW_HIP_OK)
      k_cells_horner<<<dim3((unsigned)horner_grid(log_c, log_l, max_blocks)), dim3(BLOCK), 0, st>>>(a, log_c, log_l, horner_items(log_c, log_l), a_out);
  } else {
    const uint64_t gs[2] = {0, rows};                          // one group: a host array, read before the call returns
    rc = sylow_hip_kzg_coset_interp_batch(vals, idx, log_c, log_l, rows, body, nullptr, stream);
    if (rc == SYLOW_HIP_OK) rc = sylow_hip_fr_lincomb_batch(body, l, rows, r_out, gs, 1, a_out, stream);   // a dropped row has the weight 0
  }
  return host::finish(rc, ws);
}

static bool sizes_ok(int log_c, int log_l, size_t rows, size_t n_com) {
  return vals_bytes(log_l, rows) != SAT && point_bytes(terms(rows, n_com)) != SAT && scratch_ok(fold_scratch_bytes(ROUTE_ROWS, log_c, log_l, rows, n_com)) &&
         scratch_ok(fold_scratch_bytes(ROUTE_COLUMNS, log_c, log_l, rows, n_com)) && scratch_ok(reduce_scratch_bytes(log_l, rows, n_com));
}
}  // namespace kzce

extern "C" {
int32_t sylow_hip_kzg_cells_fold_batch_tuned(const uint64_t* idx, const uint64_t* com_idx, const uint64_t* vals, const uint64_t* weights, int32_t log_c, int32_t log_l,
                                             size_t rows, size_t n_com, int32_t route, int64_t max_blocks, uint64_t* w_out, uint64_t* a_out, uint64_t* r_out,
                                             uint64_t* rz_out, uint8_t* in_range_out, void* stream) {
  using namespace kzg_cells_plan;
  ARGCHK(logs_ok(log_c, log_l) && route_ok(route) && max_blocks_ok(max_blocks));
  ARGCHK(a_out && in_range_out && (w_out || !n_com));
  ARGCHK(!rows || (idx && com_idx && vals && weights && r_out && rz_out));
  ARGCHK(kzce::sizes_ok(log_c, log_l, rows, n_com));
  const host::Range in[4] = {{(uintptr_t)idx, index_bytes(rows)}, {(uintptr_t)com_idx, index_bytes(rows)}, {(uintptr_t)vals, vals_bytes(log_l, rows)},
                             {(uintptr_t)weights, scalar_bytes(rows)}};
  const host::Range out[5] = {{(uintptr_t)w_out, scalar_bytes(n_com)}, {(uintptr_t)a_out, scalar_bytes(elems(log_l))}, {(uintptr_t)r_out, scalar_bytes(rows)},
                              {(uintptr_t)rz_out, scalar_bytes(rows)}, {(uintptr_t)in_range_out, 1}};
  ARGCHK(host::outputs_disjoint(in, out, disjoint_or_empty));
  if (!rows) {                                                 // no row: the sums are zero and the flag is set
    const hipStream_t st = (hipStream_t)stream;
    if (n_com) HIPCHK(hipMemsetAsync(w_out, 0, scalar_bytes(n_com), st));
    HIPCHK(hipMemsetAsync(a_out, 0, scalar_bytes(elems(log_l)), st));
    HIPCHK(hipMemsetAsync(in_range_out, 1, 1, st));
    return SYLOW_HIP_OK;
  }
  return kzce::fold(idx, com_idx, vals, weights, log_c, log_l, rows, n_com, route_of(route, log_c, rows), max_blocks, w_out, a_out, r_out, rz_out, in_range_out, stream);
}
int32_t sylow_hip_kzg_cells_fold_batch(const uint64_t* idx, const uint64_t* com_idx, const uint64_t* vals, const uint64_t* weights, int32_t log_c, int32_t log_l,
                                       size_t rows, size_t n_com, uint64_t* w_out, uint64_t* a_out, uint64_t* r_out, uint64_t* rz_out, uint8_t* in_range_out,
                                       void* stream) {
  return sylow_hip_kzg_cells_fold_batch_tuned(idx, com_idx, vals, weights, log_c, log_l, rows, n_com, -1, -1, w_out, a_out, r_out, rz_out, in_range_out, stream);
}
int32_t sylow_hip_kzg_cells_reduce_batch(const uint64_t* srs_g1_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* idx, const uint64_t* com_idx,
                                         const uint64_t* vals, const uint64_t* pi_xy, const uint8_t* pi_inf, const uint64_t* weights, int32_t log_c, int32_t log_l,
                                         size_t rows, size_t n_com, uint64_t* f_xy, uint8_t* f_inf, uint64_t* p_xy, uint8_t* p_inf, uint8_t* in_range_out,
                                         void* stream) {
  using namespace kzg_cells_plan;
  ARGCHK(logs_ok(log_c, log_l));
  ARGCHK(srs_g1_xy && f_xy && f_inf && p_xy && p_inf && in_range_out && (c_xy || !n_com));
  ARGCHK(!rows || (idx && com_idx && vals && pi_xy && weights));
  ARGCHK(kzce::sizes_ok(log_c, log_l, rows, n_com));
  const host::Range in[9] = {{(uintptr_t)srs_g1_xy, point_bytes(elems(log_l))}, {(uintptr_t)c_xy, point_bytes(n_com)}, {(uintptr_t)c_inf, n_com},
                             {(uintptr_t)idx, index_bytes(rows)}, {(uintptr_t)com_idx, index_bytes(rows)}, {(uintptr_t)vals, vals_bytes(log_l, rows)},
                             {(uintptr_t)pi_xy, point_bytes(rows)}, {(uintptr_t)pi_inf, rows}, {(uintptr_t)weights, scalar_bytes(rows)}};
  const host::Range out[5] = {{(uintptr_t)f_xy, point_bytes(1)}, {(uintptr_t)f_inf, 1}, {(uintptr_t)p_xy, point_bytes(1)}, {(uintptr_t)p_inf, 1}, {(uintptr_t)in_range_out, 1}};
  ARGCHK(host::outputs_disjoint(in, out, disjoint_or_empty));
  const hipStream_t st = (hipStream_t)stream;
  const size_t l = elems(log_l), total = terms(rows, n_com);
  host::Lease ws;
  const ReduceLayout lay = reduce_layout(log_l, rows, n_com);
  int32_t rc = ws.acquire(lay.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *w = ws.at<u64>(lay.w), *a = ws.at<u64>(lay.a), *r = ws.at<u64>(lay.r), *rz = ws.at<u64>(lay.rz), *sc = ws.at<u64>(lay.sc), *bases = ws.at<u64>(lay.bases),
      *m1 = ws.at<u64>(lay.m1), *at = ws.at<u64>(lay.at);
  uint8_t *binf = ws.at<uint8_t>(lay.binf), *m1inf = ws.at<uint8_t>(lay.m1inf), *atinf = ws.at<uint8_t>(lay.atinf);
  rc = sylow_hip_kzg_cells_fold_batch(idx, com_idx, vals, weights, log_c, log_l, rows, n_com, w, a, r, rz, in_range_out, stream);
  if (rc == SYLOW_HIP_OK && total)
    kzce::k_cells_concat<<<dim3((unsigned)grid(blocks_of(total), -1)), dim3(BLOCK), 0, st>>>(w, c_xy, c_inf, rz, pi_xy, pi_inf, n_com, rows, sc, bases, binf);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_msm(total ? bases : nullptr, binf, total ? sc : nullptr, total, m1, m1inf, stream);   // sum W_b C_b + sum (r_k v^i_k) pi_k
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_kzg_commit_batch(srs_g1_xy, a, l, 1, at, atinf, stream);                              // A(tau) G1gen
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_sub_batch(m1, m1inf, at, atinf, f_xy, f_inf, 1, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_msm(pi_xy, pi_inf, rows ? r : nullptr, rows, p_xy, p_inf, stream);                   // sum r_k pi_k
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_cells_verify_weighted(const uint64_t* srs_g1_xy, const uint64_t* tau_l_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* idx,
                                            const uint64_t* com_idx, const uint64_t* vals, const uint64_t* pi_xy, const uint8_t* pi_inf, const uint64_t* weights,
                                            int32_t log_c, int32_t log_l, size_t rows, size_t n_com, uint64_t* gt_out, uint8_t* is_one, uint8_t* in_range_out,
                                            void* stream) {
  using namespace kzg_cells_plan;
  ARGCHK(logs_ok(log_c, log_l));
  ARGCHK((gt_out || is_one) && srs_g1_xy && tau_l_g2_xy && (c_xy || !n_com));
  ARGCHK(!rows || (idx && com_idx && vals && pi_xy && weights));
  ARGCHK(kzce::sizes_ok(log_c, log_l, rows, n_com));
  const host::Range in[10] = {{(uintptr_t)srs_g1_xy, point_bytes(elems(log_l))}, {(uintptr_t)tau_l_g2_xy, G2_WORDS * sizeof(uint64_t)}, {(uintptr_t)c_xy, point_bytes(n_com)},
                              {(uintptr_t)c_inf, n_com}, {(uintptr_t)idx, index_bytes(rows)}, {(uintptr_t)com_idx, index_bytes(rows)},
                              {(uintptr_t)vals, vals_bytes(log_l, rows)}, {(uintptr_t)pi_xy, point_bytes(rows)}, {(uintptr_t)pi_inf, rows},
                              {(uintptr_t)weights, scalar_bytes(rows)}};
  const host::Range out[3] = {{(uintptr_t)gt_out, 48 * sizeof(uint64_t)}, {(uintptr_t)is_one, 1}, {(uintptr_t)in_range_out, 1}};
  ARGCHK(host::outputs_disjoint(in, out, disjoint_or_empty));
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  const VerifyLayout lay = verify_layout();
  int32_t rc = ws.acquire(lay.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *f = ws.at<u64>(lay.f), *p = ws.at<u64>(lay.p), *pxy = ws.at<u64>(lay.pxy), *qxy = ws.at<u64>(lay.qxy);
  uint8_t *finf = ws.at<uint8_t>(lay.finf), *pinf_one = ws.at<uint8_t>(lay.pinf_one), *pinf = ws.at<uint8_t>(lay.pinf), *qinf = ws.at<uint8_t>(lay.qinf),
          *flag = ws.at<uint8_t>(lay.flag), *one = ws.at<uint8_t>(lay.one);
  rc = sylow_hip_kzg_cells_reduce_batch(srs_g1_xy, c_xy, c_inf, idx, com_idx, vals, pi_xy, pi_inf, weights, log_c, log_l, rows, n_com, f, finf, p, pinf_one, flag, stream);
  if (rc == SYLOW_HIP_OK) {
    kzce::k_cells_pairs<<<1, 64, 0, st>>>(f, finf, p, pinf_one, tau_l_g2_xy, pxy, pinf, qxy, qinf);
    rc = sylow_hip_pairing_product_batch(pxy, pinf, qxy, qinf, 2, /*skip_infinity=*/1, gt_out, one, stream);
  }
  if (rc == SYLOW_HIP_OK) kzce::k_cells_close<<<1, 64, 0, st>>>(one, flag, is_one, in_range_out);
  return host::finish(rc, ws);
}
}  // extern "C"
