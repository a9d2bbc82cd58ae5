// fr_scan.hip -- scans over Fr under + and *, the scan of a ratio num_i / den_i formed on the way, and PLONK's permutation grand product
// (include/sylow_hip_fr_scan.h):
//   sylow_hip_fr_scan_batch            out_j[k] = a_j[0] o .. o a_j[k] (or up to k - 1), and the row's total;
//   sylow_hip_fr_ratio_scan_batch      the exclusive scan of t_i = num_i den_i^-1, the chunk's denominators through ONE inversion;
//   sylow_hip_plonk_identity_batch     the columns k_j w^i;
//   sylow_hip_plonk_permutation_batch  z_0 = 1, z_(i+1) = z_i prod_j (w_j(i) + beta k_j w^i + gamma) / prod_j (w_j(i) + beta sigma_j(i) + gamma).
// Three stream-ordered phases and NO BLOCK WAITS FOR ANOTHER: the chunk-local scan and the chunk's total; one block per row over the totals,
// a tile at a time with the running value carried in a register; every element of a later chunk combined with its chunk's prefix.
// Geometry, tiles and scratch: fr_scan_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_block.hpp"
#include "fr_scan_plan.hpp"
#include "../../include/sylow_hip_fr_scan.h"

namespace frs {
using namespace fr_scan_plan;
static_assert(SCAN_BLOCK == BLOCK, "the kernels run one chunk per block of BLOCK lanes");
static_assert(SYLOW_HIP_PLONK_WIRES_MAX == PLONK_WIRES_MAX, "the header's bound is the plan's");
constexpr int L = SCAN_LANE_ELEMS;

// ---- phase 1 of the plain scan -------------------------------------------------------------------------------------------------------------
// Item (j, c).  A lane folds its L elements and keeps the L running values (registers: the loops are unrolled; an element past len adds
// nothing); block_prefix turns the lane totals into the value in front of every lane; out_k = that value o the lane's running value at k
// (inclusive) or at k - 1 (exclusive).  The chunk's total goes to totals [4][items]; totals NULL: the row has this chunk alone, and its
// total is the row's, for total_out [4][m] (may be NULL).
template <bool PRODUCT>
__global__ void __launch_bounds__(BLOCK) k_scan_local(const u64* a, size_t len, size_t n_chunks, size_t items, int exclusive, u64* out, u64* totals, u64* total_out,
                                                      size_t m) {
  __shared__ u32 buf[BLOCK][8];
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t j = item_row(it, n_chunks), c = item_chunk(it, n_chunks), base = lane_base(c, threadIdx.x);
    const u64* aj = a + j * FR_WORDS * len;
    u64* oj = out + j * FR_WORDS * len;
    Fp p[L];
    Fp run = fr_scan_identity<PRODUCT>();
#pragma unroll
    for (int i = 0; i < L; ++i) {
      if (base + i < len) run = fr_scan_op<PRODUCT>(run, elem(aj, len, base + i));
      p[i] = run;
    }
    Fp total;
    const Fp e = block_prefix<PRODUCT>(run, buf, live_lanes(len, c), total);
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const size_t k = base + i;
      if (k >= len) continue;
      const Fp q = exclusive ? (i ? p[i ? i - 1 : 0] : fr_scan_identity<PRODUCT>()) : p[i];
      store_plain(oj, len, k, 0, fr_scan_op<PRODUCT>(e, q));
    }
    if (threadIdx.x == 0) {
      if (totals) store_plain(totals, items, it, 0, total);
      else if (total_out) store_plain(total_out, m, j, 0, total);
    }
    __syncthreads();                                         // buf is free for the next chunk
  }
}

// ---- phase 1 of the ratio scan: the shared inversion fused with the scan ------------------------------------------------------------------
// Item (j, c).  Forward, a lane multiplies its L denominators together and keeps the L prefix products; a denominator = 0 mod r enters the
// chain as 1, an element past len too.  block_inverses (bn254_fr_block.hpp, the chunk's ONE inversion, as k_fr_batch_inv) turns the lane
// totals into their inverses.  Backward, den_i^-1 = run p_(i-1) and run *= den_i, the denominators read a second time, and the slot of the
// prefix product that is no longer needed takes the ratio t_i = num_i den_i^-1 (0 for a zero denominator).  Then the plain scan's steps
// over the ratios in registers: the lane's running values, block_prefix, out_k = the value in front of the lane o the running value at
// k - 1.  zflag [items]: a denominator of the chunk was 0.  totals NULL: the row has this chunk alone; its total goes to total_out (may be
// NULL) and its status to status [m], bit 1 with `closing` when the total is not 1.
template <bool PRODUCT>
__global__ void __launch_bounds__(BLOCK) k_ratio_local(const u64* num, const u64* den, size_t len, size_t n_chunks, size_t items, u64* out, u64* totals,
                                                       uint8_t* zflag, u64* total_out, uint8_t* status, size_t m, int closing) {
  __shared__ u32 pre[BLOCK][8], suf[BLOCK][8], inv[1][8];
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t j = item_row(it, n_chunks), c = item_chunk(it, n_chunks), base = lane_base(c, threadIdx.x);
    const u64 *nj = num ? num + j * FR_WORDS * len : nullptr, *dj = den + j * FR_WORDS * len;
    u64* oj = out + j * FR_WORDS * len;
    const int live = live_lanes(len, c);
    Fp p[L];
    Fp run = fr_one();
    int any_zero = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      if (base + i < len) {
        const Fp v = elem(dj, len, base + i);
        if (fp_is_zero(v)) any_zero = 1;
        else run = fr_mul(run, v);
      }
      p[i] = run;
    }
    Fp r = block_inverses(run, pre, suf, inv, live);
#pragma unroll
    for (int i = L - 1; i >= 0; --i) {
      const size_t k = base + i;
      if (k >= len) {
        p[i] = fr_scan_identity<PRODUCT>();
        continue;
      }
      const Fp v = elem(dj, len, k);
      const bool zero = fp_is_zero(v);
      const Fp o = i ? fr_mul(r, p[i ? i - 1 : 0]) : r;
      if (i && !zero) r = fr_mul(r, v);
      p[i] = zero ? fr_zero() : nj ? fr_mul(elem(nj, len, k), o) : o;
    }
    any_zero = __syncthreads_or(any_zero);                    // and pre, suf and inv are free for the scan
    run = fr_scan_identity<PRODUCT>();
#pragma unroll
    for (int i = 0; i < L; ++i) {
      run = fr_scan_op<PRODUCT>(run, p[i]);
      p[i] = run;
    }
    Fp total;
    const Fp e = block_prefix<PRODUCT>(run, pre, live, total);
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const size_t k = base + i;
      if (k >= len) continue;
      store_plain(oj, len, k, 0, i ? fr_scan_op<PRODUCT>(e, p[i ? i - 1 : 0]) : e);
    }
    if (threadIdx.x == 0) {
      if (totals) {
        store_plain(totals, items, it, 0, total);
        zflag[it] = any_zero ? 1 : 0;
      } else {
        if (total_out) store_plain(total_out, m, j, 0, total);
        status[j] = (uint8_t)((any_zero ? STATUS_ZERO_DEN : 0) | (closing && !fp_eq(total, fr_one()) ? STATUS_NOT_CLOSED : 0));
      }
    }
    __syncthreads();                                         // pre is free for the next chunk
  }
}

// ---- phase 2: a block per row ----------------------------------------------------------------------------------------------------------------
// The row's n_chunks totals go by `tile` at a time, a lane per total: block_prefix over the tile, every slot rewritten IN PLACE as the
// prefix of its chunk (the carry o the totals in front of it in the tile), and the carry, which every lane holds, takes the tile's total.
// At the end the carry is the row's total: total_out (may be NULL); status (NULL for the plain scan) from the chunks' zero flags and, with
// `closing`, from total != 1.
template <bool PRODUCT>
__global__ void __launch_bounds__(BLOCK) k_scan_totals(u64* totals, size_t n_chunks, size_t items, size_t m, int tile, u64* total_out, const uint8_t* zflag,
                                                       int closing, uint8_t* status) {
  __shared__ u32 buf[BLOCK][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t j = blockIdx.x; j < m; j += gridDim.x) {
    Fp carry = fr_scan_identity<PRODUCT>();
    int any_zero = 0;
#pragma unroll 1
    for (size_t step = 0; step < tile_steps(n_chunks, tile); ++step) {
      const size_t first = tile_first(step, tile), slot = j * n_chunks + first + (size_t)t;
      const int cnt = tile_count(n_chunks, first, tile);
      Fp T = fr_scan_identity<PRODUCT>();
      if (t < cnt) {
        T = load_plain(totals, items, slot, 0);
        if (zflag && zflag[slot]) any_zero = 1;
      }
      Fp total;
      const Fp e = block_prefix<PRODUCT>(T, buf, cnt, total);
      if (t < cnt) store_plain(totals, items, slot, 0, fr_scan_op<PRODUCT>(carry, e));
      carry = fr_scan_op<PRODUCT>(carry, total);
      __syncthreads();                                       // buf is free for the next tile
    }
    if (status) {
      any_zero = __syncthreads_or(any_zero);
      if (t == 0) status[j] = (uint8_t)((any_zero ? STATUS_ZERO_DEN : 0) | (closing && !fp_eq(carry, fr_one()) ? STATUS_NOT_CLOSED : 0));
    }
    if (t == 0 && total_out) store_plain(total_out, m, j, 0, carry);
  }
}

// ---- phase 3: item (j, c >= 1): out_k = the chunk's prefix o out_k over the chunk, lanes BLOCK apart ------------------------------------------
template <bool PRODUCT>
__global__ void __launch_bounds__(BLOCK) k_scan_apply(const u64* prefixes, size_t len, size_t n_chunks, size_t items, size_t work, u64* out) {
#pragma unroll 1
  for (size_t it = blockIdx.x; it < work; it += gridDim.x) {
    const size_t j = apply_row(it, n_chunks), c = apply_chunk(it, n_chunks);
    u64* oj = out + j * FR_WORDS * len;
    const Fp pre = load_plain(prefixes, items, j * n_chunks + c, 0);
#pragma unroll 2
    for (int i = 0; i < L; ++i) {
      const size_t k = apply_elem(c, i, threadIdx.x);
      if (k < len) store_plain(oj, len, k, 0, fr_scan_op<PRODUCT>(pre, load_plain(oj, len, k, 0)));
    }
  }
}

// ---- PLONK -----------------------------------------------------------------------------------------------------------------------------------
// flat (column, element) pairs, a lane each: out_j[i] = shifts_j w^i, w^i one load from the table of the transform of n points
__global__ void __launch_bounds__(BLOCK) k_plonk_identity(const u64* shifts, const u64* roots, int log_n, int wires, size_t tiles, u64* out) {
  const size_t n = elems(log_n), total = n * (size_t)wires;
#pragma unroll 1
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t flat = tile * BLOCK + threadIdx.x;
    if (flat >= total) continue;
    const size_t j = flat >> log_n, i = flat & (n - 1);
    store_plain(out + j * FR_WORDS * n, n, i, 0, fr_mul(elem(shifts, (size_t)wires, j), fr_root_from_half_table(roots, log_n, i)));
  }
}
// Item (instance s, tile of BLOCK elements), a lane per element i:  num_i = prod_j (w_j(i) + gamma + (beta k_j) w^i)  and
// den_i = prod_j (w_j(i) + gamma + beta sigma_j(i))  into num, den [m][4][n].  The lanes below `wires` form beta k_j once per item, through
// LDS; w^i is one load from the table.  Four products per column and element.
__global__ void __launch_bounds__(BLOCK) k_plonk_terms(const u64* wires_in, const u64* sigma, const u64* shifts, const u64* beta, const u64* gamma, const u64* roots,
                                                       int log_n, int wires, size_t m, size_t tiles, size_t items, u64* num, u64* den) {
  __shared__ u32 bk[PLONK_WIRES_MAX][8];
  const size_t n = elems(log_n);
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t s = it / tiles, i = (it - s * tiles) * BLOCK + (size_t)t;
    const Fp b = elem(beta, m, s), g = elem(gamma, m, s);
    __syncthreads();                                         // the item before has read bk
    if (t < wires) lds_put(bk, t, fr_mul(b, elem(shifts, (size_t)wires, (size_t)t)));
    __syncthreads();
    if (i >= n) continue;                                    // the barriers above are reached by whole blocks: `it` is the block's
    const Fp x = fr_root_from_half_table(roots, log_n, i);
    Fp nu = fr_one(), de = fr_one();
#pragma unroll 1
    for (int j = 0; j < wires; ++j) {
      const Fp wv = fr_add(elem(wires_in + (s * (size_t)wires + (size_t)j) * FR_WORDS * n, n, i), g);
      nu = fr_mul(nu, fr_add(wv, fr_mul(lds_get(bk, j), x)));
      de = fr_mul(de, fr_add(wv, fr_mul(b, elem(sigma + (size_t)j * FR_WORDS * n, n, i))));
    }
    store_plain(num + s * FR_WORDS * n, n, i, 0, nu);
    store_plain(den + s * FR_WORDS * n, n, i, 0, de);
  }
}

// ---- launchers: len > 0, m > 0, the arguments checked ----------------------------------------------------------------------------------------
// phases 2 and 3 over the totals phase 1 left; zflag and status NULL for the plain scan
template <bool PRODUCT>
static void upper(u64* totals, const uint8_t* zflag, size_t len, size_t m, long long max_blocks, int tile, int closing, u64* out, u64* total_out, uint8_t* status,
                  hipStream_t st) {
  const size_t n_chunks = chunks(len), its = items(len, m), work = apply_items(len, m);
  k_scan_totals<PRODUCT><<<dim3((unsigned)totals_grid(m, max_blocks)), dim3(BLOCK), 0, st>>>(totals, n_chunks, its, m, tile, total_out, zflag, closing, status);
  k_scan_apply<PRODUCT><<<dim3((unsigned)grid(work, max_blocks)), dim3(BLOCK), 0, st>>>(totals, len, n_chunks, its, work, out);
}
template <bool PRODUCT>
static int32_t scan(const u64* a, size_t len, size_t m, int exclusive, long long max_blocks, int tile, u64* out, u64* total_out, hipStream_t st) {
  const size_t n_chunks = chunks(len), its = items(len, m);
  const dim3 per_item((unsigned)grid(its, max_blocks));
  if (!upper_phases(len)) {
    k_scan_local<PRODUCT><<<per_item, dim3(BLOCK), 0, st>>>(a, len, n_chunks, its, exclusive, out, nullptr, total_out, m);
    LAUNCHED();
  }
  host::Lease ws;
  const ScanLayout l = scan_layout(len, m, false);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* totals = ws.at<u64>(l.totals);
  k_scan_local<PRODUCT><<<per_item, dim3(BLOCK), 0, st>>>(a, len, n_chunks, its, exclusive, out, totals, nullptr, m);
  upper<PRODUCT>(totals, nullptr, len, m, max_blocks, tile, 0, out, total_out, nullptr, st);
  return host::finish(SYLOW_HIP_OK, ws);
}
template <bool PRODUCT>
static int32_t ratio_scan(const u64* num, const u64* den, size_t len, size_t m, long long max_blocks, int tile, int closing, u64* out, u64* total_out, uint8_t* status,
                          hipStream_t st) {
  const size_t n_chunks = chunks(len), its = items(len, m);
  const dim3 per_item((unsigned)grid(its, max_blocks));
  if (!upper_phases(len)) {
    k_ratio_local<PRODUCT><<<per_item, dim3(BLOCK), 0, st>>>(num, den, len, n_chunks, its, out, nullptr, nullptr, total_out, status, m, closing);
    LAUNCHED();
  }
  host::Lease ws;
  const ScanLayout l = scan_layout(len, m, true);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* totals = ws.at<u64>(l.totals);
  uint8_t* zflag = ws.at<uint8_t>(l.zflag);
  k_ratio_local<PRODUCT><<<per_item, dim3(BLOCK), 0, st>>>(num, den, len, n_chunks, its, out, totals, zflag, nullptr, nullptr, m, closing);
  upper<PRODUCT>(totals, zflag, len, m, max_blocks, tile, closing, out, total_out, status, st);
  return host::finish(SYLOW_HIP_OK, ws);
}
}  // namespace frs

extern "C" {
int32_t sylow_hip_fr_scan_batch_tuned(const uint64_t* a, size_t len, size_t m, int32_t op, int32_t exclusive, int64_t max_blocks, int32_t totals_tile, uint64_t* out,
                                      uint64_t* total_out, void* stream) {
  using namespace fr_scan_plan;
  ARGCHK(len && op_ok(op) && flag_ok(exclusive) && max_blocks_ok(max_blocks) && tile_ok(totals_tile));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(a && out);
  ARGCHK(rows_bytes(len, m) != SAT && scalars_bytes(m) != SAT && scratch_ok(scan_scratch_bytes(len, m, false)));
  const host::Range in[1] = {{(uintptr_t)a, rows_bytes(len, m)}};
  const host::Range outs[2] = {{(uintptr_t)out, rows_bytes(len, m)}, {(uintptr_t)total_out, scalars_bytes(m)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  return op == OP_PRODUCT ? frs::scan<true>(a, len, m, exclusive, max_blocks, tile_of(totals_tile), out, total_out, st)
                          : frs::scan<false>(a, len, m, exclusive, max_blocks, tile_of(totals_tile), out, total_out, st);
}
int32_t sylow_hip_fr_scan_batch(const uint64_t* a, size_t len, size_t m, int32_t op, int32_t exclusive, uint64_t* out, uint64_t* total_out, void* stream) {
  return sylow_hip_fr_scan_batch_tuned(a, len, m, op, exclusive, -1, -1, out, total_out, stream);
}
int32_t sylow_hip_fr_ratio_scan_batch_tuned(const uint64_t* num, const uint64_t* den, size_t len, size_t m, int32_t op, int64_t max_blocks, int32_t totals_tile,
                                            uint64_t* out, uint64_t* total_out, uint8_t* status, void* stream) {
  using namespace fr_scan_plan;
  ARGCHK(len && op_ok(op) && max_blocks_ok(max_blocks) && tile_ok(totals_tile));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(den && out && status);
  ARGCHK(rows_bytes(len, m) != SAT && scalars_bytes(m) != SAT && scratch_ok(scan_scratch_bytes(len, m, true)));
  const host::Range in[2] = {{(uintptr_t)num, rows_bytes(len, m)}, {(uintptr_t)den, rows_bytes(len, m)}};
  const host::Range outs[3] = {{(uintptr_t)out, rows_bytes(len, m)}, {(uintptr_t)total_out, scalars_bytes(m)}, {(uintptr_t)status, m}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  return op == OP_PRODUCT ? frs::ratio_scan<true>(num, den, len, m, max_blocks, tile_of(totals_tile), 0, out, total_out, status, st)
                          : frs::ratio_scan<false>(num, den, len, m, max_blocks, tile_of(totals_tile), 0, out, total_out, status, st);
}
int32_t sylow_hip_fr_ratio_scan_batch(const uint64_t* num, const uint64_t* den, size_t len, size_t m, int32_t op, uint64_t* out, uint64_t* total_out, uint8_t* status,
                                      void* stream) {
  return sylow_hip_fr_ratio_scan_batch_tuned(num, den, len, m, op, -1, -1, out, total_out, status, stream);
}
int32_t sylow_hip_plonk_identity_batch(const uint64_t* shifts, int32_t log_n, int32_t W, uint64_t* out, void* stream) {
  using namespace fr_scan_plan;
  ARGCHK(plonk_ok(log_n, W));
  ARGCHK(shifts && out);
  ARGCHK(identity_bytes(log_n, W) != SAT && scratch_ok(identity_scratch_bytes(log_n)));
  const host::Range in[1] = {{(uintptr_t)shifts, scalars_bytes((size_t)W)}};
  const host::Range outs[1] = {{(uintptr_t)out, identity_bytes(log_n, W)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  int32_t rc = ws.acquire(identity_scratch_bytes(log_n), st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* roots = ws.at<u64>(0);
  if (log_n >= 1) rc = ntth::build_table(log_n, roots, stream);
  if (rc == SYLOW_HIP_OK) {
    const size_t tiles = identity_items(log_n, W);
    frs::k_plonk_identity<<<dim3((unsigned)grid(tiles, -1)), dim3(BLOCK), 0, st>>>(shifts, roots, log_n, W, tiles, out);
  }
  return host::finish(rc, ws);
}
int32_t sylow_hip_plonk_permutation_batch_tuned(const uint64_t* wires, const uint64_t* sigma, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma,
                                                int32_t log_n, int32_t W, size_t m, int64_t max_blocks, int32_t totals_tile, uint64_t* z_out, uint64_t* total_out,
                                                uint8_t* status, void* stream) {
  using namespace fr_scan_plan;
  ARGCHK(plonk_ok(log_n, W) && max_blocks_ok(max_blocks) && tile_ok(totals_tile));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(wires && sigma && shifts && beta && gamma && z_out && status);
  const size_t n = elems(log_n);
  ARGCHK(wires_bytes(log_n, W, m) != SAT && scalars_bytes(m) != SAT && scratch_ok(permutation_scratch_bytes(log_n, m)) &&
         scratch_ok(scan_scratch_bytes(n, m, true)));
  const host::Range in[5] = {{(uintptr_t)wires, wires_bytes(log_n, W, m)}, {(uintptr_t)sigma, identity_bytes(log_n, W)}, {(uintptr_t)shifts, scalars_bytes((size_t)W)},
                             {(uintptr_t)beta, scalars_bytes(m)}, {(uintptr_t)gamma, scalars_bytes(m)}};
  const host::Range outs[3] = {{(uintptr_t)z_out, rows_bytes(n, m)}, {(uintptr_t)total_out, scalars_bytes(m)}, {(uintptr_t)status, m}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  const PermutationLayout l = permutation_layout(log_n, m);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *roots = ws.at<u64>(l.roots), *num = ws.at<u64>(l.num), *den = ws.at<u64>(l.den);
  if (log_n >= 1) rc = ntth::build_table(log_n, roots, stream);
  if (rc == SYLOW_HIP_OK) {
    const size_t tiles = terms_tiles(log_n), its = terms_items(log_n, m);
    frs::k_plonk_terms<<<dim3((unsigned)grid(its, max_blocks)), dim3(BLOCK), 0, st>>>(wires, sigma, shifts, beta, gamma, roots, log_n, W, m, tiles, its, num, den);
    rc = frs::ratio_scan<true>(num, den, n, m, max_blocks, tile_of(totals_tile), 1, z_out, total_out, status, st);
  }
  return host::finish(rc, ws);
}
int32_t sylow_hip_plonk_permutation_batch(const uint64_t* wires, const uint64_t* sigma, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma,
                                          int32_t log_n, int32_t W, size_t m, uint64_t* z_out, uint64_t* total_out, uint8_t* status, void* stream) {
  return sylow_hip_plonk_permutation_batch_tuned(wires, sigma, shifts, beta, gamma, log_n, W, m, -1, -1, z_out, total_out, status, stream);
}
}  // extern "C"
