// plonk_quotient.hip -- PLONK's quotient polynomial (include/sylow_plonk.h):
//   sylow_plonk_quotient_prepare       the table of a circuit: its selectors, sigma and L_1 on the coset K = 5 <w_N>, and (X^n - 1)^-1 there;
//   sylow_plonk_quotient_evals_batch   t_ext = (gate + alpha perm + alpha^2 boundary) / (X^n - 1) point by point on K, ONE fused kernel;
//   sylow_plonk_quotient_batch         the route from coefficients: pad, one transform onto K, the fused kernel, one transform back, the status.
// The fused kernel keeps a lane per point and streams over the wire columns with three accumulators: the gate sum, unreduced through
// mul_acc, and the two running products of the permutation argument, which start from z_i and z_(i+E).  Nothing of size W lives in
// registers.  Geometry, the degree bound, chunks and scratch: plonk_quotient_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_block.hpp"
#include "bn254_fr_acc.hpp"
#include "plonk_quotient_plan.hpp"
#include "../../include/sylow_plonk.h"

namespace pq {
using namespace plonk_quotient_plan;
static_assert(PQ_BLOCK == BLOCK, "the kernels run one tile per block of BLOCK lanes");
enum { CH_BETA, CH_GAMMA, CH_ALPHA, CH_ALPHA2, CH_COUNT };      // the challenges of an instance, behind its W products beta k_j 5
static_assert(SYLOW_HIP_PLONK_WIRES_MAX == PQ_WIRES_MAX && PQ_WIRES_MAX + CH_COUNT <= BLOCK && CH_COUNT == PQ_CHALLENGE_SLOTS, "the header's bound is the plan's; a lane per constant of an instance");

// element k of an Fr SoA array of stride n, mod r (bn254_fr_block.hpp's elem), the reduction out of line for the same reason as fold below
BN_NOINLINE Fp canon(Fp a) { return fr_reduce_plain(a); }
BN_DEV Fp at(const u64* a, size_t n, size_t k) { return canon(load_plain(a, n, k, 0)); }
struct Wide {
  u32 v[16];
};
// the one Barrett reduction of the kernel, out of line: its constants stay out of the kernel's scalar registers
BN_NOINLINE Fp fold(Wide a) { return fr_reduce_wide(a.v); }
// acc += a b, unreduced; the PQ_FLUSH products before it are folded first.  THE BOUND (bn254_fr_acc.hpp): both factors are canonical and a
// fold leaves a residue below r, so the accumulator stays below r + 16 r^2 < 2^512.
BN_DEV void gate_add(Wide& acc, int& pending, const Fp& a, const Fp& b) {
  if (pending == PQ_FLUSH) {
    const Fp f = fold(acc);
#pragma unroll
    for (int k = 0; k < 16; ++k) acc.v[k] = k < 8 ? f.v[k] : 0;
    pending = 0;
  }
  mul_acc(acc.v, a, b);
  ++pending;
}

// The constants of instance s0 + s, s < mc, a lane per (s, c): consts [mc][W + CH_COUNT][4], entry c < W = beta k_c 5 -- formed ONCE per (instance,
// column), not per point -- then beta, gamma, alpha and alpha^2, all canonical
__global__ void __launch_bounds__(BLOCK) k_pq_consts(const u64* shifts, const u64* beta, const u64* gamma, const u64* alpha, size_t m, size_t s0, size_t mc, int W,
                                                     u64* consts) {
  const size_t per = const_slots(W);
#pragma unroll 1
  for (size_t f = TID; f < mc * per; f += (size_t)gridDim.x * BLOCK) {
    const size_t s = f / per, c = f - s * per;
    Fp v;
    if (c < (size_t)W) v = fr_mul(fr_mul(elem(beta, m, s0 + s), elem(shifts, (size_t)W, c)), fp_from_limbs((u32)PQ_COSET_SHIFT, 0, 0, 0, 0, 0, 0, 0));
    else {
      const int k = (int)(c - (size_t)W);
      v = elem(k == CH_BETA ? beta : k == CH_GAMMA ? gamma : alpha, m, s0 + s);
      if (k == CH_ALPHA2) v = fr_mul(v, v);
    }
    store_plain(consts + f * FR_WORDS, 1, 0, 0, v);
  }
}

// Item (instance s, tile of BLOCK points), a lane per point i of K, x_i = 5 w_N^i:
//   gate = q_M w_0 w_1 + sum_j q_j w_j + q_C + PI,   A = z_i prod_j (w_j + gamma + (beta k_j 5) w_N^i),   B = z_(i+E) prod_j (w_j + gamma + beta sigma_j),
//   out_i = (gate + alpha (A - B) + alpha^2 L_1 (z_i - 1)) zinv[i mod E].
// The first W + CH_COUNT lanes bring the instance's constants (k_pq_consts) into LDS once per item; w_N^i is one load from the table of the
// N / 2 roots.  inst_cols = 0: the caller's arrays, wires [.][W][4][N], z and pi [.][4][N]; inst_cols > 0: one buffer [.][inst_cols][4][N]
// that holds an instance's wires, then z, then pi, and `wires`, `z` and `pi` point at the first instance's.  pi may be NULL.  Every index is
// size_t; i < N and i + E wraps inside N.  A row of the table or a column of the wires is reached through the element index: row r of
// [.][4][N] is element r 4 N + i of the first.
__global__ void __launch_bounds__(BLOCK) k_pq_fused(const u64* table, const u64* wires, const u64* z, const u64* pi, size_t inst_cols, const u64* consts,
                                                    const u64* roots, int log_n, int log_e, int W, size_t n_items, u64* out) {
  __shared__ u32 cs[PQ_WIRES_MAX + CH_COUNT][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    // the sizes are derived per item from two scalars the compiler must take as new here: hoisted out of this loop, the dozen values
    // derived from them (masks, halves, row offsets) would each hold scalar registers across the column loop, more than there are
    asm volatile("" : "+s"(log_n), "+s"(log_e));
    const int lb = log_big(log_n, log_e);
    const size_t N = elems(lb), row = row_words(log_n, log_e), n_tiles = tiles(log_n, log_e);
    const size_t s = item_instance(it, n_tiles), i = point(item_tile(it, n_tiles), t);
    __syncthreads();                                         // the item before has read cs
    if (t < W + CH_COUNT) lds_put(cs, t, load_plain(consts + (s * const_slots(W) + (size_t)t) * FR_WORDS, 1, 0, 0));
    __syncthreads();
    if (i >= N) continue;                                    // the barriers above are reached by whole blocks: `it` is the block's
    const Fp x = fr_root_from_half_table(roots, lb, i), b = lds_get(cs, W + CH_BETA), g = lds_get(cs, W + CH_GAMMA);
    const u64 *ws = wires + s * (inst_cols ? inst_cols : (size_t)W) * row, *zs = z + s * (inst_cols ? inst_cols : 1) * row;
    Fp nu = at(zs, N, i), de = at(zs, N, next_point(i, log_n, log_e)), w01 = fr_one();
    Wide acc;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc.v[k] = 0;
    int pending = 0;
#pragma unroll 1
    for (int j = 0; j < W; ++j) {
      const Fp w = at(ws, N, (size_t)j * row + i);
      const Fp wg = fr_add(w, g);
      nu = fr_mul(nu, fr_add(wg, fr_mul(lds_get(cs, j), x)));
      de = fr_mul(de, fr_add(wg, fr_mul(b, at(table, N, row_sigma(W, j) * row + i))));
      if (j < 2) w01 = j ? fr_mul(w01, w) : w;
      gate_add(acc, pending, at(table, N, row_selector(j) * row + i), w);
    }
    gate_add(acc, pending, at(table, N, row_qm(W) * row + i), w01);
    gate_add(acc, pending, lds_get(cs, W + CH_ALPHA), fr_sub(nu, de));
    gate_add(acc, pending, lds_get(cs, W + CH_ALPHA2), fr_mul(at(table, N, row_l1(W) * row + i), fr_sub(at(zs, N, i), fr_one())));
    Fp sum = fr_add(fold(acc), at(table, N, row_qc(W) * row + i));
    if (pi) sum = fr_add(sum, at(pi + s * (inst_cols ? inst_cols : 1) * row, N, i));
    store_plain(out + s * row, N, i, 0, fr_mul(sum, at(table + zinv_offset_words(log_n, log_e, W), elems(log_e), zinv_slot(i, log_e))));
  }
}

// Item (array a, tile): dst array (a / per) dst_per + col0 + a % per, [4][N], takes the `len` elements of src array a, [4][len], as they
// lie (the transform reduces them) and zeros from len on
__global__ void __launch_bounds__(BLOCK) k_pq_pad(const u64* src, size_t len, size_t per, size_t dst_per, size_t col0, size_t N, size_t n_tiles, size_t n_items,
                                                  u64* dst) {
#pragma unroll 1
  for (size_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const size_t a = it / n_tiles, i = point(it % n_tiles, threadIdx.x);
    if (i >= N) continue;
    u64* d = dst + ((a / per) * dst_per + col0 + a % per) * FR_WORDS * N;
    store_plain(d, N, i, 0, i < len ? load_plain(src + a * FR_WORDS * len, len, i, 0) : fr_zero());
  }
}
// the values of L_1 on <w_n>: 1, 0, .., 0
__global__ void __launch_bounds__(BLOCK) k_pq_l1(u64* out, size_t n) {
#pragma unroll 1
  for (size_t i = TID; i < n; i += (size_t)gridDim.x * BLOCK) store_plain(out, n, i, 0, i ? fr_zero() : fr_one());
}
__global__ void k_pq_shift(u64* g) {
  if (TID < PQ_SHIFT_WORDS) g[TID] = TID ? 0 : PQ_COSET_SHIFT;
}
// zinv_k = (5^n w_N^(n k) - 1)^-1 for k < E, a lane each: w_N^(n k) is one load from the table of the N / 2 roots (n k < N)
__global__ void __launch_bounds__(BLOCK) k_pq_zinv(const u64* roots, int log_n, int log_e, u64* out) {
  const size_t E = elems(log_e);
#pragma unroll 1
  for (size_t k = TID; k < E; k += (size_t)gridDim.x * BLOCK) {
    const Fp v = fr_mul(fr_pow(fp_from_limbs((u32)PQ_COSET_SHIFT, 0, 0, 0, 0, 0, 0, 0), (u64)elems(log_n)), fr_root_from_half_table(roots, log_big(log_n, log_e), k << log_n));
    store_plain(out, E, k, 0, fr_inv(fr_sub(v, fr_one())));
  }
}
__global__ void __launch_bounds__(BLOCK) k_pq_status_clear(uint8_t* status, size_t m) {
#pragma unroll 1
  for (size_t j = TID; j < m; j += (size_t)gridDim.x * BLOCK) status[j] = 0;
}
// Item (instance s, tile of the tail): the coefficients first .. N - 1 of t [m][4][N], canonical, a lane each; a block that meets one that is
// not 0 stores STATUS_NOT_DIVISIBLE into status[s] (every such block stores the same byte over the 0 the launch before left)
__global__ void __launch_bounds__(BLOCK) k_pq_status_tail(const u64* t_out, size_t N, size_t first, size_t n_tiles, size_t n_items, uint8_t* status) {
#pragma unroll 1
  for (size_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const size_t s = it / n_tiles, k = first + point(it % n_tiles, threadIdx.x);
    const int nz = k < N && !fp_is_zero(load_plain(t_out + s * FR_WORDS * N, N, k, 0)) ? 1 : 0;
    if (__syncthreads_or(nz) && threadIdx.x == 0) status[s] = (uint8_t)STATUS_NOT_DIVISIBLE;
  }
}

// the constants of instances s0 .. s0 + mc - 1 into `consts`, then the fused kernel over them
static void fused_launch(const u64* table, const u64* wires, const u64* z, const u64* pi, size_t inst_cols, const u64* shifts, const u64* beta, const u64* gamma,
                         const u64* alpha, size_t m, size_t s0, size_t mc, u64* consts, const u64* roots, int log_n, int log_e, int W, long long max_blocks, u64* out,
                         hipStream_t st) {
  const size_t its = items(log_n, log_e, mc);
  k_pq_consts<<<dim3((unsigned)grid(tail_tiles(mc * const_slots(W)), max_blocks)), dim3(BLOCK), 0, st>>>(shifts, beta, gamma, alpha, m, s0, mc, W, consts);
  k_pq_fused<<<dim3((unsigned)grid(its, max_blocks)), dim3(BLOCK), 0, st>>>(table, wires, z, pi, inst_cols, consts, roots, log_n, log_e, W, its, out);
}
static void pad_launch(const u64* src, size_t len, size_t arrays, size_t per, size_t dst_per, size_t col0, int log_n, int log_e, long long max_blocks, u64* dst,
                       hipStream_t st) {
  const size_t n_tiles = tiles(log_n, log_e), its = mul_sat(n_tiles, arrays);
  k_pq_pad<<<dim3((unsigned)grid(its, max_blocks)), dim3(BLOCK), 0, st>>>(src, len, per, dst_per, col0, elems(log_big(log_n, log_e)), n_tiles, its, dst);
}

struct Job {
  const u64 *table, *wires, *z, *pi, *shifts, *beta, *gamma, *alpha;
  size_t len_w, len_z, m, mc_lease;                   // mc_lease: the instances of the largest chunk, which fixes the layout of the lease
  int log_n, log_e, W;
  long long max_blocks;
  u64* t_out;
};
// instances s0 .. s0 + mc - 1 through the lease ws (chunk_layout): A [mc][cols][4][N] | B the same
static int32_t chunk(const Job& j, size_t s0, size_t mc, const host::Lease& ws, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const int lb = log_big(j.log_n, j.log_e);
  const size_t N = elems(lb), n = elems(j.log_n), row = row_words(j.log_n, j.log_e), cols = columns(j.W, j.pi != nullptr);
  const ChunkLayout l = chunk_layout(j.log_n, j.log_e, j.W, cols, j.mc_lease, mc);
  u64 *g = ws.at<u64>(l.g), *roots = ws.at<u64>(l.roots), *consts = ws.at<u64>(l.consts), *A = ws.at<u64>(l.a), *B = ws.at<u64>(l.b);
  pad_launch(j.wires + s0 * (size_t)j.W * FR_WORDS * j.len_w, j.len_w, mc * (size_t)j.W, (size_t)j.W, cols, 0, j.log_n, j.log_e, j.max_blocks, A, st);
  pad_launch(j.z + s0 * FR_WORDS * j.len_z, j.len_z, mc, 1, cols, col_z(j.W), j.log_n, j.log_e, j.max_blocks, A, st);
  if (j.pi) pad_launch(j.pi + s0 * FR_WORDS * n, n, mc, 1, cols, col_pi(j.W), j.log_n, j.log_e, j.max_blocks, A, st);
  int32_t rc = sylow_hip_fr_ntt_batch(A, lb, mc * cols, /*inverse=*/0, g, B, stream);                 // every column's values on K
  if (rc != SYLOW_HIP_OK) return rc;
  fused_launch(j.table, B, B + col_z(j.W) * row, j.pi ? B + col_pi(j.W) * row : nullptr, cols, j.shifts, j.beta, j.gamma, j.alpha, j.m, s0, mc, consts, roots, j.log_n,
               j.log_e, j.W, j.max_blocks, A, st);
  return sylow_hip_fr_ntt_batch(A, lb, mc, /*inverse=*/1, g, j.t_out + s0 * FR_WORDS * N, stream);   // t's coefficients from its values on K
}
}  // namespace pq

extern "C" {
int32_t sylow_plonk_quotient_prepare(const uint64_t* selectors, const uint64_t* sigma, int32_t log_n, int32_t log_e, int32_t W, uint64_t* table, void* stream) {
  using namespace plonk_quotient_plan;
  ARGCHK(dims_ok(log_n, log_e, W));
  ARGCHK(selectors && sigma && table);
  ARGCHK(scratch_ok(prepare_scratch_bytes(log_n, log_e, W)));
  const host::Range in[2] = {{(uintptr_t)selectors, selectors_bytes(log_n, W)}, {(uintptr_t)sigma, sigma_bytes(log_n, W)}};
  const host::Range outs[1] = {{(uintptr_t)table, table_bytes(log_n, log_e, W)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  const int lb = log_big(log_n, log_e);
  const size_t n = elems(log_n), rows = table_rows(W);
  host::Lease ws;
  const PrepareLayout l = prepare_layout(log_n, log_e, W);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *g = ws.at<u64>(l.g), *roots = ws.at<u64>(l.roots), *coeff = ws.at<u64>(l.coeff), *l1 = ws.at<u64>(l.l1), *padded = ws.at<u64>(l.padded);
  pq::k_pq_shift<<<1, 64, 0, st>>>(g);
  pq::k_pq_l1<<<dim3((unsigned)grid(tiles(log_n, 0), -1)), dim3(BLOCK), 0, st>>>(l1, n);
  rc = sylow_hip_fr_ntt_batch(selectors, log_n, (size_t)W + 2, /*inverse=*/1, nullptr, coeff, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_fr_ntt_batch(sigma, log_n, (size_t)W, /*inverse=*/1, nullptr, coeff + row_sigma(W, 0) * FR_WORDS * n, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_fr_ntt_batch(l1, log_n, 1, /*inverse=*/1, nullptr, coeff + row_l1(W) * FR_WORDS * n, stream);
  if (rc == SYLOW_HIP_OK) {
    pq::pad_launch(coeff, n, rows, rows, rows, 0, log_n, log_e, -1, padded, st);
    rc = sylow_hip_fr_ntt_batch(padded, lb, rows, /*inverse=*/0, g, table, stream);
  }
  if (rc == SYLOW_HIP_OK && lb >= 1) rc = ntth::build_table(lb, roots, stream);
  if (rc == SYLOW_HIP_OK)
    pq::k_pq_zinv<<<dim3((unsigned)grid(tiles(log_e, 0), -1)), dim3(BLOCK), 0, st>>>(roots, log_n, log_e, table + zinv_offset_words(log_n, log_e, W));
  return host::finish(rc, ws);
}

int32_t sylow_plonk_quotient_evals_batch_tuned(const uint64_t* table, const uint64_t* wires_ext, const uint64_t* z_ext, const uint64_t* pi_ext,
                                               const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, int32_t log_n,
                                               int32_t log_e, int32_t W, size_t m, int64_t max_blocks, uint64_t* t_ext_out, void* stream) {
  using namespace plonk_quotient_plan;
  ARGCHK(dims_ok(log_n, log_e, W) && max_blocks_ok(max_blocks));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(table && wires_ext && z_ext && shifts && beta && gamma && alpha && t_ext_out);
  ARGCHK(ext_bytes(log_n, log_e, mul_sat((size_t)W, m)) != SAT && scalars_bytes(m) != SAT && items(log_n, log_e, m) != SAT && scratch_ok(evals_scratch_bytes(log_n, log_e, W, m)));
  const host::Range in[8] = {{(uintptr_t)table, table_bytes(log_n, log_e, W)}, {(uintptr_t)wires_ext, ext_bytes(log_n, log_e, (size_t)W * m)},
                             {(uintptr_t)z_ext, ext_bytes(log_n, log_e, m)}, {(uintptr_t)pi_ext, ext_bytes(log_n, log_e, m)},
                             {(uintptr_t)shifts, scalars_bytes((size_t)W)}, {(uintptr_t)beta, scalars_bytes(m)}, {(uintptr_t)gamma, scalars_bytes(m)},
                             {(uintptr_t)alpha, scalars_bytes(m)}};
  const host::Range outs[1] = {{(uintptr_t)t_ext_out, ext_bytes(log_n, log_e, m)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  const int lb = log_big(log_n, log_e);
  host::Lease ws;
  const EvalsLayout l = evals_layout(log_n, log_e, W, m);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *roots = ws.at<u64>(l.roots), *consts = ws.at<u64>(l.consts);
  if (lb >= 1) rc = ntth::build_table(lb, roots, stream);
  if (rc == SYLOW_HIP_OK) pq::fused_launch(table, wires_ext, z_ext, pi_ext, 0, shifts, beta, gamma, alpha, m, 0, m, consts, roots, log_n, log_e, W, max_blocks, t_ext_out, st);
  return host::finish(rc, ws);
}
int32_t sylow_plonk_quotient_evals_batch(const uint64_t* table, const uint64_t* wires_ext, const uint64_t* z_ext, const uint64_t* pi_ext, const uint64_t* shifts,
                                         const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, int32_t log_n, int32_t log_e, int32_t W, size_t m,
                                         uint64_t* t_ext_out, void* stream) {
  return sylow_plonk_quotient_evals_batch_tuned(table, wires_ext, z_ext, pi_ext, shifts, beta, gamma, alpha, log_n, log_e, W, m, -1, t_ext_out, stream);
}

int32_t sylow_plonk_quotient_batch_tuned(const uint64_t* table, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* pi,
                                         const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, int32_t log_n,
                                         int32_t log_e, int32_t W, size_t m, int64_t max_blocks, uint64_t* t_out, uint8_t* status, void* stream) {
  using namespace plonk_quotient_plan;
  ARGCHK(dims_ok(log_n, log_e, W) && max_blocks_ok(max_blocks) && lens_ok(log_n, log_e, len_w, len_z) && degree_ok(log_n, log_e, W, len_w, len_z));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(table && wires && z && shifts && beta && gamma && alpha && t_out && status);
  const size_t cols = columns(W, pi != nullptr);
  ARGCHK(ext_bytes(log_n, log_e, mul_sat(cols, m)) != SAT && scalars_bytes(m) != SAT && pad_tiles(log_n, log_e, cols, m) != SAT);
  const host::Range in[8] = {{(uintptr_t)table, table_bytes(log_n, log_e, W)}, {(uintptr_t)wires, coeff_bytes(len_w, (size_t)W * m)},
                             {(uintptr_t)z, coeff_bytes(len_z, m)}, {(uintptr_t)pi, coeff_bytes(elems(log_n), m)}, {(uintptr_t)shifts, scalars_bytes((size_t)W)},
                             {(uintptr_t)beta, scalars_bytes(m)}, {(uintptr_t)gamma, scalars_bytes(m)}, {(uintptr_t)alpha, scalars_bytes(m)}};
  const host::Range outs[2] = {{(uintptr_t)t_out, ext_bytes(log_n, log_e, m)}, {(uintptr_t)status, m}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const size_t lim = host::scratch_limit(), mc = instances_per_chunk(log_n, log_e, W, cols, m, lim ? lim : msmh::default_budget());
  if (!mc) {
    snprintf(sylow_g_err, sizeof(sylow_g_err), "plonk_quotient: the scratch limit does not hold one instance (%zu bytes)", chunk_budget_bytes(log_n, log_e, W, cols, 1));
    return SYLOW_HIP_E_HIP;
  }
  const hipStream_t st = (hipStream_t)stream;
  const int lb = log_big(log_n, log_e);
  host::Lease ws;
  const ChunkLayout l = chunk_layout(log_n, log_e, W, cols, mc, mc);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  pq::k_pq_shift<<<1, 64, 0, st>>>(ws.at<u64>(l.g));
  if (lb >= 1) rc = ntth::build_table(lb, ws.at<u64>(l.roots), stream);
  const pq::Job job = {table, wires, z, pi, shifts, beta, gamma, alpha, len_w, len_z, m, mc, log_n, log_e, W, max_blocks, t_out};
  for (size_t s0 = 0; s0 < m && rc == SYLOW_HIP_OK; s0 += mc) rc = pq::chunk(job, s0, chunk_size(m, mc, s0), ws, stream);
  if (rc == SYLOW_HIP_OK) {
    const size_t tail = tail_len(log_n, log_e, W, len_w, len_z), n_tiles = tail_tiles(tail), its = tail_items(tail, m);
    pq::k_pq_status_clear<<<dim3((unsigned)grid(tail_tiles(m), max_blocks)), dim3(BLOCK), 0, st>>>(status, m);
    if (its)
      pq::k_pq_status_tail<<<dim3((unsigned)grid(its, max_blocks)), dim3(BLOCK), 0, st>>>(t_out, elems(lb), tail_first(log_n, W, len_w, len_z), n_tiles, its, status);
  }
  return host::finish(rc, ws);
}
int32_t sylow_plonk_quotient_batch(const uint64_t* table, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* pi,
                                   const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, int32_t log_n, int32_t log_e,
                                   int32_t W, size_t m, uint64_t* t_out, uint8_t* status, void* stream) {
  return sylow_plonk_quotient_batch_tuned(table, wires, len_w, z, len_z, pi, shifts, beta, gamma, alpha, log_n, log_e, W, m, -1, t_out, status, stream);
}
}  // extern "C"
