// groth16.hip -- the G1 / Fr side of batched Groth16 verification under ONE verifying key (include/sylow_hip.h, "Groth16"):
//   vk_x_i = IC_0 + sum_j x_ij IC_j for n proofs with the bases shared by every lane (Straus interleaving against per-call window tables),
//   the Fr column sums s = sum_i r_i, s_j = sum_i r_i x_ij of the weighted one-boolean test, and that test itself, composed from the
//   library's own stream-ordered calls.  The per-proof pairing check lives with the line-table kernels it reuses (groth16_pair.hpp,
//   compiled as the tail of plk_multi.hip).
#include "host.hpp"
#include "bn254_fr_block.hpp"
#include "weighted_plan.hpp"

namespace g16 {
static_assert(weighted_plan::WEIGHTED_BLOCK == BLOCK, "a part of a column sum is one block of BLOCK lanes");
// ------------------------------------------------------------------ vk_x: shared bases, one proof per lane ----------
// Window tables, built once per call by one lane per base: T[b][d] = d IC_b, d = 0..15, projective carry-free digits in the 7 x 16-byte
// entry of ProjTableGlobal (bn254_pairing.hpp), 1792 bytes per base -- a verifying key of 17 bases is 30 KB, resident in L2 and mostly in
// the vector L1 for the whole launch.  The base's address is wave-uniform; the digit picks one of its 16 entries.
typedef ProjTableGlobal<G1W> Tab;
constexpr int ENT = 16;
constexpr size_t BASE_BYTES = (size_t)ENT * 7 * 16;
BN_DEV Tab tab_of(const uint8_t* table, size_t b) { return Tab{(Tab::gptr)(table + b * BASE_BYTES)}; }

__global__ void __launch_bounds__(64) k_groth16_ic_table(const u64* ic, size_t n_bases, uint8_t* table) {
  const size_t b = TID;
  if (b >= n_bases) return;
  Tab tab = tab_of(table, b);
  const G1W p{f29_from_fp_reduced(load_fp(ic, n_bases, b, 0)), f29_from_fp_reduced(load_fp(ic, n_bases, b, 4)), OpsF29::one()};
  G1W acc = proj_zero<OpsF29>();
  tab.put(0, acc);
#pragma unroll 1
  for (int d = 1; d < ENT; ++d) {                       // complete formulas: 0 + P and P + P need no special case
    acc = proj_add_lazy<OpsF29>(acc, p);
    tab.put(d, acc);
  }
}
// Straus: ONE chain of 252 doublings per proof and, per 4-bit window, one complete addition per input (digit 0 adds the identity).  The
// inputs are walked as the RAW 256-bit words: every point of E(Fp) has order r, so x IC = (x mod r) IC and no reduction is needed -- any
// 256-bit word is legal, the rule of sylow_hip_evm_ecmul_batch.  The digit's word is re-read per window (input-major: a wavefront reads 64
// consecutive words; each is used for 16 windows and stays in cache) so that no per-input state lives in registers: n_inputs is unbounded.
__global__ void HEAVY_BOUNDS k_groth16_vk_x(const uint8_t* table, const u64* inputs, size_t n_inputs, size_t n, u64* oxy, uint8_t* oinf) {
  const size_t i = TID;
  if (i >= n) return;
  const size_t stride = n_inputs * n;
  G1W res = proj_zero<OpsF29>();
#pragma unroll 1
  for (int w = 63; w >= 0; --w) {
    if (w != 63) {
#pragma unroll 1
      for (int q = 0; q < 4; ++q) res = proj_double_lazy<OpsF29I>(res);
    }
    const u64* row = inputs + (size_t)(w >> 4) * stride + i;
    const int sh = 4 * (w & 15);
#pragma unroll 1
    for (size_t j = 0; j < n_inputs; ++j) {
      const int d = (int)((row[j * n] >> sh) & 15);
      res = proj_add_lazy<OpsF29I>(res, tab_of(table, j + 1).get(d));
    }
  }
  res = proj_add_lazy<OpsF29I>(res, tab_of(table, 0).get(1));      // + 1 IC_0
  Fp x, y; bool rinf;
  g1_to_affine(x, y, rinf, G1P{f29_to_fp(res.x), f29_to_fp(res.y), f29_to_fp(res.z)});      // spelt out: see g1w_to_affine (common.hpp)
  store_fp(oxy, n, i, 0, x); store_fp(oxy, n, i, 4, y);
  oinf[i] = rinf ? 1 : 0;
}

// ------------------------------------------------------------------ the weighted test's scalar side ----------
// weights -> weights mod r (the scalar multiplications and the MSM take values < p), and the per-call bases IC_0 .. IC_l, alpha as one
// SoA array [8][l + 2] for one batch of scalar multiplications
__global__ void __launch_bounds__(BLOCK) k_groth16_weighted_prep(const u64* weights, size_t n, u64* wr, const u64* ic, const u64* alpha, size_t n_bases, u64* bases) {
  const size_t i = TID;
  if (i < n) store_plain(wr, n, i, 0, fr_reduce_plain(load_plain(weights, n, i, 0)));
  if (i < n_bases + 1) {
    const bool a = i == n_bases;
#pragma unroll
    for (int w = 0; w < 8; ++w) bases[(size_t)w * (n_bases + 1) + i] = a ? alpha[w] : ic[(size_t)w * n_bases + i];
  }
}
// Column sums over the batch: column 0 is s = sum_i r_i, column j >= 1 is s_j = sum_i r_i x_ij (input j - 1 of the input-major array),
// all mod r.  A modular sum is exact, so the order of the reduction does not show in the result.  Two levels, so that a few columns
// still fill the GPU: block (col, part) of k_groth16_fr_sums adds up rows part * BLOCK + t, + parts * BLOCK, ... of its column and leaves one
// partial; k_groth16_fr_sums_join, one block per column, adds the column's partials.  out [4][cols + 1]: the columns, then s once more
// (the scalar of alpha) -- the scalar array that goes with k_groth16_weighted_prep's bases.  The number of parts: weighted_plan.hpp.
// partial [4][cols * parts]: the partial of (col, part) at index col * parts + part
__global__ void __launch_bounds__(BLOCK) k_groth16_fr_sums(const u64* wr, const u64* inputs, size_t n, size_t cols, size_t parts, u64* partial) {
  __shared__ u32 part[BLOCK][8];
  const size_t col = blockIdx.x, pt = blockIdx.y;
  Fp acc = fp_from_limbs(0, 0, 0, 0, 0, 0, 0, 0);
  const size_t n_in = (cols - 1) * n;
#pragma unroll 1
  for (size_t i = pt * BLOCK + threadIdx.x; i < n; i += parts * BLOCK) {
    const Fp r = load_plain(wr, n, i, 0);
    acc = fr_add(acc, col == 0 ? r : fr_mul(r, fr_reduce_plain(load_plain(inputs, n_in, (col - 1) * n + i, 0))));
  }
  const Fp s = block_sum(acc, part);
  if (threadIdx.x == 0) store_plain(partial, cols * parts, col * parts + pt, 0, s);
}
__global__ void __launch_bounds__(BLOCK) k_groth16_fr_sums_join(const u64* partial, size_t cols, size_t parts, u64* out) {
  __shared__ u32 part[BLOCK][8];
  const size_t col = blockIdx.x;
  const Fp s = column_sum(partial, cols, parts, col, part);
  if (threadIdx.x == 0) {
    store_plain(out, cols + 1, col, 0, s);
    if (col == 0) store_plain(out, cols + 1, cols, 0, s);
  }
}
// The n + 3 pairs of the weighted test as one SoA pair list (stride n + 3): (r_i A_i, B_i) for i < n, then
// (-s alpha, beta), (-sum_j s_j IC_j, gamma), (-sum_i r_i C_i, delta).  prod [8][cols + 1] + flags: s IC_0, s_1 IC_1 .. s_l IC_l, s alpha.
__global__ void __launch_bounds__(BLOCK) k_groth16_weighted_pairs(const u64* ra, const uint8_t* ra_inf, const u64* b, const uint8_t* b_inf, size_t n,
                                                                  const u64* prod, const uint8_t* prod_inf, size_t cols, const u64* sc, const uint8_t* sc_inf,
                                                                  const u64* beta, const u64* gamma, const u64* delta,
                                                                  u64* pxy, uint8_t* pinf, u64* qxy, uint8_t* qinf) {
  const size_t i = TID, m = n + 3;
  if (i >= m) return;
  if (i < n) {
#pragma unroll
    for (int w = 0; w < 8; ++w) pxy[(size_t)w * m + i] = ra[(size_t)w * n + i];
#pragma unroll
    for (int w = 0; w < 16; ++w) qxy[(size_t)w * m + i] = b[(size_t)w * n + i];
    pinf[i] = ra_inf[i];
    qinf[i] = b_inf ? b_inf[i] : 0;
    return;
  }
  const int which = (int)(i - n);
  G1W p = proj_zero<OpsF29>();                            // the identity joins as (0 : 1 : 0): the formulas are complete
  if (which == 1) {
#pragma unroll 1
    for (size_t j = 0; j < cols; ++j) p = proj_add_lazy<OpsF29>(p, load_g1w_flagged(prod, prod_inf, cols + 1, j));
  } else {
    p = which == 0 ? load_g1w_flagged(prod, prod_inf, cols + 1, cols) : load_g1w_flagged(sc, sc_inf, 1, 0);
  }
  Fp x, y; bool inf;
  g1w_to_affine(x, y, inf, p);
  if (!inf) y = fp_neg(y);
  store_fp(pxy, m, i, 0, x); store_fp(pxy, m, i, 4, y);
  pinf[i] = inf ? 1 : 0;
  const u64* q = which == 0 ? beta : which == 1 ? gamma : delta;
#pragma unroll
  for (int w = 0; w < 16; ++w) qxy[(size_t)w * m + i] = q[w];
  qinf[i] = 0;
}
}  // namespace g16

extern "C" {
int32_t sylow_hip_groth16_vk_x_batch(const uint64_t* vk_ic, size_t n_inputs, const uint64_t* inputs, size_t n,
                                     uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  ARGCHK(out_xy && out_inf && (n == 0 || (vk_ic && (inputs || !n_inputs)))); if (!n) return SYLOW_HIP_OK;
  host::Lease ws;
  int32_t rc = ws.acquire((n_inputs + 1) * g16::BASE_BYTES, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint8_t* table = (uint8_t*)ws.p;
  g16::k_groth16_ic_table<<<dim3((unsigned)((n_inputs + 1 + 63) / 64)), dim3(64), 0, (hipStream_t)stream>>>(vk_ic, n_inputs + 1, table);
  g16::k_groth16_vk_x<<<GRID(n)>>>(table, inputs, n_inputs, n, out_xy, out_inf);
  return host::finish(SYLOW_HIP_OK, ws);
}

int32_t sylow_hip_groth16_batch_verify_weighted(const uint64_t* vk_alpha, const uint64_t* vk_beta, const uint64_t* vk_gamma, const uint64_t* vk_delta,
                                                const uint64_t* vk_ic, size_t n_inputs, const uint64_t* a_xy, const uint8_t* a_inf,
                                                const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy, const uint8_t* c_inf,
                                                const uint64_t* inputs, const uint64_t* weights, size_t n, uint64_t* gt_out, uint8_t* is_one, void* stream) {
  ARGCHK((gt_out || is_one) && (n == 0 || (vk_alpha && vk_beta && vk_gamma && vk_delta && vk_ic && a_xy && b_xy && c_xy && weights && (inputs || !n_inputs))));
  if (!n) return sylow_hip_pairing_product_batch(nullptr, nullptr, nullptr, nullptr, 0, 1, gt_out, is_one, stream);
  using namespace weighted_plan;
  const Groth16WeightedLayout l = groth16_weighted_layout(n, n_inputs);
  ARGCHK(l.bytes != SAT);
  hipStream_t st = (hipStream_t)stream;
  const size_t cols = groth16_columns(n_inputs), nb = groth16_bases(n_inputs), m = groth16_pairs(n), parts = groth16_parts(n);
  host::Lease ws;
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *wr = ws.at<u64>(l.wr), *ra = ws.at<u64>(l.ra), *bases = ws.at<u64>(l.bases), *sums = ws.at<u64>(l.sums), *prod = ws.at<u64>(l.prod), *sc = ws.at<u64>(l.sc),
      *pxy = ws.at<u64>(l.pxy), *qxy = ws.at<u64>(l.qxy), *partial = ws.at<u64>(l.partial);
  uint8_t *ra_inf = ws.at<uint8_t>(l.ra_inf), *prod_inf = ws.at<uint8_t>(l.prod_inf), *sc_inf = ws.at<uint8_t>(l.sc_inf), *pinf = ws.at<uint8_t>(l.pinf),
          *qinf = ws.at<uint8_t>(l.qinf);
  g16::k_groth16_weighted_prep<<<GRID(n > nb ? n : nb)>>>(weights, n, wr, vk_ic, vk_alpha, cols, bases);
  g16::k_groth16_fr_sums<<<dim3((unsigned)cols, (unsigned)parts), dim3(BLOCK), 0, st>>>(wr, inputs, n, cols, parts, partial);
  g16::k_groth16_fr_sums_join<<<dim3((unsigned)cols), dim3(BLOCK), 0, st>>>(partial, cols, parts, sums);
  rc = sylow_hip_g1_scalar_mul_batch(a_xy, a_inf, wr, ra, ra_inf, n, stream);                                   // r_i A_i
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_scalar_mul_batch(bases, nullptr, sums, prod, prod_inf, nb, stream);  // s IC_0, s_j IC_j, s alpha
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_msm(c_xy, c_inf, wr, n, sc, sc_inf, stream);                         // sum_i r_i C_i
  if (rc == SYLOW_HIP_OK) {
    g16::k_groth16_weighted_pairs<<<GRID(m)>>>(ra, ra_inf, b_xy, b_inf, n, prod, prod_inf, cols, sc, sc_inf, vk_beta, vk_gamma, vk_delta, pxy, pinf, qxy, qinf);
    rc = sylow_hip_pairing_product_batch(pxy, pinf, qxy, qinf, m, /*skip_infinity=*/1, gt_out, is_one, stream);
  }
  return host::finish(rc, ws);
}
}  // extern "C"
