// groth16_prove.hip -- the prover's half of Groth16 on BN254 (include/sylow_hip.h, "Groth16, the prover's side"): the R1CS products A z, B z,
//   C z as a sparse matrix times m vectors over Fr (k_fr_spmv, new here); the quotient h = (a b - c) / (X^n - 1) through the transforms of
//   ntt.hip and ONE element-wise kernel on the coset 5 <w_n>; and the proof (A, B, C) from the library's own multi-scalar multiplications
//   and stream-ordered group calls, in chunks of whole witnesses.
// Lanes per row, grids, scratch and chunks: groth16_prove_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_acc.hpp"
#include "bn254_fr_dev.hpp"
#include "bn254_groth16_zinv.hpp"
#include "groth16_prove_plan.hpp"

namespace g16p {
using namespace g16_plan;
static_assert(G16_BLOCK == BLOCK, "the kernels run blocks of BLOCK lanes");
static_assert(BLOCK >> SPMV_LANES_LOG_MAX >= 1 && (1 << SPMV_LANES_LOG_MAX) <= 64, "the lanes of a row are lanes of one wavefront");

struct Scalar : FrArg {};      // a kernel names its parameter types in its symbol: this one stays a type of this namespace so that the symbol does not move

// out_j[i] = sum_e val_e w_j[col_e] over the entries e of row i, for the rows i < n_out of the arrays j < m (the grid's y, walked with a
// stride past G16_GRID_Y_CAP); rows from `rows` on are the padding and come out zero.  2^lg lanes share a row: lane `sub` takes the entries
// sub, sub + 2^lg, ... of the row into its accumulator, then the lanes add their residues with lg rounds of __shfl_xor and lane 0 stores.
// NO READ LEAVES THE ARRAYS, whatever row_ptr and col hold: a row's two ends are clamped to nnz (an end before its start is an empty row), and
// an entry whose column is n_cols or more is skipped, i.e. contributes zero.  w is canonical (k_fr_canon); val is taken mod r at the load.
// Every lane of a block walks the same number of row blocks, so the shuffles are reached by whole wavefronts.  Every index is size_t.
__global__ void __launch_bounds__(BLOCK) k_fr_spmv(const u64* row_ptr, const u64* col, const u64* val, size_t rows, size_t nnz, const u64* wc, size_t n_cols,
                                                   size_t m, size_t n_out, size_t row_blocks, u64* out, int lg) {
  const int lanes = 1 << lg, sub = threadIdx.x & (lanes - 1);
  const size_t rpb = (size_t)BLOCK >> lg;
#pragma unroll 1
  for (size_t j = blockIdx.y; j < m; j += gridDim.y) {
    const u64* w = wc + j * 4 * n_cols;
    u64* o = out + j * 4 * n_out;
#pragma unroll 1
    for (size_t g = blockIdx.x; g < row_blocks; g += gridDim.x) {
      const size_t i = g * rpb + (size_t)(threadIdx.x >> lg);
      size_t e = 0, end = 0;
      if (i < rows) {
        e = row_ptr[i];
        end = row_ptr[i + 1];
        e = e < nnz ? e : nnz;
        end = end < nnz ? end : nnz;
      }
      u32 acc[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] = 0;
      int terms = 0;
#pragma unroll 1
      for (e += (size_t)sub; e < end; e += (size_t)lanes) {
        const u64 c = col[e];
        if (c >= n_cols) continue;
        if (terms == SPMV_FLUSH) {                            // fold: the residue is one term of the next round
          const Fp f = fr_reduce_wide(acc);
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[k] = k < 8 ? f.v[k] : 0;
          terms = 1;
        }
        mul_acc(acc, fr_reduce_plain(load_plain(val, nnz, e, 0)), load_plain(w, n_cols, (size_t)c, 0));
        ++terms;
      }
      Fp s = fr_reduce_wide(acc);
#pragma unroll 1
      for (int off = 1; off < lanes; off <<= 1) s = fr_add(s, shfl_xor_fp(s, off));
      if (sub == 0 && i < n_out) store_plain(o, n_out, i, 0, s);
    }
  }
}

// dst = src mod r over `total` consecutive elements of arrays of n elements each: src and dst are [.][4][n]
__global__ void __launch_bounds__(BLOCK) k_fr_canon(const u64* src, u64* dst, size_t n, size_t total) {
#pragma unroll 1
  for (size_t t = TID; t < total; t += (size_t)gridDim.x * BLOCK) {
    const size_t j = t / n, i = t - j * n;
    store_plain(dst + j * 4 * n, n, i, 0, fr_reduce_plain(load_plain(src + j * 4 * n, n, i, 0)));
  }
}
// dst [count][4][len] = elements off .. off + len - 1 of src [count][4][stride]: the private part of a witness, the n - 1 terms of a quotient
__global__ void __launch_bounds__(BLOCK) k_fr_slice(const u64* src, size_t stride, size_t off, size_t len, u64* dst, size_t total) {
#pragma unroll 1
  for (size_t t = TID; t < total; t += (size_t)gridDim.x * BLOCK) {
    const size_t j = t / len, i = t - j * len;
    store_plain(dst + j * 4 * len, len, i, 0, load_plain(src + j * 4 * stride, stride, off + i, 0));
  }
}
// The coset's element-wise step over x = [3 m][4][n] (the values of a, b, c on g <w_n>, canonical): y_j = (a_j b_j - c_j) zinv, j < m.
// X^n - 1 is the constant g^n - 1 on the coset, zinv its inverse (bn254_groth16_zinv.hpp).
__global__ void __launch_bounds__(BLOCK) k_g16_quot_coset(const u64* x, u64* y, size_t n, size_t m, size_t total, Scalar zinv) {
  const Fp zi = from_scalar(zinv);
#pragma unroll 1
  for (size_t t = TID; t < total; t += (size_t)gridDim.x * BLOCK) {
    const size_t j = t / n, i = t - j * n;
    const Fp a = load_plain(x + j * 4 * n, n, i, 0), b = load_plain(x + (m + j) * 4 * n, n, i, 0), c = load_plain(x + (2 * m + j) * 4 * n, n, i, 0);
    store_plain(y + j * 4 * n, n, i, 0, fr_mul(fr_sub(fr_mul(a, b), c), zi));
  }
}
__global__ void k_g16_shift(u64* g) {
  if (TID < 4) g[TID] = TID ? 0 : G16_COSET_SHIFT;
}

static unsigned lane_grid(size_t total) { return (unsigned)grid_x(lane_blocks(total)); }

// out [m][4][n_out] = M wc_j for canonical wc [m][4][n_cols]
static void spmv_launch(const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t rows, size_t nnz, const u64* wc, size_t n_cols, size_t m,
                        size_t n_out, int32_t lg, uint64_t* out, hipStream_t st) {
  const size_t rb = spmv_row_blocks(n_out, lg);
  k_fr_spmv<<<dim3((unsigned)grid_x(rb), (unsigned)grid_y(m)), dim3(BLOCK), 0, st>>>(row_ptr, col, val, rows, nnz, wc, n_cols, m, n_out, rb, out, lg);
}

// h = the quotient of the 3 m arrays in x (a_j, b_j, c_j at arrays j, m + j, 2 m + j; any words) -> h [m][4][n]; x and y are buffers of
// 3 m arrays each and both are overwritten; h may be x (the prover) but not y.  g: 4 device words for the shift.
static int32_t quotient_core(u64* x, u64* y, u64* g, int32_t log_n, size_t m, uint64_t* h, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = elems(log_n), total = n * m;
  k_g16_shift<<<1, 64, 0, st>>>(g);
  int32_t rc = sylow_hip_fr_ntt_batch(x, log_n, 3 * m, /*inverse=*/1, nullptr, y, stream);            // the three polynomials' coefficients
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_fr_ntt_batch(y, log_n, 3 * m, /*inverse=*/0, g, x, stream);  // their values on the coset
  if (rc != SYLOW_HIP_OK) return rc;
  const uint64_t* zi = BN_G16_ZINV[log_n];
  k_g16_quot_coset<<<dim3(lane_grid(total)), dim3(BLOCK), 0, st>>>(x, y, n, m, total, Scalar{{zi[0], zi[1], zi[2], zi[3]}});
  return sylow_hip_fr_ntt_batch(y, log_n, m, /*inverse=*/1, g, h, stream);                             // h's coefficients from its coset values
}

// ---- the closing sums of a chunk of mc witnesses -------------------------------------------------------------------------------------------
enum { P_ALPHA, P_BETA1, P_DELTA1, P_SA, P_SB1, P_SL, P_SH, P_RD, P_SD, P_RSD, P_A, P_B1, P_S_A, P_R_B1, P_T1, P_T2, P_C, P_COUNT };   // G1 [8][mc] each
enum { Q_BETA2, Q_DELTA2, Q_SB2, Q_SD2, Q_T, Q_B, Q_COUNT };                                                                             // G2 [16][mc] each
enum { F_R, F_S, F_RS, F_COUNT };                                                                                                        // Fr [4][mc] each
static_assert(P_COUNT == CLOSE_G1 && Q_COUNT == CLOSE_G2 && F_COUNT == CLOSE_FR, "the plan prices these arrays");
static_assert(P_SB1 == P_SA + 1 && P_SL == P_SA + 2 && P_SH == P_SA + 3 && CLOSE_RAW_G1 == 4 && CLOSE_RAW_G2 == 1, "the gather writes the four G1 sums in a row");

// lane j < mc: the five key points replicated, r_j and s_j mod r, and r_j s_j
__global__ void __launch_bounds__(BLOCK) k_g16_close_prep(const u64* alpha, const u64* beta1, const u64* delta1, const u64* beta2, const u64* delta2, const u64* r,
                                                          const u64* s, size_t m, size_t j0, size_t mc, u64* p, u64* q, u64* f) {
  const size_t j = TID;
  if (j >= mc) return;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    p[((size_t)P_ALPHA * 8 + w) * mc + j] = alpha[w];
    p[((size_t)P_BETA1 * 8 + w) * mc + j] = beta1[w];
    p[((size_t)P_DELTA1 * 8 + w) * mc + j] = delta1[w];
  }
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    q[((size_t)Q_BETA2 * 16 + w) * mc + j] = beta2[w];
    q[((size_t)Q_DELTA2 * 16 + w) * mc + j] = delta2[w];
  }
  const Fp rj = fr_reduce_plain(load_plain(r, m, j0 + j, 0)), sj = fr_reduce_plain(load_plain(s, m, j0 + j, 0));
  store_plain(f + (size_t)F_R * 4 * mc, mc, j, 0, rj);
  store_plain(f + (size_t)F_S * 4 * mc, mc, j, 0, sj);
  store_plain(f + (size_t)F_RS * 4 * mc, mc, j, 0, fr_mul(rj, sj));
}
// the sums as the multi-scalar multiplications left them (one point of 8 / 16 consecutive words each, sum k of witness j at k mc + j) into
// the SoA arrays P_SA .. P_SH and Q_SB2, flags beside them
__global__ void __launch_bounds__(BLOCK) k_g16_close_gather(const u64* raw1, const uint8_t* raw1_inf, const u64* raw2, const uint8_t* raw2_inf, size_t mc, u64* p,
                                                            uint8_t* p_inf, u64* q, uint8_t* q_inf) {
  const size_t t = TID;
  if (t < 4 * mc) {
    const size_t k = t / mc, j = t - k * mc;
#pragma unroll
    for (int w = 0; w < 8; ++w) p[(((size_t)P_SA + k) * 8 + w) * mc + j] = raw1[t * 8 + w];
    p_inf[((size_t)P_SA + k) * mc + j] = raw1_inf[t];
  } else if (t < 5 * mc) {
    const size_t j = t - 4 * mc;
#pragma unroll
    for (int w = 0; w < 16; ++w) q[((size_t)Q_SB2 * 16 + w) * mc + j] = raw2[j * 16 + w];
    q_inf[(size_t)Q_SB2 * mc + j] = raw2_inf[j];
  }
}
// A, B, C of the chunk into columns j0 .. j0 + mc - 1 of the caller's arrays of stride m
__global__ void __launch_bounds__(BLOCK) k_g16_close_put(const u64* p, const uint8_t* p_inf, const u64* q, const uint8_t* q_inf, size_t mc, size_t m, size_t j0,
                                                         u64* a_xy, uint8_t* a_inf, u64* b_xy, uint8_t* b_inf, u64* c_xy, uint8_t* c_inf) {
  const size_t j = TID;
  if (j >= mc) return;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    a_xy[(size_t)w * m + j0 + j] = p[((size_t)P_A * 8 + w) * mc + j];
    c_xy[(size_t)w * m + j0 + j] = p[((size_t)P_C * 8 + w) * mc + j];
  }
#pragma unroll
  for (int w = 0; w < 16; ++w) b_xy[(size_t)w * m + j0 + j] = q[((size_t)Q_B * 16 + w) * mc + j];
  a_inf[j0 + j] = p_inf[(size_t)P_A * mc + j];
  c_inf[j0 + j] = p_inf[(size_t)P_C * mc + j];
  b_inf[j0 + j] = q_inf[(size_t)Q_B * mc + j];
}

struct Circuit {
  const uint64_t *row_ptr[3], *col[3], *val[3];
  size_t nnz[3], n_cons, n_vars, n_inputs;
  int32_t log_n;
};
struct Key {
  const uint64_t *alpha_g1, *beta_g1, *delta_g1, *beta_g2, *delta_g2;
  const uint64_t *a_query, *b_g1_query, *b_g2_query, *h_query, *l_query;
  const uint8_t *a_inf, *b_g1_inf, *b_g2_inf, *h_inf, *l_inf;
};
struct Proofs {
  uint64_t *a_xy, *b_xy, *c_xy;
  uint8_t *a_inf, *b_inf, *c_inf;
};

// the witnesses j0 .. j0 + mc - 1 in the arrays of one lease
static int32_t prove_chunk(const Circuit& ct, const Key& pk, const uint64_t* z, const uint64_t* r, const uint64_t* s, size_t m, size_t j0, size_t mc,
                           const host::Lease& ws, const Proofs& out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = elems(ct.log_n), nv = ct.n_vars, nl = private_vars(nv, ct.n_inputs), nh = n - 1;
  const ProveLayout l = prove_layout(ct.log_n, nv, ct.n_inputs, mc);      // of THIS chunk: a short last one sits at the front of the lease
  u64 *zc = ws.at<u64>(l.zc), *zl = ws.at<u64>(l.zl), *g = ws.at<u64>(l.quot.g), *x = ws.at<u64>(l.quot.x), *y = ws.at<u64>(l.quot.y), *hq = ws.at<u64>(l.hq);
  u64 *raw1 = ws.at<u64>(l.raw1), *raw2 = ws.at<u64>(l.raw2), *p = ws.at<u64>(l.p), *q = ws.at<u64>(l.q), *f = ws.at<u64>(l.f);
  uint8_t *raw1_inf = ws.at<uint8_t>(l.raw1_inf), *raw2_inf = ws.at<uint8_t>(l.raw2_inf), *p_inf = ws.at<uint8_t>(l.p_inf), *q_inf = ws.at<uint8_t>(l.q_inf);

  // 1. the witnesses mod r -- the vectors of the sparse products AND the scalars of the sums (below r, so below p: Fp::new leaves them alone)
  k_fr_canon<<<dim3(lane_grid(nv * mc)), dim3(BLOCK), 0, st>>>(z + j0 * 4 * nv, zc, nv, nv * mc);
  if (nl) k_fr_slice<<<dim3(lane_grid(nl * mc)), dim3(BLOCK), 0, st>>>(zc, nv, ct.n_inputs + 1, nl, zl, nl * mc);
  // 2. A z, B z, C z padded to the domain, straight into the quotient's first buffer
  for (int k = 0; k < 3; ++k)
    spmv_launch(ct.row_ptr[k], ct.col[k], ct.val[k], ct.n_cons, ct.nnz[k], zc, nv, mc, n, spmv_lanes_log(ct.n_cons, ct.nnz[k]), x + (size_t)k * mc * 4 * n, st);
  // 3. h, then its first n - 1 coefficients as h_query's scalars
  int32_t rc = quotient_core(x, y, g, ct.log_n, mc, x, stream);
  if (rc != SYLOW_HIP_OK) return rc;
  if (nh) k_fr_slice<<<dim3(lane_grid(nh * mc)), dim3(BLOCK), 0, st>>>(x, n, 0, nh, hq, nh * mc);
  // 4. the five sums of every witness
  for (size_t j = 0; j < mc && rc == SYLOW_HIP_OK; ++j) {
    const u64 *zj = zc + j * 4 * nv, *zlj = zl + j * 4 * nl, *hj = hq + j * 4 * nh;
    rc = sylow_hip_g1_msm(pk.a_query, pk.a_inf, zj, nv, raw1 + (0 * mc + j) * 8, raw1_inf + 0 * mc + j, stream);
    if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_msm(pk.b_g1_query, pk.b_g1_inf, zj, nv, raw1 + (1 * mc + j) * 8, raw1_inf + 1 * mc + j, stream);
    if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_msm(pk.l_query, pk.l_inf, zlj, nl, raw1 + (2 * mc + j) * 8, raw1_inf + 2 * mc + j, stream);
    if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_msm(pk.h_query, pk.h_inf, hj, nh, raw1 + (3 * mc + j) * 8, raw1_inf + 3 * mc + j, stream);
    if (rc == SYLOW_HIP_OK) rc = sylow_hip_g2_msm(pk.b_g2_query, pk.b_g2_inf, zj, nv, raw2 + j * 16, raw2_inf + j, stream);
  }
  if (rc != SYLOW_HIP_OK) return rc;
  // 5. the closing sums, mc lanes wide
  k_g16_close_prep<<<GRID(mc)>>>(pk.alpha_g1, pk.beta_g1, pk.delta_g1, pk.beta_g2, pk.delta_g2, r, s, m, j0, mc, p, q, f);
  k_g16_close_gather<<<GRID(5 * mc)>>>(raw1, raw1_inf, raw2, raw2_inf, mc, p, p_inf, q, q_inf);
  auto P = [&](int k) { return p + (size_t)k * 8 * mc; };
  auto PI = [&](int k) { return p_inf + (size_t)k * mc; };
  auto Q = [&](int k) { return q + (size_t)k * 16 * mc; };
  auto QI = [&](int k) { return q_inf + (size_t)k * mc; };
  auto F = [&](int k) { return f + (size_t)k * 4 * mc; };
  auto mul1 = [&](int base, const uint8_t* base_inf, int k, int dst) {
    if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_scalar_mul_batch(P(base), base_inf, F(k), P(dst), PI(dst), mc, stream);
  };
  auto add1 = [&](int a, const uint8_t* a_inf, int b, int dst) {
    if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_add_batch(P(a), a_inf, P(b), PI(b), P(dst), PI(dst), mc, stream);
  };
  mul1(P_DELTA1, nullptr, F_R, P_RD);
  mul1(P_DELTA1, nullptr, F_S, P_SD);
  mul1(P_DELTA1, nullptr, F_RS, P_RSD);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g2_scalar_mul_batch(Q(Q_DELTA2), nullptr, F(F_S), Q(Q_SD2), QI(Q_SD2), mc, stream);
  add1(P_ALPHA, nullptr, P_SA, P_T1);                        // A = alpha + sum z a_query + r delta
  add1(P_T1, PI(P_T1), P_RD, P_A);
  add1(P_BETA1, nullptr, P_SB1, P_T1);                       // B1 = beta + sum z b_g1_query + s delta, in G1
  add1(P_T1, PI(P_T1), P_SD, P_B1);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g2_add_batch(Q(Q_BETA2), nullptr, Q(Q_SB2), QI(Q_SB2), Q(Q_T), QI(Q_T), mc, stream);     // B, the same in G2
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g2_add_batch(Q(Q_T), QI(Q_T), Q(Q_SD2), QI(Q_SD2), Q(Q_B), QI(Q_B), mc, stream);
  mul1(P_A, PI(P_A), F_S, P_S_A);
  mul1(P_B1, PI(P_B1), F_R, P_R_B1);
  add1(P_SL, PI(P_SL), P_SH, P_T1);                          // C = sum z l_query + sum h h_query + s A + r B1 - r s delta
  add1(P_T1, PI(P_T1), P_S_A, P_T2);
  add1(P_T2, PI(P_T2), P_R_B1, P_T1);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_sub_batch(P(P_T1), PI(P_T1), P(P_RSD), PI(P_RSD), P(P_C), PI(P_C), mc, stream);
  if (rc != SYLOW_HIP_OK) return rc;
  k_g16_close_put<<<GRID(mc)>>>(p, p_inf, q, q_inf, mc, m, j0, out.a_xy, out.a_inf, out.b_xy, out.b_inf, out.c_xy, out.c_inf);
  return SYLOW_HIP_OK;
}
}  // namespace g16p

extern "C" {
int32_t sylow_hip_fr_spmv_batch_tuned(const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t rows, size_t nnz, const uint64_t* w, size_t n_cols,
                                      size_t m, size_t n_out, int32_t lanes_log, uint64_t* out, void* stream) {
  using namespace g16_plan;
  ARGCHK(n_out >= rows && spmv_lanes_log_ok(lanes_log));
  if (!m || !n_out) return SYLOW_HIP_OK;
  ARGCHK(row_ptr && out && (!nnz || (col && val)) && (!n_cols || w));
  ARGCHK(mul_sat(batch_words(n_out, m), 8) != SAT && mul_sat(batch_words(n_cols, m), 8) != SAT && mul_sat(nnz, 32) != SAT && rows != SAT);
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  int32_t rc = ws.acquire(spmv_scratch_bytes(n_cols, m), st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* wc = ws.at<u64>(0);
  if (n_cols) g16p::k_fr_canon<<<dim3(g16p::lane_grid(n_cols * m)), dim3(BLOCK), 0, st>>>(w, wc, n_cols, n_cols * m);
  g16p::spmv_launch(row_ptr, col, val, rows, nnz, wc, n_cols, m, n_out, spmv_lanes_log_or_default(lanes_log, rows, nnz), out, st);
  return host::finish(SYLOW_HIP_OK, ws);
}
int32_t sylow_hip_fr_spmv_batch(const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t rows, size_t nnz, const uint64_t* w, size_t n_cols,
                                size_t m, size_t n_out, uint64_t* out, void* stream) {
  return sylow_hip_fr_spmv_batch_tuned(row_ptr, col, val, rows, nnz, w, n_cols, m, n_out, -1, out, stream);
}
int32_t sylow_hip_groth16_quotient_batch(const uint64_t* a, const uint64_t* b, const uint64_t* c, int32_t log_n, size_t m, uint64_t* h_out, void* stream) {
  using namespace g16_plan;
  ARGCHK(log_n_ok(log_n));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(a && b && c && h_out);
  const QuotLayout l = quot_layout(log_n, m);
  const size_t bytes = l.bytes, one = batch_words(elems(log_n), m);
  ARGCHK(bytes != SAT);
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  int32_t rc = ws.acquire(bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *g = ws.at<u64>(l.g), *x = ws.at<u64>(l.x), *y = ws.at<u64>(l.y);
  const uint64_t* src[3] = {a, b, c};
  for (int k = 0; k < 3 && rc == SYLOW_HIP_OK; ++k) {
    const hipError_t e = hipMemcpyAsync(x + (size_t)k * one, src[k], one * sizeof(u64), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) rc = host::fail(e, "hipMemcpyAsync of the quotient's inputs");
  }
  if (rc == SYLOW_HIP_OK) rc = g16p::quotient_core(x, y, g, log_n, m, h_out, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_groth16_prove_batch(const uint64_t* a_row_ptr, const uint64_t* a_col, const uint64_t* a_val, size_t a_nnz, const uint64_t* b_row_ptr,
                                      const uint64_t* b_col, const uint64_t* b_val, size_t b_nnz, const uint64_t* c_row_ptr, const uint64_t* c_col,
                                      const uint64_t* c_val, size_t c_nnz, size_t n_cons, size_t n_vars, size_t n_inputs, int32_t log_n, const uint64_t* alpha_g1,
                                      const uint64_t* beta_g1, const uint64_t* delta_g1, const uint64_t* beta_g2, const uint64_t* delta_g2, const uint64_t* a_query,
                                      const uint8_t* a_query_inf, const uint64_t* b_g1_query, const uint8_t* b_g1_query_inf, const uint64_t* b_g2_query,
                                      const uint8_t* b_g2_query_inf, const uint64_t* h_query, const uint8_t* h_query_inf, const uint64_t* l_query,
                                      const uint8_t* l_query_inf, const uint64_t* z, const uint64_t* r, const uint64_t* s, size_t m, uint64_t* a_xy, uint8_t* a_inf,
                                      uint64_t* b_xy, uint8_t* b_inf, uint64_t* c_xy, uint8_t* c_inf, void* stream) {
  using namespace g16_plan;
  ARGCHK(log_n_ok(log_n));
  ARGCHK(n_cons <= elems(log_n) && n_inputs < n_vars);
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(a_row_ptr && b_row_ptr && c_row_ptr && (!a_nnz || (a_col && a_val)) && (!b_nnz || (b_col && b_val)) && (!c_nnz || (c_col && c_val)));
  ARGCHK(alpha_g1 && beta_g1 && delta_g1 && beta_g2 && delta_g2 && a_query && b_g1_query && b_g2_query);
  ARGCHK((log_n == 0 || h_query) && (private_vars(n_vars, n_inputs) == 0 || l_query));
  ARGCHK(z && r && s && a_xy && a_inf && b_xy && b_inf && c_xy && c_inf);
  ARGCHK(mul_sat(a_nnz, 32) != SAT && mul_sat(b_nnz, 32) != SAT && mul_sat(c_nnz, 32) != SAT && mul_sat(batch_words(n_vars, m), 8) != SAT);
  const size_t lim = host::scratch_limit(), mc = witnesses_per_chunk(log_n, n_vars, n_inputs, m, lim ? lim : msmh::default_budget());
  if (!mc) {
    snprintf(sylow_g_err, sizeof(sylow_g_err), "groth16_prove: the scratch limit does not hold one witness (%zu bytes)", prove_budget_bytes(log_n, n_vars, n_inputs, 1));
    return SYLOW_HIP_E_HIP;
  }
  const g16p::Circuit ct = {{a_row_ptr, b_row_ptr, c_row_ptr}, {a_col, b_col, c_col}, {a_val, b_val, c_val}, {a_nnz, b_nnz, c_nnz}, n_cons, n_vars, n_inputs, log_n};
  const g16p::Key pk = {alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, a_query, b_g1_query, b_g2_query, h_query, l_query,
                        a_query_inf, b_g1_query_inf, b_g2_query_inf, h_query_inf, l_query_inf};
  const g16p::Proofs out = {a_xy, b_xy, c_xy, a_inf, b_inf, c_inf};
  host::Lease ws;
  int32_t rc = ws.acquire(prove_chunk_bytes(log_n, n_vars, n_inputs, mc), (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  for (size_t j0 = 0; j0 < m && rc == SYLOW_HIP_OK; j0 += mc) rc = g16p::prove_chunk(ct, pk, z, r, s, m, j0, m - j0 < mc ? m - j0 : mc, ws, out, stream);
  return host::finish(rc, ws);
}
}  // extern "C"
