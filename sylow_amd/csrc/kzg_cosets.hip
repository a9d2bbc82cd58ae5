// kzg_cosets.hip -- the KZG proofs of a polynomial on EVERY COSET of its domain in n log n (include/sylow_hip_kzg_cosets.h), the multi-proof
//   form of the Feist-Khovratovich construction.  n = c l points, coset i the roots of X^l - v^i, v = w^l:
//   pi_i = sum_(t<c) v^(it) h_t,   h_t = sum_k f_(k+(t+1)l) s_k = sum_(a<l) h^(a)_t   -- a forward G1 transform of c points of a sum of l Toeplitz
//   products of size c, each kzg_open_all.hip's with n -> c, coefficients f_(a+lj) and SRS points s_(a+lu): h = the first c points of
//   G1-INTT_2c( sum_a F^(a)_j T^(a)_j ), F^(a) = Fr-NTT_2c((2c)^-1 f_(a+l.), then c zeros), T^(a) = G1-NTT_2c(x^(a)).
// Per polynomial: one split launch, ONE Fr transform of m l arrays, the product-sums fused with stage 0 of the inverse transform (2l
// multiplications from the affine table per butterfly, cut into planes where c m alone does not fill the device), the fold of the planes, and
// from there the launches of kzg_open_all.hip with n -> c: g1ntth::stage, kzoah::fwd_first, g1ntth::close.
// The verifier's side reduces a cell to a row of the single-point check: R = f mod (X^l - v^i) by an inverse Fr transform and a twist.
// Geometry, planes, ping-pong, grids and scratch: kzg_cosets_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "g1_ntt_dev.hpp"
#include "bn254_fr_dev.hpp"
#include "bn254_fr_roots.hpp"
#include "kzg_cosets_plan.hpp"
#include "../../include/sylow_hip_kzg_cosets.h"

namespace kzco {
using namespace kzg_cosets_plan;
using g1ntt::butterfly_store;
using g1ntt::load_input;
using g1ntt::store_canonical;
using g1ntt::store_identity;
using g1ntt::to_core;
static_assert(g1_ntt_plan::G1_NTT_BLOCK == BLOCK, "the kernels run blocks of BLOCK lanes");
static_assert(g1_ntt_plan::G1_NTT_TABLE_BYTES_PER_LANE == G1_TABLE_BYTES_PER_LANE, "a lane's window table");
static_assert(SYLOW_HIP_KZG_COSETS_LOG_N_MAX == COSETS_LOG_N_MAX, "the header's bound is the plan's");

struct Scalar : FrArg {};      // a kernel names its parameter types in its symbol: this one stays a type of this namespace so that the symbol does not move

// the l arrays x^(a) of the plan, [l][8][2c] + [l][2c]: the SRS point x_srs_index names, word for word, or the identity
__global__ void __launch_bounds__(BLOCK) k_open_cosets_x(const u64* srs, int log_c, int log_l, size_t total, u64* xy, uint8_t* inf) {
  const size_t n = elems(log_n(log_c, log_l)), cc = wide(log_c), lanes = (size_t)gridDim.x * BLOCK;
#pragma unroll 1
  for (size_t i = TID; i < total; i += lanes) {
    const size_t a = i >> wide_log(log_c), k = i & (cc - 1), t = x_srs_index(a, k, log_c, log_l);
    u64* out = xy + a * G1_NTT_AFFINE_WORDS * cc;
    if (t == X_IDENTITY) { store_identity(out, inf + a * cc, cc, k); continue; }
#pragma unroll
    for (int w = 0; w < (int)G1_NTT_AFFINE_WORDS; ++w) out[(size_t)w * cc + k] = srs[(size_t)w * n + t];
    inf[i] = 0;
  }
}
// log_c = 0: the one proof of each polynomial is the identity
__global__ void __launch_bounds__(BLOCK) k_open_cosets_trivial(u64* pi_xy, uint8_t* pi_inf, size_t m) {
  const size_t lanes = (size_t)gridDim.x * BLOCK;
  for (size_t j = TID; j < m; j += lanes) store_identity(pi_xy + j * G1_NTT_AFFINE_WORDS, pi_inf + j, 1, 0);
}
// P^(a)_j = s (f_(a + l j) mod r) for j < c, then c zeros, over the m l rows of [m l][4][2c]: consecutive lanes write consecutive words
__global__ void __launch_bounds__(BLOCK) k_open_cosets_split(const u64* coeffs, u64* padded, int log_c, int log_l, size_t total, Scalar s) {
  const size_t n = elems(log_n(log_c, log_l)), cc = wide(log_c), lanes = (size_t)gridDim.x * BLOCK;
  const Fp ss = from_scalar(s);
#pragma unroll 1
  for (size_t i = TID; i < total; i += lanes) {
    const size_t row = split_row(i, log_c), k = split_col(i, log_c);
    Fp v = fp_from_limbs(0, 0, 0, 0, 0, 0, 0, 0);
    if (!split_is_zero(k, log_c))
      v = fr_mul(ss, fr_reduce_plain(load_plain(coeffs + split_poly(row, log_l) * FR_WORDS * n, n, split_src(split_residue(row, log_l), k, log_l), 0)));
    store_plain(padded + row * FR_WORDS * cc, cc, k, 0, v);
  }
}
BN_DEV G1P times(const G1P& t, const u64* f, size_t nn, size_t k, void* region) {
  const Fp s = load_plain(f, nn, k, 0);               // canonical: the Fr transform wrote it
  u32 kk[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) kk[q] = s.v[q];
  G1P p = g1_scalar_mul_ws(t, kk, region);
  const bool inf = fp_is_zero(p.z);                   // (0 : 1 : 0) for every Z = 0, as the stage kernel hands its product on
  p.x = fp_select(p.x, fp_zero(), inf);
  p.y = fp_select(p.y, fp_one(), inf);
  return p;
}
// a + b by the complete addition, the identity as (0 : 1 : 0) so that a further addition may follow
BN_DEV G1W add_canonical(const G1W& a, const G1W& b) {
  const G1W r = proj_add_lazy<OpsF29>(a, b);
  const bool inf = OpsF29::is_zero(r.z);
  return G1W{OpsF29::select(r.x, OpsF29::zero(), inf), OpsF29::select(r.y, OpsF29::one(), inf), r.z};
}
// sum over the residues a of a slice of F^(a)_k T^(a)_k at column k of the 2c: ONE accumulator lives across the multiplications
BN_DEV G1W product_sum(const u64* txy, const uint8_t* tinf, const u64* f, size_t cc, size_t k, size_t a0, size_t a1, void* region) {
  G1W acc = proj_zero<OpsF29>();
#pragma unroll 1
  for (size_t a = a0; a < a1; ++a) {
    const G1P t = load_input(txy + a * G1_NTT_AFFINE_WORDS * cc, tinf ? tinf + a * cc : nullptr, cc, k);
    acc = add_canonical(acc, to_core(times(t, f + a * FR_WORDS * cc, cc, k, region)));
  }
  return acc;
}
// The product-sums fused with stage 0 of the inverse transform of 2c points (every twiddle is 1) over items (plane, polynomial, butterfly):
// U = sum_a F^(a)_j T^(a)_j over the plane's residues, then V = the same at j + c; out[2j] = U + V, out[2j + 1] = U - V into a projective
// buffer [12][stride] at the columns of array p m + A.  U is summed over the whole slice before V starts and waits in column 2j, which only
// this lane writes: the interleaved order keeps two accumulators alive across every multiplication, this one keeps one.
// tables: one region per lane of the launch, as k_g1_ntt_stage.
__global__ void HEAVY_BOUNDS k_open_cosets_first(const u64* txy, const uint8_t* tinf, const u64* f, u64* dst, int log_c, int log_l, int pl, size_t m, size_t total,
                                                 size_t stride, uint8_t* tables) {
  const size_t cc = wide(log_c), lanes = (size_t)gridDim.x * BLOCK;
  void* region = tables + TID * G1_TABLE_BYTES_PER_LANE;
#pragma unroll 1
  for (size_t b = TID; b < total; b += lanes) {
    const size_t arr = first_array(b, log_c), j = first_butterfly(b, log_c), p = first_plane(arr, m), A = first_poly(arr, m);
    const size_t a0 = slice_begin(p, log_l, pl), a1 = a0 + slice_len(log_l, pl);
    const u64* fa = f + fr_row(A, 0, log_l) * FR_WORDS * cc;
    const size_t o0 = first_out0(arr, j, log_c);
    G1W v;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {                       // one body for both sums; U waits in its own output column while V is formed
      v = product_sum(txy, tinf, fa, cc, h ? first_in1(j, log_c) : first_in0(j), a0, a1, region);
      if (!h) store_canonical(dst, stride, o0, v);
    }
    butterfly_store(dst, stride, o0, first_out1(arr, j, log_c), g1w_load_proj(dst, stride, o0), v, OpsF29::is_zero(v.z));
  }
}
// column q of the m 2c: the sum over the planes, into the buffer the stages read
__global__ void __launch_bounds__(BLOCK) k_open_cosets_fold(const u64* src, u64* dst, int log_c, int pl, size_t m, size_t total, size_t src_stride, size_t stride) {
  const size_t lanes = (size_t)gridDim.x * BLOCK, planes = elems(pl);
#pragma unroll 1
  for (size_t q = TID; q < total; q += lanes) {
    G1W acc = g1w_load_proj(src, src_stride, fold_in(q, 0, log_c, m));
#pragma unroll 1
    for (size_t p = 1; p < planes; ++p) acc = add_canonical(acc, g1w_load_proj(src, src_stride, fold_in(q, p, log_c, m)));
    store_canonical(dst, stride, q, acc);
  }
}

// Item (row, lane q of 2^lanes_log): r_k <- r_k g^k for k = q, q + lanes, .. with g = w^(-idx) and a running product.  Lane 0 of the row
// writes z = v^idx and the range flag where the caller wants them (z, in_range_out: either may be NULL).
__global__ void __launch_bounds__(BLOCK) k_coset_twist(u64* r, const u64* idx, int log_c, int log_l, size_t total, size_t n_rows, u64* z, uint8_t* in_range_out) {
  const size_t l = elems(log_l), lanes = (size_t)gridDim.x * BLOCK;
  const int ql = twist_lanes_log(log_l);
  // w_n by ntt_plan::root_squarings squarings, spelt out: behind a function the compiler closes this loop with the opposite branch
  Fp w = fp_from_limbs(BN_FR_ROOT28);
#pragma unroll 1
  for (int i = 0; i < ntt_plan::root_squarings(log_n(log_c, log_l)); ++i) w = fr_mul(w, w);
#pragma unroll 1
  for (size_t i = TID; i < total; i += lanes) {
    const size_t row = i >> ql, q = i & (elems(ql) - 1);
    const u64 id = idx[row];
    if (q == 0) {
      if (z) store_plain(z, n_rows, row, 0, fr_pow(w, z_exp(id, log_c, log_l)));
      if (in_range_out) in_range_out[row] = in_range(id, log_c) ? 1 : 0;
    }
    const Fp g = fr_pow(w, twist_exp(id, log_c, log_l)), step = fr_pow(g, elems(ql));
    Fp p = fr_pow(g, q);
    u64* rr = r + row * FR_WORDS * l;
#pragma unroll 1
    for (size_t k = q; k < l; k += elems(ql)) {
      store_plain(rr, l, k, 0, fr_mul(load_plain(rr, l, k, 0), p));
      p = fr_mul(p, step);
    }
  }
}
__global__ void __launch_bounds__(BLOCK) k_coset_flags(uint8_t* ok, const uint8_t* in_range, size_t n) {
#pragma unroll 1
  for (size_t j = TID; j < n; j += (size_t)gridDim.x * BLOCK) ok[j] = ok[j] && in_range[j] ? 1 : 0;
}

static int32_t open_cosets(const uint64_t* txy, const uint8_t* tinf, const uint64_t* coeffs, int log_c, int log_l, size_t m, long long max_blocks, int pl,
                           uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const ScratchLayout l = scratch_layout(log_c, log_l, m, pl, max_blocks);
  if (l.bytes > SAT / 2) return host::fail(hipErrorOutOfMemory, "scratch of the proofs on every coset");
  int32_t rc = y_out ? sylow_hip_fr_ntt_batch(coeffs, log_n(log_c, log_l), m, /*inverse=*/0, nullptr, y_out, stream) : SYLOW_HIP_OK;
  if (rc != SYLOW_HIP_OK) return rc;
  if (trivial(log_c)) {
    k_open_cosets_trivial<<<dim3((unsigned)oa::trivial_grid(m)), dim3(BLOCK), 0, st>>>(pi_xy, pi_inf, m);
    LAUNCHED();
  }
  host::Lease ws;
  rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  uint8_t* tables = ws.at<uint8_t>(l.tables);
  u64 *tw_wide = ws.at<u64>(l.tw_wide), *tw = ws.at<u64>(l.tw);
  u64* buf[2] = {ws.at<u64>(l.buf[0]), ws.at<u64>(l.buf[1])};
  u64 *planes = ws.at<u64>(l.planes), *padded = ws.at<u64>(l.padded), *f = ws.at<u64>(l.f);
  const size_t str = stride(log_c, m);
  const int L = wide_log(log_c);
  const ntt_plan::Words4 ni = ntt_plan::n_inverse(L);
  k_open_cosets_split<<<dim3((unsigned)split_grid(log_c, log_l, m)), dim3(BLOCK), 0, st>>>(coeffs, padded, log_c, log_l, split_items(log_c, log_l, m),
                                                                                           Scalar{{ni.w[0], ni.w[1], ni.w[2], ni.w[3]}});
  rc = sylow_hip_fr_ntt_batch(padded, L, rows(log_l, m), /*inverse=*/0, nullptr, f, stream);
  if (rc == SYLOW_HIP_OK) rc = ntth::build_table(L, tw_wide, stream);
  if (rc == SYLOW_HIP_OK && log_c >= 2) rc = ntth::build_table(log_c, tw, stream);
  if (rc == SYLOW_HIP_OK) {
    k_open_cosets_first<<<dim3((unsigned)first_grid(log_c, m, pl, max_blocks)), dim3(BLOCK), 0, st>>>(
        txy, tinf, f, folds(pl) ? planes : buf[oa::inv_dst(0)], log_c, log_l, pl, m, first_items(log_c, m, pl), folds(pl) ? plane_stride(log_c, m, pl) : str, tables);
    if (folds(pl))
      k_open_cosets_fold<<<dim3((unsigned)fold_grid(log_c, m, max_blocks)), dim3(BLOCK), 0, st>>>(planes, buf[oa::inv_dst(0)], log_c, pl, m, fold_items(log_c, m),
                                                                                                  plane_stride(log_c, m, pl), str);
  }
  for (int s = 1; s < oa::inv_stages(log_c) && rc == SYLOW_HIP_OK; ++s)
    rc = g1ntth::stage(buf[oa::inv_src(s)], buf[oa::inv_dst(s)], L, m, str, s, /*inverse=*/true, tw_wide, tables, max_blocks, stream);
  if (rc == SYLOW_HIP_OK) rc = kzoah::fwd_first(buf[oa::fwd_src(log_c, 0)], buf[oa::fwd_dst(log_c, 0)], log_c, m, str, max_blocks, stream);
  for (int s = 1; s < oa::fwd_stages(log_c) && rc == SYLOW_HIP_OK; ++s)
    rc = g1ntth::stage(buf[oa::fwd_src(log_c, s)], buf[oa::fwd_dst(log_c, s)], log_c, m, str, s, /*inverse=*/false, tw, tables, max_blocks, stream);
  if (rc == SYLOW_HIP_OK) rc = g1ntth::close(buf[oa::close_src(log_c)], log_c, m, str, pi_xy, pi_inf, max_blocks, stream);
  return host::finish(rc, ws);
}
// r_out <- the interpolants; z and the flags where asked for
static int32_t interp(const uint64_t* vals, const uint64_t* idx, int log_c, int log_l, size_t n_rows, uint64_t* r_out, uint64_t* z, uint8_t* in_range_out, void* stream) {
  const int32_t rc = sylow_hip_fr_ntt_batch(vals, log_l, n_rows, /*inverse=*/1, nullptr, r_out, stream);
  if (rc != SYLOW_HIP_OK) return rc;
  k_coset_twist<<<dim3((unsigned)twist_grid(log_l, n_rows)), dim3(BLOCK), 0, (hipStream_t)stream>>>(r_out, idx, log_c, log_l, twist_items(log_l, n_rows), n_rows, z,
                                                                                                   in_range_out);
  LAUNCHED();
}
}  // namespace kzco

extern "C" {
int32_t sylow_hip_kzg_open_cosets_prepare(const uint64_t* srs_g1_xy, int32_t log_c, int32_t log_l, uint64_t* table_xy, uint8_t* table_inf, void* stream) {
  using namespace kzg_cosets_plan;
  ARGCHK(logs_ok(log_c, log_l));
  ARGCHK(srs_g1_xy && table_xy && table_inf);
  ARGCHK(prepare_scratch_bytes(log_c, log_l) != SAT);
  const PrepareLayout l = prepare_layout(log_c, log_l);
  host::Lease ws;
  int32_t rc = ws.acquire(l.bytes, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* xy = ws.at<u64>(l.xy);
  uint8_t* inf = ws.at<uint8_t>(l.inf);
  kzco::k_open_cosets_x<<<dim3((unsigned)prepare_grid(log_c, log_l)), dim3(BLOCK), 0, (hipStream_t)stream>>>(srs_g1_xy, log_c, log_l, prepare_items(log_c, log_l), xy, inf);
  rc = sylow_hip_g1_ntt_batch(xy, inf, wide_log(log_c), elems(log_l), /*inverse=*/0, table_xy, table_inf, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_open_cosets_batch_tuned(const uint64_t* table_xy, const uint8_t* table_inf, const uint64_t* coeffs, int32_t log_c, int32_t log_l, size_t m,
                                              int64_t max_blocks, int32_t planes_log, uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  using namespace kzg_cosets_plan;
  ARGCHK(logs_ok(log_c, log_l) && max_blocks_ok(max_blocks) && planes_log_ok(planes_log, log_l));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(table_xy && coeffs && pi_xy && pi_inf);
  const int pl = planes_log_of(planes_log, log_c, log_l, m, max_blocks);
  const size_t fb = fr_bytes(log_c, log_l, m), pb = pi_xy_bytes(log_c, m), tb = table_xy_bytes(log_c, log_l);
  ARGCHK(fb != SAT && pb != SAT && tb != SAT && split_words(log_c, log_l, m) != SAT && plane_stride(log_c, m, pl) != SAT);
  ARGCHK(!y_out || disjoint((uintptr_t)coeffs, fb, (uintptr_t)y_out, fb));                 // the Fr transform reads what other blocks of it write
  ARGCHK(!y_out || disjoint((uintptr_t)table_xy, tb, (uintptr_t)y_out, fb));
  ARGCHK(disjoint((uintptr_t)coeffs, fb, (uintptr_t)pi_xy, pb) && disjoint((uintptr_t)table_xy, tb, (uintptr_t)pi_xy, pb));
  return kzco::open_cosets(table_xy, table_inf, coeffs, log_c, log_l, m, max_blocks, pl, y_out, pi_xy, pi_inf, stream);
}
int32_t sylow_hip_kzg_open_cosets_batch(const uint64_t* table_xy, const uint8_t* table_inf, const uint64_t* coeffs, int32_t log_c, int32_t log_l, size_t m,
                                        uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  return sylow_hip_kzg_open_cosets_batch_tuned(table_xy, table_inf, coeffs, log_c, log_l, m, -1, -1, y_out, pi_xy, pi_inf, stream);
}
int32_t sylow_hip_kzg_coset_interp_batch(const uint64_t* vals, const uint64_t* idx, int32_t log_c, int32_t log_l, size_t rows, uint64_t* r_out, uint8_t* in_range_out,
                                         void* stream) {
  using namespace kzg_cosets_plan;
  ARGCHK(logs_ok(log_c, log_l));
  if (!rows) return SYLOW_HIP_OK;
  ARGCHK(vals && idx && r_out);
  const size_t vb = vals_bytes(log_l, rows);
  ARGCHK(vb != SAT && disjoint((uintptr_t)vals, vb, (uintptr_t)r_out, vb));
  ARGCHK(disjoint((uintptr_t)idx, rows * sizeof(uint64_t), (uintptr_t)r_out, vb));
  return kzco::interp(vals, idx, log_c, log_l, rows, r_out, nullptr, in_range_out, stream);
}
int32_t sylow_hip_kzg_cosets_reduce_batch(const uint64_t* srs_g1_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* idx, const uint64_t* vals,
                                          int32_t log_c, int32_t log_l, size_t rows, uint64_t* cred_xy, uint8_t* cred_inf, uint64_t* z_out, uint8_t* in_range_out,
                                          void* stream) {
  using namespace kzg_cosets_plan;
  ARGCHK(logs_ok(log_c, log_l));
  if (!rows) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && c_xy && idx && vals && cred_xy && cred_inf && z_out);
  const ReduceLayout l = reduce_layout(log_l, rows);
  const size_t bytes = l.bytes, vb = vals_bytes(log_l, rows), pb = point_bytes(rows), sb = scalar_bytes(rows);
  ARGCHK(bytes != SAT);
  ARGCHK(disjoint((uintptr_t)c_xy, pb, (uintptr_t)cred_xy, pb) && disjoint((uintptr_t)vals, vb, (uintptr_t)cred_xy, pb) && disjoint((uintptr_t)vals, vb, (uintptr_t)z_out, sb));
  ARGCHK(disjoint((uintptr_t)idx, rows * sizeof(uint64_t), (uintptr_t)cred_xy, pb) && disjoint((uintptr_t)idx, rows * sizeof(uint64_t), (uintptr_t)z_out, sb));
  ARGCHK(disjoint((uintptr_t)c_xy, pb, (uintptr_t)z_out, sb));
  host::Lease ws;
  int32_t rc = ws.acquire(bytes, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *r = ws.at<u64>(l.r), *rc_xy = ws.at<u64>(l.rc_xy);
  uint8_t* rc_inf = ws.at<uint8_t>(l.rc_inf);
  rc = kzco::interp(vals, idx, log_c, log_l, rows, r, z_out, in_range_out, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_kzg_commit_batch(srs_g1_xy, r, elems(log_l), rows, rc_xy, rc_inf, stream);        // R(tau) G1gen
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_sub_batch(c_xy, c_inf, rc_xy, rc_inf, cred_xy, cred_inf, rows, stream);       // C - R(tau) G1gen
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_verify_cosets_batch(const uint64_t* srs_g1_xy, const uint64_t* tau_l_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* idx,
                                          const uint64_t* vals, int32_t log_c, int32_t log_l, size_t rows, const uint64_t* pi_xy, const uint8_t* pi_inf, uint8_t* ok,
                                          void* stream) {
  using namespace kzg_cosets_plan;
  ARGCHK(logs_ok(log_c, log_l));
  if (!rows) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && tau_l_g2_xy && c_xy && idx && vals && pi_xy && ok);
  const VerifyLayout l = verify_layout(rows);
  const size_t bytes = l.bytes, sb = scalar_bytes(rows);
  ARGCHK(bytes != SAT && reduce_scratch_bytes(log_l, rows) != SAT);
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  int32_t rc = ws.acquire(bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *cred = ws.at<u64>(l.cred), *z = ws.at<u64>(l.z), *y = ws.at<u64>(l.y);
  uint8_t *cred_inf = ws.at<uint8_t>(l.cred_inf), *in_rng = ws.at<uint8_t>(l.in_rng);
  if (hipMemsetAsync(y, 0, sb, st) != hipSuccess) rc = host::fail(hipGetLastError(), "clearing y");
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_kzg_cosets_reduce_batch(srs_g1_xy, c_xy, c_inf, idx, vals, log_c, log_l, rows, cred, cred_inf, z, in_rng, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_kzg_verify_batch(tau_l_g2_xy, cred, cred_inf, z, y, pi_xy, pi_inf, ok, rows, stream);
  if (rc == SYLOW_HIP_OK) kzco::k_coset_flags<<<dim3((unsigned)g1_ntt_plan::grid(rows, -1)), dim3(BLOCK), 0, st>>>(ok, in_rng, rows);
  return host::finish(rc, ws);
}
}  // extern "C"
