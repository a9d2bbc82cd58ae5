// kzg_open_all.hip -- the KZG proofs of a polynomial at ALL n = 2^log_n points of its domain in n log n (include/sylow_hip.h, "KZG, the
//   prover's side: every point of the domain at once"), the Feist-Khovratovich construction:
//   pi_i = sum_b w^(ib) h_b,   h_b = sum_(t <= n-2-b) f_(b+1+t) s_t   -- a forward G1 transform of a Toeplitz product, and the Toeplitz product a
//   cyclic convolution of 2n points: h = the first n points of G1-INTT_2n(F_i T_i) with F = Fr-NTT_2n(f, then n zeros) and T = G1-NTT_2n(x),
//   x_(2n-1-t) = s_t.  T depends on the SRS alone: sylow_hip_kzg_open_all_prepare builds it once (through sylow_hip_g1_ntt_batch).
// Per polynomial nothing between F and the affine proofs leaves the device or projective form: the pointwise products are fused with
// stage 0 of the inverse transform (two multiplications from the affine table per butterfly), the factor (2n)^-1 is one Fr product per
// coefficient BEFORE the Fr transform (which is linear) instead of a scalar multiplication per point after the inverse one, the stages from 1 on and the closing kernel
// are g1_ntt.hip's (g1ntth::stage, g1ntth::close), and the forward transform's stage 0 reads h where the inverse transform left it.
// Geometry, ping-pong, grids and scratch: kzg_open_all_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "g1_ntt_dev.hpp"
#include "bn254_fr_dev.hpp"
#include "kzg_open_all_plan.hpp"

namespace kzoa {
using namespace kzg_open_all_plan;
using g1ntt::butterfly_store;
using g1ntt::load_input;
using g1ntt::store_identity;
using g1ntt::to_core;
static_assert(g1_ntt_plan::G1_NTT_BLOCK == BLOCK, "the kernels run blocks of BLOCK lanes");
static_assert(g1_ntt_plan::G1_NTT_TABLE_BYTES_PER_LANE == G1_TABLE_BYTES_PER_LANE, "a lane's window table");

struct Scalar : FrArg {};      // a kernel names its parameter types in its symbol: this one stays a type of this namespace so that the symbol does not move

// x of the plan over its 2n columns: the SRS point x_srs_index names, word for word, or the identity
__global__ void __launch_bounds__(BLOCK) k_open_all_x(const u64* srs, int log_n, u64* xy, uint8_t* inf) {
  const size_t n = elems(log_n), nn = wide(log_n), k = TID;
  if (k >= nn) return;
  const size_t t = x_srs_index(k, log_n);
  if (t == X_IDENTITY) { store_identity(xy, inf, nn, k); return; }
#pragma unroll
  for (int w = 0; w < (int)G1_NTT_AFFINE_WORDS; ++w) xy[(size_t)w * nn + k] = srs[(size_t)w * n + t];
  inf[k] = 0;
}
// log_n = 0: the one proof of each polynomial is the identity
__global__ void __launch_bounds__(BLOCK) k_open_all_trivial(u64* pi_xy, uint8_t* pi_inf, size_t m) {
  const size_t lanes = (size_t)gridDim.x * BLOCK;
  for (size_t j = TID; j < m; j += lanes) store_identity(pi_xy + j * G1_NTT_AFFINE_WORDS, pi_inf + j, 1, 0);
}
// P = c (f mod r), then n zeros, over the m 2n columns of [m][4][2n]
__global__ void __launch_bounds__(BLOCK) k_open_all_pad(const u64* coeffs, u64* padded, int log_n, size_t total, Scalar c) {
  const size_t n = elems(log_n), nn = wide(log_n), lanes = (size_t)gridDim.x * BLOCK;
  const Fp cc = from_scalar(c);
#pragma unroll 1
  for (size_t i = TID; i < total; i += lanes) {
    const size_t a = i >> wide_log(log_n), k = i & (nn - 1);
    Fp v = fp_from_limbs(0, 0, 0, 0, 0, 0, 0, 0);
    if (k < n) v = fr_mul(cc, fr_reduce_plain(load_plain(coeffs + a * FR_WORDS * n, n, k, 0)));
    store_plain(padded + a * FR_WORDS * nn, nn, k, 0, v);
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
// The pointwise products fused with stage 0 of the inverse transform of 2n points (every twiddle is 1) over items (array, butterfly):
// U = F_j T_j, V = F_(j+n) T_(j+n) from the affine table [8][2n] + [2n] and F [m][4][2n], out[2j] = U + V, out[2j + 1] = U - V into a projective
// buffer [12][stride].  tables: one region per lane of the launch, as k_g1_ntt_stage.
__global__ void HEAVY_BOUNDS k_open_all_first(const u64* txy, const uint8_t* tinf, const u64* f, u64* dst, int log_n, size_t total, size_t stride, uint8_t* tables) {
  const size_t n = elems(log_n), nn = wide(log_n), lanes = (size_t)gridDim.x * BLOCK;
  void* region = tables + TID * G1_TABLE_BYTES_PER_LANE;
#pragma unroll 1
  for (size_t b = TID; b < total; b += lanes) {
    const size_t a = b >> log_n, j = b & (n - 1);
    const u64* fa = f + a * FR_WORDS * nn;
    const G1P u = times(load_input(txy, tinf, nn, first_in0(j)), fa, nn, first_in0(j), region);
    const G1P v = times(load_input(txy, tinf, nn, first_in1(j, log_n)), fa, nn, first_in1(j, log_n), region);
    butterfly_store(dst, stride, first_out0(a, j, log_n), first_out1(a, j, log_n), to_core(u), to_core(v), fp_is_zero(v.z));
  }
}
// Stage 0 of the forward transform of n points over items (array, butterfly), reading h where the inverse transform of 2n points left it:
// U = h_j at column a 2n + j, V = h_(j + n/2) -- the identity for h_(n-1), whatever the buffer holds there -- and out[2j] = U + V,
// out[2j + 1] = U - V at columns a n + ... of the other buffer, same stride.
__global__ void __launch_bounds__(BLOCK) k_open_all_fwd_first(const u64* src, u64* dst, int log_n, size_t total, size_t stride) {
  const size_t hn = g1_ntt_plan::half(log_n), lanes = (size_t)gridDim.x * BLOCK;
#pragma unroll 1
  for (size_t b = TID; b < total; b += lanes) {
    const size_t a = b >> (log_n - 1), j = b & (hn - 1);
    G1W v = g1w_load_proj(src, stride, fwd_in1(a, j, log_n));
    const bool v_inf = fwd_in1_is_identity(j, log_n) || OpsF29::is_zero(v.z);
    v.x = OpsF29::select(v.x, OpsF29::zero(), v_inf);
    v.y = OpsF29::select(v.y, OpsF29::one(), v_inf);
    v.z = OpsF29::select(v.z, OpsF29::zero(), v_inf);
    butterfly_store(dst, stride, fwd_out0(a, j, log_n), fwd_out1(a, j, log_n), g1w_load_proj(src, stride, fwd_in0(a, j, log_n)), v, v_inf);
  }
}

static int32_t open_all(const uint64_t* txy, const uint8_t* tinf, const uint64_t* coeffs, int log_n, size_t m, long long max_blocks, uint64_t* y_out,
                        uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  int32_t rc = y_out ? sylow_hip_fr_ntt_batch(coeffs, log_n, m, /*inverse=*/0, nullptr, y_out, stream) : SYLOW_HIP_OK;
  if (rc != SYLOW_HIP_OK) return rc;
  if (trivial(log_n)) {
    k_open_all_trivial<<<dim3((unsigned)trivial_grid(m)), dim3(BLOCK), 0, st>>>(pi_xy, pi_inf, m);
    LAUNCHED();
  }
  const ScratchLayout l = scratch_layout(log_n, m, max_blocks);
  if (l.bytes > SAT / 2) return host::fail(hipErrorOutOfMemory, "scratch of the proofs at every point");
  host::Lease ws;
  rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  uint8_t* tables = ws.at<uint8_t>(l.tables);
  u64 *tw_wide = ws.at<u64>(l.tw_wide), *tw = ws.at<u64>(l.tw);
  u64* buf[2] = {ws.at<u64>(l.buf[0]), ws.at<u64>(l.buf[1])};
  u64 *padded = ws.at<u64>(l.padded), *f = ws.at<u64>(l.f);
  const size_t str = stride(log_n, m);
  const int L = wide_log(log_n);
  const ntt_plan::Words4 ni = ntt_plan::n_inverse(L);
  k_open_all_pad<<<dim3((unsigned)pad_grid(log_n, m)), dim3(BLOCK), 0, st>>>(coeffs, padded, log_n, str, Scalar{{ni.w[0], ni.w[1], ni.w[2], ni.w[3]}});
  rc = sylow_hip_fr_ntt_batch(padded, L, m, /*inverse=*/0, nullptr, f, stream);
  if (rc == SYLOW_HIP_OK) rc = ntth::build_table(L, tw_wide, stream);
  if (rc == SYLOW_HIP_OK && log_n >= 2) rc = ntth::build_table(log_n, tw, stream);
  if (rc == SYLOW_HIP_OK)
    k_open_all_first<<<dim3((unsigned)first_grid(log_n, m, max_blocks)), dim3(BLOCK), 0, st>>>(txy, tinf, f, buf[inv_dst(0)], log_n, first_items(log_n, m), str, tables);
  for (int s = 1; s < inv_stages(log_n) && rc == SYLOW_HIP_OK; ++s)
    rc = g1ntth::stage(buf[inv_src(s)], buf[inv_dst(s)], L, m, str, s, /*inverse=*/true, tw_wide, tables, max_blocks, stream);
  if (rc == SYLOW_HIP_OK) rc = kzoah::fwd_first(buf[fwd_src(log_n, 0)], buf[fwd_dst(log_n, 0)], log_n, m, str, max_blocks, stream);
  for (int s = 1; s < fwd_stages(log_n) && rc == SYLOW_HIP_OK; ++s)
    rc = g1ntth::stage(buf[fwd_src(log_n, s)], buf[fwd_dst(log_n, s)], log_n, m, str, s, /*inverse=*/false, tw, tables, max_blocks, stream);
  if (rc == SYLOW_HIP_OK) rc = g1ntth::close(buf[close_src(log_n)], log_n, m, str, pi_xy, pi_inf, max_blocks, stream);
  return host::finish(rc, ws);
}
}  // namespace kzoa

namespace kzoah {
// For kzg_cosets.hip, whose forward transform of c points reads h the same way: the launch of open_all() above with the caller's geometry
int32_t fwd_first(const uint64_t* src, uint64_t* dst, int log_n, size_t m, size_t stride, long long max_blocks, void* stream) {
  using namespace kzg_open_all_plan;
  kzoa::k_open_all_fwd_first<<<dim3((unsigned)fwd_grid(log_n, m, max_blocks)), dim3(BLOCK), 0, (hipStream_t)stream>>>(src, dst, log_n, fwd_items(log_n, m), stride);
  LAUNCHED();
}
}  // namespace kzoah

extern "C" {
int32_t sylow_hip_kzg_open_all_prepare(const uint64_t* srs_g1_xy, int32_t log_n, uint64_t* table_xy, uint8_t* table_inf, void* stream) {
  using namespace kzg_open_all_plan;
  ARGCHK(log_n_ok(log_n));
  ARGCHK(srs_g1_xy && table_xy && table_inf);
  host::Lease ws;
  const PrepareLayout l = prepare_layout(log_n);
  int32_t rc = ws.acquire(l.bytes, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  u64* xy = ws.at<u64>(l.xy);
  uint8_t* inf = ws.at<uint8_t>(l.inf);
  kzoa::k_open_all_x<<<dim3((unsigned)prepare_grid(log_n)), dim3(BLOCK), 0, (hipStream_t)stream>>>(srs_g1_xy, log_n, xy, inf);
  rc = sylow_hip_g1_ntt_batch(xy, inf, wide_log(log_n), 1, /*inverse=*/0, table_xy, table_inf, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_kzg_open_all_batch_tuned(const uint64_t* table_xy, const uint8_t* table_inf, const uint64_t* coeffs, int32_t log_n, size_t m, int64_t max_blocks,
                                           uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  using namespace kzg_open_all_plan;
  ARGCHK(log_n_ok(log_n) && max_blocks_ok(max_blocks));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(table_xy && coeffs && pi_xy && pi_inf);
  const size_t fb = fr_bytes(log_n, m), pb = pi_xy_bytes(log_n, m);
  ARGCHK(fb != SAT && pb != SAT && stride(log_n, m) != SAT);
  ARGCHK(!y_out || disjoint((uintptr_t)coeffs, fb, (uintptr_t)y_out, fb));                 // the Fr transform reads what other blocks of it write
  ARGCHK(disjoint((uintptr_t)coeffs, fb, (uintptr_t)pi_xy, pb) && disjoint((uintptr_t)table_xy, table_xy_bytes(log_n), (uintptr_t)pi_xy, pb));
  return kzoa::open_all(table_xy, table_inf, coeffs, log_n, m, max_blocks, y_out, pi_xy, pi_inf, stream);
}
int32_t sylow_hip_kzg_open_all_batch(const uint64_t* table_xy, const uint8_t* table_inf, const uint64_t* coeffs, int32_t log_n, size_t m, uint64_t* y_out,
                                     uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  return sylow_hip_kzg_open_all_batch_tuned(table_xy, table_inf, coeffs, log_n, m, -1, y_out, pi_xy, pi_inf, stream);
}
}  // extern "C"
