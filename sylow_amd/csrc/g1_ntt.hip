// g1_ntt.hip -- the batched radix-2 transform over G1 points (include/sylow_hip.h, "G1: transforms on radix-2 domains"): m arrays of
//   n = 2^log_n points, natural order in and out, forward  out_i = sum_k w^(ik) P_k  and inverse  out_k = n^-1 sum_i w^(-ik) P_i,  and the
//   Lagrange-basis KZG SRS as the inverse transform of the monomial one.
// A butterfly (U, V) -> (U + kV, U - kV) is one variable-base scalar multiplication (33 GLV windows: 128 doublings and 66 complete additions
// on the carry-free core, some 10^5 instructions) against 300 bytes moved, so the transform is bound by VALU issue: ONE radix-2 Stockham
// stage per launch, one butterfly per lane at a time, between two projective buffers in global memory -- no LDS tile.  Three kernels:
// stage 0 (every twiddle is 1: two additions per butterfly, affine points in), the stages after it (the multiplication skipped where the
// twiddle is 1, see g1_ntt_plan::butterfly_of for why whole wavefronts skip), and ONE closing kernel (n^-1 for the inverse, then affine +
// flags, one Fp inversion per point).  The twiddles are the table of the Fr transform, built by ntt.hip per call.
// Geometry, ping-pong, grids and scratch: g1_ntt_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "g1_ntt_plan.hpp"
#include "g1_ntt_dev.hpp"
#include "bn254_fr_dev.hpp"

namespace g1ntt {
using namespace g1_ntt_plan;
static_assert(G1_NTT_BLOCK == BLOCK, "the kernels run blocks of BLOCK lanes");
static_assert(G1_NTT_TABLE_BYTES_PER_LANE == G1_TABLE_BYTES_PER_LANE, "a lane's window table");

struct Scalar : FrArg {};      // a kernel names its parameter types in its symbol: this one stays a type of this namespace so that the symbol does not move
// Stage 0 over items (array, butterfly): U = in[j], V = in[j + n/2] from the caller's affine arrays [m][8][n] + [m][n], out[2j] = U + V,
// out[2j + 1] = U - V into a projective buffer [12][stride], array a at columns a n ...
__global__ void __launch_bounds__(BLOCK) k_g1_ntt_first(const u64* pxy, const uint8_t* pinf, u64* dst, int log_n, size_t total, size_t stride) {
  const size_t n = elems(log_n), lanes = (size_t)gridDim.x * BLOCK;
#pragma unroll 1
  for (size_t b = TID; b < total; b += lanes) {
    const size_t a = b >> (log_n - 1), j = butterfly_of(b & (half(log_n) - 1), log_n, 0), base = a << log_n;
    const u64* xy = pxy + a * G1_NTT_AFFINE_WORDS * n;
    const uint8_t* inf = pinf ? pinf + base : nullptr;
    const G1P u = load_input(xy, inf, n, in0(j)), v = load_input(xy, inf, n, in1(j, log_n));
    butterfly_store(dst, stride, base + out0(j, 0), base + out1(j, 0), to_core(u), to_core(v), fp_is_zero(v.z));
  }
}
// Stage `stage` >= 1, projective buffer to projective buffer.  tables: gridDim.x * BLOCK regions of G1_TABLE_BYTES_PER_LANE bytes, one per lane
// of the launch, reused for every butterfly the lane walks.  The skip is decided per work item: uniform over a wavefront wherever the
// stage has 64 groups or more.
__global__ void HEAVY_BOUNDS k_g1_ntt_stage(const u64* src, u64* dst, int log_n, int stage, size_t total, size_t stride, const u64* twiddles, int inverse,
                                            uint8_t* tables) {
  const size_t hn = half(log_n), lanes = (size_t)gridDim.x * BLOCK;
  void* region = tables + TID * G1_TABLE_BYTES_PER_LANE;
#pragma unroll 1
  for (size_t b = TID; b < total; b += lanes) {
    const size_t a = b >> (log_n - 1), j = butterfly_of(b & (hn - 1), log_n, stage), base = a << log_n, iv = base + in1(j, log_n);
    G1P v{load_fp(src, stride, iv, 0), load_fp(src, stride, iv, 4), load_fp(src, stride, iv, 8)};
    if (!unit_twiddle(j, stage)) {
      const size_t e = twiddle_exp(j, log_n, stage);               // 0 < e < n / 2
      const Fp w = inverse ? fr_neg(load_plain(twiddles, hn, hn - e, 0)) : load_plain(twiddles, hn, e, 0);
      u32 k[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) k[q] = w.v[q];
      v = g1_scalar_mul_ws(v, k, region);
    }
    const bool v_inf = fp_is_zero(v.z);
    v.x = fp_select(v.x, fp_zero(), v_inf);
    v.y = fp_select(v.y, fp_one(), v_inf);
    butterfly_store(dst, stride, base + out0(j, stage), base + out1(j, stage), g1w_load_proj(src, stride, base + in0(j)), to_core(v), v_inf);
  }
}
// The closing kernel over the m n points: from the last stage's buffer (src_affine = 0) or, at n = 1, from the caller's arrays; SCALE: times
// c = n^-1 first; then affine + flag, the identity as (0, 1) + 1, into the caller's [m][8][n] + [m][n].
template <bool SCALE>
__global__ void HEAVY_BOUNDS k_g1_ntt_close(const u64* src, const uint8_t* pinf, int src_affine, u64* oxy, uint8_t* oinf, int log_n, size_t total, size_t stride,
                                            Scalar c, uint8_t* tables) {
  const size_t n = elems(log_n), lanes = (size_t)gridDim.x * BLOCK;
#pragma unroll 1
  for (size_t i = TID; i < total; i += lanes) {
    const size_t a = i >> log_n, k = i & (n - 1);
    G1P p = src_affine ? load_input(src + a * G1_NTT_AFFINE_WORDS * n, pinf ? pinf + (a << log_n) : nullptr, n, k)
                       : G1P{load_fp(src, stride, i, 0), load_fp(src, stride, i, 4), load_fp(src, stride, i, 8)};
    if (SCALE) {
      const u32 kk[8] = {(u32)c.w[0], (u32)(c.w[0] >> 32), (u32)c.w[1], (u32)(c.w[1] >> 32), (u32)c.w[2], (u32)(c.w[2] >> 32), (u32)c.w[3], (u32)(c.w[3] >> 32)};
      p = g1_scalar_mul_ws(p, kk, tables + TID * G1_TABLE_BYTES_PER_LANE);
    }
    Fp x, y; bool inf;
    g1_to_affine(x, y, inf, p);
    u64* out = oxy + a * G1_NTT_AFFINE_WORDS * n;
    store_fp(out, n, k, 0, x); store_fp(out, n, k, 4, y);
    oinf[i] = inf ? 1 : 0;
  }
}

static int32_t transform(const uint64_t* p_xy, const uint8_t* p_inf, int log_n, size_t m, bool inverse, long long max_blocks, uint64_t* out_xy, uint8_t* out_inf,
                         void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const ScratchLayout l = scratch_layout(log_n, m, inverse, max_blocks);
  if (l.bytes > SAT / 2) return host::fail(hipErrorOutOfMemory, "scratch of the G1 transform");
  host::Lease ws;
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  uint8_t* tables = ws.at<uint8_t>(l.tables);
  u64* twiddles = ws.at<u64>(l.twiddles);
  u64* buf[2] = {ws.at<u64>(l.buf[0]), ws.at<u64>(l.buf[1])};
  const size_t stride = points(log_n, m), total = butterflies(log_n, m);
  if (log_n >= 2) rc = ntth::build_table(log_n, twiddles, stream);
  for (int s = 0; s < stages(log_n) && rc == SYLOW_HIP_OK; ++s) {
    const dim3 g((unsigned)stage_grid(log_n, m, max_blocks));
    if (!stage_multiplies(s)) k_g1_ntt_first<<<g, dim3(BLOCK), 0, st>>>(p_xy, p_inf, buf[stage_dst(s)], log_n, total, stride);
    else k_g1_ntt_stage<<<g, dim3(BLOCK), 0, st>>>(buf[stage_src(s)], buf[stage_dst(s)], log_n, s, total, stride, twiddles, inverse ? 1 : 0, tables);
  }
  if (rc == SYLOW_HIP_OK) {
    const dim3 g((unsigned)closing_grid(log_n, m, max_blocks));
    const int from = closing_src(log_n);
    const u64* src = from == SRC_INPUT ? p_xy : buf[from];
    const ntt_plan::Words4 ni = ntt_plan::n_inverse(log_n);
    const Scalar c = {{ni.w[0], ni.w[1], ni.w[2], ni.w[3]}};
    if (closing_scales(log_n, inverse)) k_g1_ntt_close<true><<<g, dim3(BLOCK), 0, st>>>(src, p_inf, from == SRC_INPUT, out_xy, out_inf, log_n, stride, stride, c, tables);
    else k_g1_ntt_close<false><<<g, dim3(BLOCK), 0, st>>>(src, p_inf, from == SRC_INPUT, out_xy, out_inf, log_n, stride, stride, c, nullptr);
  }
  return host::finish(rc, ws);
}
}  // namespace g1ntt

namespace g1ntth {
// For a unit that runs part of a transform on projective buffers of its own (kzg_open_all.hip): the launches of transform() above, one at a
// time, with the caller's geometry.  Arrays of 2^log_n points, array a at columns a 2^log_n of a buffer [12][stride]; `tables` holds a window
// table for every lane of g1_ntt_plan::stage_grid(log_n, m, max_blocks) blocks.
int32_t stage(const uint64_t* src, uint64_t* dst, int log_n, size_t m, size_t stride, int stage, bool inverse, const uint64_t* twiddles, uint8_t* tables,
              long long max_blocks, void* stream) {
  using namespace g1_ntt_plan;
  g1ntt::k_g1_ntt_stage<<<dim3((unsigned)stage_grid(log_n, m, max_blocks)), dim3(BLOCK), 0, (hipStream_t)stream>>>(src, dst, log_n, stage, butterflies(log_n, m), stride,
                                                                                                                 twiddles, inverse ? 1 : 0, tables);
  LAUNCHED();
}
int32_t close(const uint64_t* src, int log_n, size_t m, size_t stride, uint64_t* out_xy, uint8_t* out_inf, long long max_blocks, void* stream) {
  using namespace g1_ntt_plan;
  g1ntt::k_g1_ntt_close<false><<<dim3((unsigned)closing_grid(log_n, m, max_blocks)), dim3(BLOCK), 0, (hipStream_t)stream>>>(src, nullptr, 0, out_xy, out_inf, log_n,
                                                                                                                          points(log_n, m), stride, g1ntt::Scalar{}, nullptr);
  LAUNCHED();
}
}  // namespace g1ntth

extern "C" {
int32_t sylow_hip_g1_ntt_batch_tuned(const uint64_t* p_xy, const uint8_t* p_inf, int32_t log_n, size_t m, int32_t inverse, int64_t max_blocks,
                                     uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  using namespace g1_ntt_plan;
  ARGCHK(log_n_ok(log_n) && (inverse == 0 || inverse == 1) && max_blocks_ok(max_blocks));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(p_xy && out_xy && out_inf);
  const size_t bytes = xy_bytes(log_n, m);
  ARGCHK(bytes != SAT);
  ARGCHK(disjoint((uintptr_t)p_xy, (uintptr_t)out_xy, bytes));                           // other lanes still read what this one writes
  ARGCHK(!p_inf || disjoint((uintptr_t)p_inf, (uintptr_t)out_inf, inf_bytes(log_n, m)));
  return g1ntt::transform(p_xy, p_inf, log_n, m, inverse != 0, max_blocks, out_xy, out_inf, stream);
}
int32_t sylow_hip_g1_ntt_batch(const uint64_t* p_xy, const uint8_t* p_inf, int32_t log_n, size_t m, int32_t inverse, uint64_t* out_xy, uint8_t* out_inf,
                               void* stream) {
  return sylow_hip_g1_ntt_batch_tuned(p_xy, p_inf, log_n, m, inverse, -1, out_xy, out_inf, stream);
}
int32_t sylow_hip_kzg_srs_lagrange(const uint64_t* srs_g1_xy, int32_t log_n, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  return sylow_hip_g1_ntt_batch_tuned(srs_g1_xy, nullptr, log_n, 1, 1, -1, out_xy, out_inf, stream);
}
}  // extern "C"
