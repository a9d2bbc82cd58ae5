// kzg_scan_dev.hpp -- the device routines of the Horner scan behind the KZG quotient, shared by the units that run it: kzg_prove.hip (one point per
// polynomial) and kzg_points.hip (several points per polynomial).  Both compile this text; the geometry is kzg_prove_plan.hpp's.  Included after
// host.hpp.
#pragma once
#include "bn254_fr_dev.hpp"
#include "kzg_prove_plan.hpp"

namespace kzg_scan {
using namespace kzg_plan;
static_assert(KZG_POLY_BLOCK == BLOCK, "the quotient kernels run one chunk per block of BLOCK lanes");
constexpr int L = KZG_POLY_LANE_COEFFS, CH = (int)KZG_POLY_CHUNK;
constexpr int LOG_L = __builtin_ctz((unsigned)L), LOG_BLOCK = __builtin_ctz((unsigned)BLOCK);

// pw[s] = z^(2^(FROM + s)), s = 0 .. LOG_BLOCK - 1: the multipliers of a block scan whose elements are 2^FROM coefficients apart.  A chain of
// squarings, so ONE wavefront walks it (the branch is wave-uniform) while the others load; the caller's next barrier publishes it.
template <int FROM>
BN_DEV void block_powers(const Fp& z, u32 (*pw)[8]) {
  if (threadIdx.x >= 64) return;
  Fp p = z;
#pragma unroll 1
  for (int s = 0; s < FROM + LOG_BLOCK; ++s) {
    if (s >= FROM && threadIdx.x == 0) lds_put(pw, s - FROM, p);
    if (s + 1 < FROM + LOG_BLOCK) p = fr_mul(p, p);
  }
}
// Every thread of the block calls it (lanes whose value is zero included: they stay through every barrier).  SCAN: lane t gets
// S_t = sum_{u >= t} v_u x^(u - t) with x^(2^s) = pw[s] -- step s adds pw[s] S_{t + 2^s}; !SCAN: only lane 0's S_0 is formed (a tree).  Lanes
// from `live` on hold zero and are never read.
template <bool SCAN>
BN_DEV Fp block_suffix(Fp v, const u32 (*pw)[8], u32 (*part)[8], int live) {
  const int t = threadIdx.x;
  lds_put(part, t, v);
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < LOG_BLOCK; ++s) {
    const int off = 1 << s;
    const bool on = (SCAN ? true : (t & (2 * off - 1)) == 0) && t + off < live;
    if (on) v = fr_add(v, fr_mul(lds_get(part, t + off), lds_get(pw, s)));
    __syncthreads();
    if (on) lds_put(part, t, v);
    __syncthreads();
  }
  return v;
}
// coefficient k of the polynomial at f (an Fr SoA array of stride len), mod r
BN_DEV Fp coeff(const u64* f, size_t len, size_t k) { return fr_reduce_plain(load_plain(f, len, k, 0)); }
// sum_{i < L} f_{a + i} z^i, coefficients past len as zero
BN_DEV Fp lane_value(const u64* f, size_t len, size_t a, const Fp& z) {
  Fp v = fr_zero();
  if (a >= len) return v;
#pragma unroll 1
  for (int i = L - 1; i >= 0; --i)
    if (a + i < len) v = fr_add(fr_mul(v, z), coeff(f, len, a + i));
  return v;
}
// lanes of chunk c that own a coefficient (the tail chunk of every polynomial has fewer than BLOCK)
BN_DEV int live_lanes(size_t len, size_t c) {
  const size_t left = len - c * CH;
  return left >= (size_t)CH ? BLOCK : (int)((left + L - 1) / L);
}
}  // namespace kzg_scan
