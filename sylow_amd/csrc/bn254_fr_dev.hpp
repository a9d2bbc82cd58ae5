// bn254_fr_dev.hpp -- the small Fr device helpers every Fr-side unit needs, once: the constants, an Fr value through LDS, through a
// kernel argument and through a shuffle, powers, and a root out of the transform's table.  All forced inline: a unit that includes this
// compiles the same device code as one that spells them out.  Included after host.hpp or common.hpp.
#pragma once
#include "common.hpp"
#include "ntt_plan.hpp"

namespace bn254 {

BN_DEV Fp fr_zero() { return fp_from_limbs(0, 0, 0, 0, 0, 0, 0, 0); }
BN_DEV Fp fr_one() { return fp_from_limbs(1, 0, 0, 0, 0, 0, 0, 0); }
// an Fr value in a row of 8 dwords of LDS
BN_DEV Fp lds_get(const u32 (*a)[8], int i) { return fp_from_limbs(a[i][0], a[i][1], a[i][2], a[i][3], a[i][4], a[i][5], a[i][6], a[i][7]); }
BN_DEV void lds_put(u32 (*a)[8], int i, const Fp& v) {
#pragma unroll
  for (int w = 0; w < 8; ++w) a[i][w] = v.v[w];
}
struct FrArg {         // an Fr value as a kernel argument
  u64 w[4];
};
BN_DEV Fp from_scalar(const FrArg& s) {
  return fp_from_limbs((u32)s.w[0], (u32)(s.w[0] >> 32), (u32)s.w[1], (u32)(s.w[1] >> 32), (u32)s.w[2], (u32)(s.w[2] >> 32), (u32)s.w[3], (u32)(s.w[3] >> 32));
}
BN_DEV Fp shfl_xor_fp(const Fp& a, int off) {
  Fp r;
#pragma unroll
  for (int w = 0; w < 8; ++w) r.v[w] = __shfl_xor(a.v[w], off);
  return r;
}
// b^e by squaring, one round per bit of e up to its top set bit
BN_DEV Fp fr_pow(Fp b, u64 e) {
  Fp p = fr_one();
#pragma unroll 1
  for (; e; e >>= 1) {
    if (e & 1) p = fr_mul(p, b);
    b = fr_mul(b, b);
  }
  return p;
}
// v^i for i < c from the table of the transform of c points (ntth::build_table): v^(e + c / 2) = -v^e; 1 at c = 1, where there is no table
BN_DEV Fp fr_root_from_half_table(const u64* roots, int log_c, size_t i) {
  if (log_c < 1) return fr_one();
  const Fp p = load_plain(roots, ntt_plan::elems(log_c - 1), ntt_plan::root_slot(i, log_c), 0);
  return ntt_plan::root_negated(i, log_c) ? fr_neg(p) : p;
}

}  // namespace bn254
