// bn254_fr_acc.hpp -- the unreduced multiply-accumulate over Fr shared by the units that add many products before one reduction:
// k_fr_spmv (groth16_prove.hip), k_fr_lincomb (kzg_multi.hip) and the mix of Poseidon (poseidon.hip).  Included after common.hpp.
#pragma once
#include "bn254_fr.hpp"

namespace bn254 {
// acc += a b, no reduction.  THE BOUND: a and b are canonical, below r < 2^254, so a product is below r^2 < 2^508, and so is a residue the
// accumulator was folded to (r < r^2).  The caller adds at most 16 such terms (SPMV_FLUSH, LINCOMB_FLUSH) between two folds: acc < 16 r^2 < 2^512, which is
// what 16 limbs hold and what fr_reduce_wide takes.  (r^2 < 0.58 2^508, so up to 27 products of canonical values fit: the mix of Poseidon at
// t = 17 adds 17 to a zeroed accumulator, 17 (r - 1)^2 + (r - 1) < 2^512, and restates that beside its call in poseidon.hip.)  Hence the top limb takes the last carry without a carry out, and the column sums below
// stay in the 64 + 32 bits of (c, ovf): a column has at most 8 products and one limb of acc.
BN_DEV void mul_acc(u32 (&acc)[16], const Fp& a, const Fp& b) {
  u64 c = 0;
  u32 ovf = 0;
#pragma unroll
  for (int k = 0; k < 15; ++k) {
    c += acc[k];                                              // c < 2^36 here: the carry of the column before
#pragma unroll
    for (int i = (k > 7 ? k - 7 : 0); i <= (k < 7 ? k : 7); ++i) mac(c, ovf, a.v[i], b.v[k - i]);
    acc[k] = (u32)c;
    c = (c >> 32) | ((u64)ovf << 32);
    ovf = 0;
  }
  acc[15] += (u32)c;
}
}  // namespace bn254
