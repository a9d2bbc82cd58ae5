// bn254_fr_block.hpp -- what a block of BLOCK lanes does together over Fr, once, for the units that walk an array chunk by chunk
// (kzg_evals.hip, fr_scan.hip) or add a column up in two levels (the weighted checks): an element of a struct-of-arrays row mod r, the
// inverse of one value on a lone lane, the inverses of the lane totals of a chunk through ONE inversion, the sum of the lane values, the
// join of a column's partial sums, and the prefix of the lane totals under + or *.  The lanes that take part and the doubling
// steps are kzg_evals_plan.hpp's.  All but the lone inversion are forced inline: a unit that includes this compiles the same device code as
// one that spells them out.  Included after host.hpp or common.hpp.
#pragma once
#include "bn254_fr_euclid.hpp"
#include "bn254_fr_dev.hpp"
#include "kzg_evals_plan.hpp"

namespace bn254 {

// element k of an Fr SoA array of stride n, mod r
BN_DEV Fp elem(const u64* a, size_t n, size_t k) { return fr_reduce_plain(load_plain(a, n, k, 0)); }
// the inverse of ONE nonzero canonical value, for a lone lane: binary extended Euclid, no product (bn254_fr_euclid.hpp)
BN_NOINLINE Fp fr_inv_lone(Fp a) {
  Fp o;
  fr_euclid::inverse(a.v, o.v);
  return o;
}

// Every thread of the block calls it.  Lane t < live brings T_t != 0, the product of its elements; it gets T_t^-1.  Two scans run side by
// side through LDS -- step s multiplies the prefix by the one 2^s lanes below and the suffix by the one 2^s lanes above -- so that pre[t] =
// T_0 .. T_t and suf[t] = T_t .. T_(live-1); the top live lane holds the chunk's product and inverts it alone; then
// T_t^-1 = (T_0 .. T_(live-1))^-1 pre[t - 1] suf[t + 1].  Lanes from `live` on hold nothing and are never read.  The caller's next barrier
// frees pre, suf and inv.
BN_DEV Fp block_inverses(const Fp& T, u32 (*pre)[8], u32 (*suf)[8], u32 (*inv)[8], int live) {
  const int t = threadIdx.x;
  const bool on = t < live;
  Fp P = T, S = T;
  if (on) {
    lds_put(pre, t, P);
    lds_put(suf, t, S);
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < kzg_evals_plan::scan_steps(live); ++s) {
    const int off = 1 << s;
    const bool lo = on && t >= off, hi = on && t + off < live;
    if (lo) P = fr_mul(P, lds_get(pre, t - off));
    if (hi) S = fr_mul(S, lds_get(suf, t + off));
    __syncthreads();
    if (lo) lds_put(pre, t, P);
    if (hi) lds_put(suf, t, S);
    __syncthreads();
  }
  if (t == live - 1) lds_put(inv, 0, fr_inv_lone(P));
  __syncthreads();
  Fp r = fr_one();
  if (on) {
    r = lds_get(inv, 0);
    if (t > 0) r = fr_mul(r, lds_get(pre, t - 1));
    if (t + 1 < live) r = fr_mul(r, lds_get(suf, t + 1));
  }
  return r;
}

// Every thread of the block calls it: lane 0 gets the sum of the block's values mod r (the other lanes partial sums).  A modular sum is
// exact and canonical: the order of the tree does not show in the words.  Ends on a barrier, so `part` is free for the next call.
BN_DEV Fp block_sum(Fp v, u32 (*part)[8]) {
  const int t = threadIdx.x;
  lds_put(part, t, v);
  __syncthreads();
#pragma unroll 1
  for (int off = BLOCK / 2; off > 0; off >>= 1) {
    if (t < off) {                                             // reads rows off .. 2 off - 1, writes rows below off
      v = fr_add(v, lds_get(part, t + off));
      lds_put(part, t, v);
    }
    __syncthreads();
  }
  return v;
}
// The join of the weighted checks, a block per column: lane 0 gets the sum of the `parts` partials of column c of partial [4][cols * parts]
// (the partial of (column, part) at index column * parts + part), what the blocks of the level before left through block_sum.
BN_DEV Fp column_sum(const u64* partial, size_t cols, size_t parts, size_t c, u32 (*part)[8]) {
  Fp acc = fr_zero();
#pragma unroll 1
  for (size_t k = threadIdx.x; k < parts; k += BLOCK) acc = fr_add(acc, load_plain(partial, cols * parts, c * parts + k, 0));
  return block_sum(acc, part);
}

// The two operations of a scan over Fr: PRODUCT false is +, with the identity 0; true is *, with the identity 1.
template <bool PRODUCT> BN_DEV Fp fr_scan_identity() { return PRODUCT ? fr_one() : fr_zero(); }
template <bool PRODUCT> BN_DEV Fp fr_scan_op(const Fp& a, const Fp& b) { return PRODUCT ? fr_mul(a, b) : fr_add(a, b); }
// Every thread of the block calls it, 1 <= live <= BLOCK.  Lane t < live brings T_t, canonical; it gets T_0 o .. o T_(t-1), the identity at
// t = 0, and EVERY lane gets total = T_0 o .. o T_(live-1).  One scan through LDS by doubling steps.  Lanes from `live` on get the identity
// and are never read.  The caller's next barrier frees buf.
template <bool PRODUCT> BN_DEV Fp block_prefix(const Fp& T, u32 (*buf)[8], int live, Fp& total) {
  const int t = threadIdx.x;
  const bool on = t < live;
  Fp P = T;
  if (on) lds_put(buf, t, P);
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < kzg_evals_plan::scan_steps(live); ++s) {
    const int off = 1 << s;
    const bool lo = on && t >= off;
    if (lo) P = fr_scan_op<PRODUCT>(P, lds_get(buf, t - off));
    __syncthreads();
    if (lo) lds_put(buf, t, P);
    __syncthreads();
  }
  total = lds_get(buf, live - 1);
  return on && t > 0 ? lds_get(buf, t - 1) : fr_scan_identity<PRODUCT>();
}

}  // namespace bn254
