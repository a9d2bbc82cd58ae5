// g2_msm.hpp -- the ways of collapsing many G2 points into one: sum_i Q_i, n_jobs weighted sums, and one large multi-scalar multiplication
// Q = sum_i k_i Q_i by the bucket method of msm_bucket.hpp on LANE PAIRS (bn254_pair.hpp: lane l and lane 7 - l of a group of 8 each hold one
// Fp coordinate of every Fp2 value; a projective point is 27 VGPRs per lane).
//
// The scalars are NOT reduced mod r (MOD_R = false): the digits are those of k mod p itself.  A point of E(Fp) has order r, a point of the
// twist need not (the twist's group order is r times a cofactor), and the contract is that of sylow_hip_g2_scalar_mul_batch: the product is
// exact on the whole twist.  k mod p < 2^254 and W c >= 255 still leave no carry out of the top window.
//
// The buckets live on the ISOMORPHIC twist E'' (g2q_to_iso, plk_group.hip): the two Fp scalings are paid once per point in k_msm_prep, and each
// of the W additions of a point then uses OpsW2I, where 3 b'' is one reduce pass and not a product leaf.  k_msm_combine ends with g2q_from_iso
// and ONE normalisation to canonical affine words + flag.
// This file is the tail of the unit plk_group.hip (included at its end): the build has no relocatable device code, and the policy here uses that
// unit's G2 group law on lane pairs (OpsW2I, g2q_to_iso / g2q_from_iso, store_g2q_affine) and its segmented sum.
// tools/msm_model.py (g2_* functions) is the host-side model of the recoding, the plan and the scratch formula (tests/test_g2_msm_model.py).
#pragma once
#include "msm_bucket.hpp"

namespace plk {
// the geometry policy of msm_bucket.hpp for G2: one lane pair per point, each lane on its own Fp coordinate of the Fp2 values
struct G2Pair {
  typedef W2 F;
  typedef OpsW2I Ops;                                       // on E''
  static constexpr int LANES = 2;
  static constexpr bool MOD_R = false;
  // the smallest measured size from which the bucket route beats sylow_hip_g2_scalar_mul_batch + the sum at every larger size:
  // 2^16 1.5 x, 2^15 0.72 x
  static constexpr size_t DEFAULT_MIN = (size_t)1 << 16;
  static constexpr size_t WIDE_FROM = (size_t)1 << 16;      // from this n on the default window is WIDE_C
  static constexpr int WIDE_C = 15;
  // k_msm_bucket_reduce at one wave per SIMD: three live points (run, acc, q or an operand: 81 VGPRs per lane) and an addition's temporaries
  // do not fit in the 256 registers of HEAVY_BOUNDS without spilling, and W T lane pairs are a few hundred wavefronts.
  static constexpr int REDUCE_WAVES = 1;
  static constexpr const char* CHUNK_LAUNCH = "g2 msm chunk launch";
  // The default window: the rule of sylow_hip_g1_msm below 2^16, c = 15 from there on.  The sweep of c at 2^16 and 2^20 has
  // c = 15 fastest at both sizes, and the G1 rule's c = 13 for 2^16 and 2^17 3.6 x slower than it: the 7-bit top window of c = 13 puts every
  // point of that window into 64 buckets of ONE tile, which k_msm_seg_join_wide joins one after the other.
  static int default_window(size_t n) { return n >= WIDE_FROM ? WIDE_C : msm::default_window(n); }
  template <class T> static BN_DEV T elem(T t) { return pair_index(t); }
  template <class T> static BN_DEV int role(T t) { return pair_role(t); }
  static BN_DEV F wrap(const F29& a) { return W2{a}; }
  static BN_DEV const F29& limbs(const F& a) { return a.c; }
  static BN_DEV G2Q prepare(const u64* pxy, size_t n, size_t i, int odd) {
    return g2q_to_iso(G2Q{w2_from_s2(load_s2(pxy, n, i, 0, odd)), w2_from_s2(load_s2(pxy, n, i, 8, odd)), OpsW2::one()});
  }
  static BN_DEV void finish(u64* oxy, uint8_t* oinf, int odd, const G2Q& acc) { store_g2q_affine(oxy, oinf, 1, 0, odd, g2q_from_iso(acc)); }
};
}  // namespace plk

namespace g2msmh {
// k_i Q_i per lane pair (exact on the whole twist), then the segmented sum: n_seg sums of c terms each, term-major
int32_t composed(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n_seg, size_t c, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  const size_t n = n_seg * c, acc_words = plkh::g2_sum_scratch_words(n_seg, c);
  host::Lease ws;
  int32_t rc = ws.acquire((acc_words + 16 * n) * sizeof(u64) + n + 256, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint64_t* acc = (uint64_t*)ws.p;
  uint64_t* xy = acc + acc_words;
  uint8_t* inf = (uint8_t*)(xy + 16 * n);
  if (n) rc = sylow_hip_g2_scalar_mul_batch(p_xy, p_inf, k, xy, inf, n, stream);
  if (rc == SYLOW_HIP_OK) rc = plkh::g2_sum(xy, inf, n_seg, c, acc, out_xy, out_inf, stream);
  return host::finish(rc, ws);
}
}  // namespace g2msmh

extern "C" {
int32_t sylow_hip_g2_sum_batch(const uint64_t* q_xy, const uint8_t* q_inf, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  ARGCHK(out_xy && out_inf && (n == 0 || q_xy));
  host::Lease ws;
  int32_t rc = ws.acquire(plkh::g2_sum_scratch_words(1, n) * sizeof(u64) + 256, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  rc = plkh::g2_sum(q_xy, q_inf, 1, n, (uint64_t*)ws.p, out_xy, out_inf, stream);
  return host::finish(rc, ws);
}
int32_t sylow_hip_g2_lincomb_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, uint64_t* out_xy, uint8_t* out_inf,
                                   size_t n_jobs, size_t n_terms, void* stream) {
  ARGCHK(out_xy && out_inf && (n_jobs * n_terms == 0 || (p_xy && k)));
  if (!n_jobs) return SYLOW_HIP_OK;
  return g2msmh::composed(p_xy, p_inf, k, n_jobs, n_terms, out_xy, out_inf, stream);
}
int32_t sylow_hip_g2_msm_tuned(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, int32_t window, int64_t min_n_arg,
                               uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  // small n (or a budget below one chunk of the bucket route): a scalar multiplication per lane pair, then the segmented sum with one segment
  return msm::tuned<plk::G2Pair>(p_xy, p_inf, k, n, window, min_n_arg, out_xy, out_inf, stream,
                                    [&] { return g2msmh::composed(p_xy, p_inf, k, 1, n, out_xy, out_inf, stream); });
}
int32_t sylow_hip_g2_msm(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  return sylow_hip_g2_msm_tuned(p_xy, p_inf, k, n, -1, -1, out_xy, out_inf, stream);
}
}  // extern "C"
