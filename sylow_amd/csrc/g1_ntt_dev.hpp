// g1_ntt_dev.hpp -- the device helpers the units that run butterflies over G1 points share (g1_ntt.hip, kzg_open_all.hip, kzg_cosets.hip):
// how an input point is read, how the identity and a butterfly's two sums are stored.  Each unit compiles its own kernels around them (no
// relocatable device code).
#pragma once
#include "common.hpp"
#include "g1_ntt_plan.hpp"

namespace g1ntt {
// An input point.  The identity is a flagged point, whatever its words hold, or the pair (0, 1) that every call of this library writes for
// it (no point of the curve: 1 != 3) with or without its flag.  It joins as the canonical (0 : 1 : 0).
BN_DEV G1P load_input(const u64* xy, const uint8_t* inf, size_t n, size_t i) {
  G1P p = load_g1_flagged(xy, inf, n, i);                 // a flagged point comes back as (0 : 1 : 0): the test below holds for it too
  p.z = fp_select(p.z, fp_zero(), fp_is_zero(p.x) && fp_eq(p.y, fp_one()));
  return p;
}
// the identity as every call of this library writes it: the words (0, 1) and the flag; affine SoA of stride n
BN_DEV void store_identity(u64* xy, uint8_t* inf, size_t n, size_t i) {
#pragma unroll
  for (int w = 0; w < (int)g1_ntt_plan::G1_NTT_AFFINE_WORDS; ++w) xy[(size_t)w * n + i] = w == 4 ? 1 : 0;
  inf[i] = 1;
}
BN_DEV G1W to_core(const G1P& p) { return G1W{f29_from_fp_reduced(p.x), f29_from_fp_reduced(p.y), f29_from_fp_reduced(p.z)}; }
// Every intermediate with Z = 0 is stored as (0 : 1 : 0): the complete formulas keep Z = 0 only for that representative across consecutive
// additions (bn254_pairing.hpp: g1_scalar_mul_t), and U - V with U = V makes identities that feed the later stages
BN_DEV void store_canonical(u64* a, size_t stride, size_t i, const G1W& r) {
  const bool inf = OpsF29::is_zero(r.z);
  g1w_store_proj(a, stride, i, G1W{OpsF29::select(r.x, OpsF29::zero(), inf), OpsF29::select(r.y, OpsF29::one(), inf), r.z});
}
BN_DEV void butterfly_store(u64* dst, size_t stride, size_t o0, size_t o1, const G1W& u, G1W v, bool v_inf) {
  store_canonical(dst, stride, o0, proj_add_lazy<OpsF29>(u, v));
  v.y = OpsF29::select(OpsF29::neg(v.y), OpsF29::one(), v_inf);
  store_canonical(dst, stride, o1, proj_add_lazy<OpsF29>(u, v));
}
}  // namespace g1ntt
