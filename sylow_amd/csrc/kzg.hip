// kzg.hip -- the G1 / Fr side of batched KZG opening verification on BN254 under ONE SRS (include/sylow_hip.h, "KZG"):
//   F_i = C_i - y_i G1gen + z_i pi_i for n openings in one launch (the fold: the pairing check is then e(F_i, G2gen) e(-pi_i, tau_g2) == 1,
//   the shape of the same-signer BLS check, whose entry points live with the fused kernel they launch: plk_verify.hip),
//   the Fr preparation of the weighted one-boolean test, and that test itself, composed from the library's own stream-ordered calls.
#include "host.hpp"
#include "bn254_fr_block.hpp"
#include "weighted_plan.hpp"

namespace kzg {
static_assert(weighted_plan::WEIGHTED_BLOCK == BLOCK, "the preparation runs a lane per opening in blocks of BLOCK lanes");
// any 256-bit word -> its residue mod r as eight limbs (the rule of sylow_hip_evm_ecmul_batch)
BN_DEV void load_scalar_mod_r(u32 (&k)[8], const u64* base, size_t n, size_t i) {
  const Fp s = fr_reduce_plain(load_plain(base, n, i, 0));
#pragma unroll
  for (int j = 0; j < 8; ++j) k[j] = s.v[j];
}
// The signed 4-bit digits of glv_digits (bn254_pairing.hpp) without a digit array: with b = m + 0x8 8888 ... 8 (33 nibbles of 8),
// m = sum_i (nibble_i(b) - 8) 16^i, every digit in [-8, 7] -- the same digits, since that representation is unique -- and the top one
// (m < 2^128) is 0 or 1.  The walk below reads digit i as a select chain over the five words: nothing is indexed dynamically, so no
// stack frame.
BN_DEV void glv_bias(u32 (&b)[5], const u32 (&m)[4]) {
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { c += (u64)m[i] + 0x88888888u; b[i] = (u32)c; c >>= 32; }
  b[4] = (u32)c + 8u;
}
BN_DEV int glv_digit(const u32 (&b)[5], int i) {
  u32 w = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q) if (q == (i >> 3)) w = b[q];
  return (int)((w >> (4 * (i & 7))) & 15u) - 8;
}
// k P on the carry-free core, the schedule of g1_scalar_mul_t (GLV split, 33 windows of four doublings and two complete additions, one
// table of 0P..8P in the lane's region of a leased block), left PROJECTIVE in the accumulator the rest of the fold adds to.  t1 is P with a
// flagged identity already the canonical (0 : 1 : 0); k < r.
BN_DEV G1W glv_walk(G1W t1, const u32 (&k)[8], G1TableGlobal& tab) {
  u32 m1[4], m2[4], b1[5], b2[5];
  bool n1, n2;
  glv_decompose(m1, n1, m2, n2, k);
  glv_bias(b1, m1);
  glv_bias(b2, m2);
  // beta 2^261 mod p
  const F29 beta{{0x18ccb791, 0x175b1c3a, 0x0b83d6e2, 0x0e8ed071, 0x1282bee2, 0x04220e84, 0x1fe4017f, 0x15084d4a, 0x00169119}};
  auto dbl = [](const G1W& a) { return proj_double_lazy<OpsF29I>(a); };
  auto add = [](const G1W& a, const G1W& b) { return proj_add_lazy<OpsF29I>(a, b); };
  {
    if (n1) t1.y = OpsF29::neg(t1.y);                    // the table holds multiples of sign(k1) P
    // 2P .. 8P with P and ONE more point live (the straight-line form of scalar_mul_window holds five: 135 registers): 4P comes
    // from the stored 2P -- a lane reads back its own store
    tab.put(0, proj_zero<OpsF29>());
    tab.put(1, t1);
    G1W a = proj_double_lazy<OpsF29>(t1);
    tab.put(2, a);
    a = proj_add_lazy<OpsF29>(a, t1);
    tab.put(3, a);
    a = proj_double_lazy<OpsF29>(a);
    tab.put(6, a);
    tab.put(7, proj_add_lazy<OpsF29>(a, t1));
    a = proj_double_lazy<OpsF29>(tab.get(2));
    tab.put(4, a);
    tab.put(5, proj_add_lazy<OpsF29>(a, t1));
    tab.put(8, proj_double_lazy<OpsF29>(a));
  }
  const bool flip2 = n1 != n2;                            // phi(table) carries sign(k1); k2 wants sign(k2)
  G1W res = proj_zero<OpsF29>();
#pragma unroll 1
  for (int i = 32; i >= 0; --i) {
    if (i != 32) {
#pragma unroll 1
      for (int j = 0; j < 4; ++j) res = dbl(res);
    }
    {
      const int d = glv_digit(b1, i), m = d < 0 ? -d : d;
      G1W q = tab.get(m);
      q.y = OpsF29::select(q.y, OpsF29::neg(q.y), d < 0);
      res = add(res, q);
    }
    {
      const int d = glv_digit(b2, i), m = d < 0 ? -d : d;
      G1W q = tab.get(m);
      q.x = OpsF29::mul(q.x, beta);
      q.y = OpsF29::select(q.y, OpsF29::neg(q.y), (d < 0) != flip2);
      res = add(res, q);
    }
  }
  return res;
}

// ------------------------------------------------------------------ the fold: one opening per lane, ONE accumulator ----------
// F = z pi - y G1gen + C:  the GLV walk of z pi (above) leaves the accumulator projective; y G1gen is the 32 signed byte digits of y mod r
// against the per-device fixed-base table of k_g1_generator_mul (g1.hip: T[w][j] = j 256^w G, affine), each entry SUBTRACTED -- 32 complete
// additions, no doublings; C joins last; one normalisation.  Against the four-call composition: no intermediate normalisation (two
// inversions fewer), no affine round trips through memory, three launches fewer.  Every addition is the complete formula, so C = +-z pi,
// C = y G1gen, pi = +-G1gen, scalars = 0 mod r and identity inputs need no case of their own.
// The launch is a fixed grid walked with a grid stride: a lane's window table lives in ITS KB of `tables` (lanes * 1 KB in all, however
// large n is) and is rebuilt per opening.  nxy != NULL: -pi_i (affine, reduced like Fp::new) and its flag go there too, for the verifier.
constexpr int COMB_WIN = 32, COMB_ENT = 128;             // the geometry of g1.hip's table (host::g1_gen_comb)
__global__ void HEAVY_BOUNDS k_kzg_fold(const u64* cxy, const uint8_t* cinf, const u64* zs, const u64* ys, const u64* pxy, const uint8_t* pinf,
                                        const i32* __restrict__ comb, uint8_t* tables, u64* oxy, uint8_t* oinf, u64* nxy, uint8_t* ninf, size_t n) {
  const size_t lanes = (size_t)gridDim.x * blockDim.x;
  G1TableGlobal tab{(G1TableGlobal::gptr)(tables + TID * G1_TABLE_BYTES_PER_LANE)};
#pragma unroll 1
  for (size_t i = TID; i < n; i += lanes) {
    u32 k[8];
    load_scalar_mod_r(k, zs, n, i);
    G1W res = glv_walk(load_g1w_flagged(pxy, pinf, n, i), k, tab);
    load_scalar_mod_r(k, ys, n, i);
    int carry = 0;
#pragma unroll 1
    for (int w = 0; w < COMB_WIN; ++w) {
      u32 byte = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) if (q == (w >> 2)) byte = (k[q] >> (8 * (w & 3))) & 255u;
      int d = (int)byte + carry;
      carry = d >= 128;
      d -= carry << 8;                                  // d in [-128, 127]; y mod r < 2^254 leaves no carry out of the last window
      const int mag = d < 0 ? -d : d;
      const i32* src = comb + ((size_t)w * COMB_ENT + (size_t)(mag ? mag - 1 : 0)) * 18;
      F29 ex, ey;
#pragma unroll
      for (int q = 0; q < 9; ++q) { ex.v[q] = src[q]; ey.v[q] = src[9 + q]; }
      const bool nz = mag != 0;
      G1W q1;                                           // digit 0 adds the identity (0 : 1 : 0); a positive digit adds MINUS its entry
      q1.x = OpsF29::select(OpsF29::zero(), ex, nz);
      q1.y = OpsF29::select(OpsF29::one(), OpsF29::select(OpsF29::neg(ey), ey, d < 0), nz);
      q1.z = OpsF29::select(OpsF29::zero(), OpsF29::one(), nz);
      res = proj_add_lazy<OpsF29>(res, q1);
    }
    res = proj_add_lazy<OpsF29>(res, load_g1w_flagged(cxy, cinf, n, i));
    Fp x, y; bool rinf;
    g1_to_affine(x, y, rinf, G1P{f29_to_fp(res.x), f29_to_fp(res.y), f29_to_fp(res.z)});      // spelt out: see g1w_to_affine (common.hpp)
    store_fp(oxy, n, i, 0, x); store_fp(oxy, n, i, 4, y);
    oinf[i] = rinf ? 1 : 0;
    if (nxy) {
      store_fp(nxy, n, i, 0, load_fp(pxy, n, i, 0));
      store_fp(nxy, n, i, 4, fp_neg(load_fp(pxy, n, i, 4)));
      ninf[i] = (pinf && pinf[i]) ? 1 : 0;
    }
  }
}

// ------------------------------------------------------------------ the weighted test's scalar side ----------
// Per opening: r_i mod r -> wr [4][n] and column i of sc [4][2n]; r_i z_i mod r -> column n + i of sc; C_i and pi_i (words and flags as given)
// -> columns i and n + i of bases [8][2n] / binf [2n] -- the 2n terms of ONE multi-scalar multiplication; and r_i y_i mod r into the block's
// partial sum, partial [4][gridDim.x].  Launched with exactly ceil(n / BLOCK) blocks.
__global__ void __launch_bounds__(BLOCK) k_kzg_weighted_prep(const u64* cxy, const uint8_t* cinf, const u64* pxy, const uint8_t* pinf, const u64* zs, const u64* ys,
                                                             const u64* weights, size_t n, u64* wr, u64* sc, u64* bases, uint8_t* binf, u64* partial) {
  __shared__ u32 part[BLOCK][8];
  const size_t i = TID, m = 2 * n;
  Fp acc = fp_from_limbs(0, 0, 0, 0, 0, 0, 0, 0);
  if (i < n) {
    const Fp r = fr_reduce_plain(load_plain(weights, n, i, 0));
    const Fp rz = fr_mul(r, fr_reduce_plain(load_plain(zs, n, i, 0)));
    acc = fr_mul(r, fr_reduce_plain(load_plain(ys, n, i, 0)));
    store_plain(wr, n, i, 0, r);
    store_plain(sc, m, i, 0, r);
    store_plain(sc, m, n + i, 0, rz);
#pragma unroll
    for (int w = 0; w < 8; ++w) { bases[(size_t)w * m + i] = cxy[(size_t)w * n + i]; bases[(size_t)w * m + n + i] = pxy[(size_t)w * n + i]; }
    binf[i] = (cinf && cinf[i]) ? 1 : 0;
    binf[n + i] = (pinf && pinf[i]) ? 1 : 0;
  }
  const Fp s = block_sum(acc, part);
  if (threadIdx.x == 0) store_plain(partial, gridDim.x, blockIdx.x, 0, s);
}
// one block: s = sum of the partials = sum_i r_i y_i mod r, out [4][1]
__global__ void __launch_bounds__(BLOCK) k_kzg_fr_join(const u64* partial, size_t parts, u64* out) {
  __shared__ u32 part[BLOCK][8];
  const Fp s = column_sum(partial, 1, parts, 0, part);
  if (threadIdx.x == 0) store_plain(out, 1, 0, 0, s);
}
// The two literal pairs as one SoA pair list of stride 2: lane 0 writes (m1 - s G1gen, G2gen), lane 1 writes (-m2, tau_g2), with
// m1 = sum r_i C_i + sum r_i z_i pi_i, m2 = sum r_i pi_i, sg = s G1gen (one affine point + flag each).
__global__ void __launch_bounds__(64) k_kzg_weighted_pairs(const u64* m1, const uint8_t* m1inf, const u64* m2, const uint8_t* m2inf, const u64* sg, const uint8_t* sginf,
                                                           const u64* tau, u64* pxy, uint8_t* pinf, u64* qxy, uint8_t* qinf) {
  const size_t i = TID;
  if (i >= 2) return;
  G1W p = load_g1w_flagged(i == 0 ? m1 : m2, i == 0 ? m1inf : m2inf, 1, 0);
  if (i == 0) {
    G1W g = load_g1w_flagged(sg, sginf, 1, 0);
    g.y = OpsF29::neg(g.y);
    p = proj_add_lazy<OpsF29>(p, g);
  }
  Fp x, y; bool inf;
  g1w_to_affine(x, y, inf, p);
  if (i == 0) store_closing_pair(0, x, y, inf, tau, pxy, pinf, qxy, qinf);
  else store_closing_pair(1, x, y, inf, tau, pxy, pinf, qxy, qinf);
}
}  // namespace kzg

namespace kzgh {
// F_i into out_xy / out_inf and, when neg_xy is given, -pi_i into neg_xy / neg_inf: one launch.  The grid is capped at two blocks per
// compute unit of window tables (BLOCK KB each); larger batches walk it with a grid stride.
int32_t fold(const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z, const uint64_t* y, const uint64_t* pi_xy, const uint8_t* pi_inf,
             uint64_t* out_xy, uint8_t* out_inf, uint64_t* neg_xy, uint8_t* neg_inf, size_t n, void* stream) {
  const bn254::i32* comb = nullptr;
  int32_t rc = host::g1_gen_comb(&comb, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  const unsigned cu = host::compute_units();
  const size_t cap = 2 * (size_t)(cu ? cu : 256), want = (n + BLOCK - 1) / BLOCK, blocks = want < cap ? want : cap;
  host::Lease ws;
  if ((rc = ws.acquire(blocks * BLOCK * G1_TABLE_BYTES_PER_LANE, (hipStream_t)stream)) != SYLOW_HIP_OK) return rc;
  kzg::k_kzg_fold<<<dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream>>>(c_xy, c_inf, z, y, pi_xy, pi_inf, comb, (uint8_t*)ws.p, out_xy, out_inf,
                                                                                neg_xy, neg_inf, n);
  return host::finish(SYLOW_HIP_OK, ws);
}
}  // namespace kzgh

extern "C" {
int32_t sylow_hip_kzg_fold_batch(const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z, const uint64_t* y, const uint64_t* pi_xy, const uint8_t* pi_inf,
                                 uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream) {
  ARGCHK(out_xy && out_inf && (n == 0 || (c_xy && z && y && pi_xy))); if (!n) return SYLOW_HIP_OK;
  return kzgh::fold(c_xy, c_inf, z, y, pi_xy, pi_inf, out_xy, out_inf, nullptr, nullptr, n, stream);
}

int32_t sylow_hip_kzg_batch_verify_weighted(const uint64_t* tau_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z, const uint64_t* y,
                                            const uint64_t* pi_xy, const uint8_t* pi_inf, const uint64_t* weights, size_t n,
                                            uint64_t* gt_out, uint8_t* is_one, void* stream) {
  ARGCHK((gt_out || is_one) && (n == 0 || (tau_g2_xy && c_xy && z && y && pi_xy && weights)));
  if (!n) return sylow_hip_pairing_product_batch(nullptr, nullptr, nullptr, nullptr, 0, 1, gt_out, is_one, stream);
  using namespace weighted_plan;
  const KzgWeightedLayout l = kzg_weighted_layout(n);
  ARGCHK(l.bytes != SAT);
  hipStream_t st = (hipStream_t)stream;
  const size_t parts = kzg_parts(n);
  host::Lease ws;
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *wr = ws.at<u64>(l.wr), *sc = ws.at<u64>(l.sc), *bases = ws.at<u64>(l.bases), *partial = ws.at<u64>(l.partial), *s = ws.at<u64>(l.s), *m1 = ws.at<u64>(l.m1),
      *m2 = ws.at<u64>(l.m2), *sg = ws.at<u64>(l.sg), *pxy = ws.at<u64>(l.pxy), *qxy = ws.at<u64>(l.qxy);
  uint8_t *binf = ws.at<uint8_t>(l.binf), *m1inf = ws.at<uint8_t>(l.m1inf), *m2inf = ws.at<uint8_t>(l.m2inf), *sginf = ws.at<uint8_t>(l.sginf),
          *pinf = ws.at<uint8_t>(l.pinf), *qinf = ws.at<uint8_t>(l.qinf);
  kzg::k_kzg_weighted_prep<<<dim3((unsigned)parts), dim3(BLOCK), 0, st>>>(c_xy, c_inf, pi_xy, pi_inf, z, y, weights, n, wr, sc, bases, binf, partial);
  kzg::k_kzg_fr_join<<<1, BLOCK, 0, st>>>(partial, parts, s);
  rc = sylow_hip_g1_msm(bases, binf, sc, 2 * n, m1, m1inf, stream);                        // sum r_i C_i + sum (r_i z_i) pi_i
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_msm(pi_xy, pi_inf, wr, n, m2, m2inf, stream);   // sum r_i pi_i
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_generator_mul_batch(s, sg, sginf, 1, stream);   // (sum r_i y_i) G1gen
  if (rc == SYLOW_HIP_OK) {
    kzg::k_kzg_weighted_pairs<<<1, 64, 0, st>>>(m1, m1inf, m2, m2inf, sg, sginf, tau_g2_xy, pxy, pinf, qxy, qinf);
    rc = sylow_hip_pairing_product_batch(pxy, pinf, qxy, qinf, 2, /*skip_infinity=*/1, gt_out, is_one, stream);
  }
  return host::finish(rc, ws);
}
}  // extern "C"
