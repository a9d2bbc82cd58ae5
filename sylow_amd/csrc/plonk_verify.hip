// plonk_verify.hip -- the batched PLONK verifier (include/sylow_pverify.h):
//   sylow_pverify_scalars_batch          the T term scalars of C, the value y and the status of m proofs: the verifier's Fr side;
//   sylow_pverify_fold_batch             the KZG row (C, y, pi) of every proof: the scalars, ONE gather, sylow_hip_g1_lincomb_batch twice;
//   sylow_pverify_verify_batch           the fold, sylow_hip_kzg_verify_batch on the rows (C, 0, y, pi), and the veto of the status;
//   sylow_pverify_batch_verify_weighted  one boolean: the weighted scalars and column sums, then the library's MSM and pairing product.
// No pairing, group-law or MSM kernel lives here: the kernels below work over Fr and copy points.  Terms, slots, columns, chunks and scratch:
// plonk_verify_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_block.hpp"
#include "bn254_fr_roots.hpp"
#include "plonk_verify_plan.hpp"
#include "../../include/sylow_pverify.h"

namespace pv {
using namespace plonk_verify_plan;
static_assert(PV_BLOCK == BLOCK, "a lane per proof, a block of BLOCK lanes");
static_assert(SYLOW_HIP_PLONK_WIRES_MAX == plonk_open_plan::PO_WIRES_MAX, "the header's bound is the plan's");

// what every proof of a call brings: the arrays of the header, all of stride m (evals: (2 W + 1) m; pub: n_pub m)
struct In {
  const u64 *evals, *pub, *shifts, *beta, *gamma, *alpha, *zeta, *v, *u;
  size_t n_pub, m;
  int log_n, log_e, W;
};

// w_n: the 2^28-th root squared down, as the transform's table forms it
BN_DEV Fp root_of(int log_n) {
  Fp w = fp_from_limbs(BN_FR_ROOT28);
#pragma unroll 1
  for (int i = 0; i < ntt_plan::root_squarings(log_n); ++i) w = fr_mul(w, w);
  return w;
}

// den [4][n_pub mc], input-major: zeta_(s0 + i) - w_n^j at j mc + i, canonical.  A lane per element; i < mc and j < n_pub by the count.
__global__ void __launch_bounds__(BLOCK) k_pv_den(const u64* zeta, size_t m, size_t s0, size_t mc, int log_n, size_t n_pub, u64* den) {
  const size_t total = n_pub * mc;
  const Fp w = root_of(log_n);
#pragma unroll 1
  for (size_t idx = TID; idx < total; idx += (size_t)gridDim.x * BLOCK) {
    const size_t j = idx / mc, i = idx - j * mc;
    store_plain(den, total, idx, 0, fr_sub(elem(zeta, m, s0 + i), fr_pow(w, (u64)j)));
  }
}

// Proof s0 + i, i < mc, a lane each: its T scalars into k [4][T mc] at c mc + i, y into y [4][m] and the status byte, both at s0 + i.
// inv [4][n_pub mc]: the inverses of k_pv_den's values (inv(0) = 0), canonical.  Every plane load of a challenge, of pub and of inv and every
// store to k is an 8-byte word at consecutive proofs on consecutive lanes; the evaluations are instance-major, as the prover wrote them.
// Nothing of size W, E or n_pub lives in registers: the powers of v and of zeta^n and w_n^j are running products.
__global__ void __launch_bounds__(BLOCK) k_pv_scalars(In a, size_t s0, size_t mc, const u64* inv, u64* k, u64* y_out, uint8_t* status) {
  const int W = a.W;
  const size_t T = terms(a.log_e, W), kn = T * mc, ev_n = evals_count(W, a.m), E = elems(a.log_e);
  const Fp w = root_of(a.log_n);
#pragma unroll 1
  for (size_t i = TID; i < mc; i += (size_t)gridDim.x * BLOCK) {
    const size_t g = s0 + i, e0 = g * eval_slots(W);
    const Fp x = elem(a.zeta, a.m, g), b = elem(a.beta, a.m, g), gm = elem(a.gamma, a.m, g), al = elem(a.alpha, a.m, g);
    const Fp vv = elem(a.v, a.m, g), uu = elem(a.u, a.m, g);
    // zeta^n by log_n squarings; L1 without an inversion, as plonk_open.hip forms it: (zeta^n - 1) / (zeta - 1) is the product of
    // 1 + zeta^(2^i), inv(n) is log_n halvings of 1, and zeta = 1 is the one point where inv(0) = 0 shows
    Fp zn = x, geo = fr_one(), ninv = fr_one();
#pragma unroll 1
    for (int q = 0; q < a.log_n; ++q) {
      geo = fr_mul(geo, fr_add(fr_one(), zn));
      zn = fr_mul(zn, zn);
      fr_euclid::half_mod(ninv.v);
    }
    const Fp zh = fr_sub(zn, fr_one());
    const Fp l1 = fp_eq(x, fr_one()) ? fr_zero() : fr_mul(geo, ninv);
    // p = ZH inv(n) sum_j pub_j w_n^j inv(zeta - w_n^j)
    Fp p = fr_zero();
    {
      Fp wj = fr_one();
#pragma unroll 1
      for (size_t j = 0; j < a.n_pub; ++j) {
        p = fr_add(p, fr_mul(fr_mul(elem(a.pub, a.n_pub * a.m, j * a.m + g), wj), load_plain(inv, a.n_pub * mc, j * mc + i, 0)));
        wj = fr_mul(wj, w);
      }
      p = fr_mul(p, fr_mul(zh, ninv));
    }
    const Fp bx = fr_mul(b, x);
    Fp A = fr_one(), B = fr_one(), a01 = fr_one(), last = fr_zero(), y = fr_zero(), vp = vv, vq = fr_pow(vv, (u64)W + 1);
#pragma unroll 1
    for (int j = 0; j < W; ++j) {
      const Fp aj = elem(a.evals, ev_n, e0 + slot_wire(j)), ag = fr_add(aj, gm);
      A = fr_mul(A, fr_add(ag, fr_mul(bx, elem(a.shifts, (size_t)W, (size_t)j))));
      if (j < 2) a01 = j ? fr_mul(a01, aj) : aj;
      store_plain(k, kn, term_selector(j) * mc + i, 0, aj);
      store_plain(k, kn, term_wire(W, j) * mc + i, 0, vp);
      y = fr_add(y, fr_mul(vp, aj));
      vp = fr_mul(vp, vv);
      if (j + 1 < W) {
        const Fp sj = elem(a.evals, ev_n, e0 + slot_sigma(W, j));
        B = fr_mul(B, fr_add(ag, fr_mul(b, sj)));
        store_plain(k, kn, term_sigma(W, j) * mc + i, 0, vq);
        y = fr_add(y, fr_mul(vq, sj));
        vq = fr_mul(vq, vv);
      } else {
        last = ag;
      }
    }
    const Fp zw = elem(a.evals, ev_n, e0 + slot_zw(W));
    const Fp al2l1 = fr_mul(fr_mul(al, al), l1), bp = fr_mul(fr_mul(al, B), zw);                 // B' = alpha B zw
    store_plain(k, kn, term_qm(W) * mc + i, 0, a01);
    store_plain(k, kn, term_qc(W) * mc + i, 0, fr_one());
    store_plain(k, kn, term_sigma(W, W - 1) * mc + i, 0, fr_neg(fr_mul(b, bp)));
    store_plain(k, kn, term_z(W) * mc + i, 0, fr_add(fr_add(fr_mul(al, A), al2l1), uu));
    Fp zp = fr_neg(zh);
#pragma unroll 1
    for (size_t e = 0; e < E; ++e) {
      store_plain(k, kn, term_chunk(W, e) * mc + i, 0, zp);
      zp = fr_mul(zp, zn);
    }
    store_plain(k, kn, term_wzeta(a.log_e, W) * mc + i, 0, x);
    store_plain(k, kn, term_womega(a.log_e, W) * mc + i, 0, fr_mul(uu, fr_mul(x, w)));
    y = fr_add(y, fr_mul(uu, zw));
    y = fr_sub(y, fr_sub(fr_sub(p, fr_mul(bp, last)), al2l1));
    store_plain(y_out, a.m, g, 0, y);
    status[g] = (uint8_t)(fp_is_zero(zh) ? STATUS_ZETA_IN_DOMAIN : 0);
  }
}

// The bases of a chunk, term-major: term c of proof s0 + i at c mc + i of bases [8][T mc] / binf [T mc] -- the key point c replicated for
// every proof, the proof's own point copied from slot c - (2 W + 2) -- words and flags as given; and the two terms of pi: W_zeta and W_omega
// at i and mc + i of pbases [8][2 mc] / pbinf [2 mc], their scalars 1 and u mod r at the same places of psc [4][2 mc].
__global__ void __launch_bounds__(BLOCK) k_pv_gather(const u64* vk_xy, const uint8_t* vk_inf, const u64* proof_xy, const uint8_t* proof_inf, const u64* u, size_t m,
                                                     size_t s0, size_t mc, int log_e, int W, u64* bases, uint8_t* binf, u64* pbases, uint8_t* pbinf, u64* psc) {
  const size_t K = key_points(W), P = proof_points(log_e, W), total = (K + P) * mc, pn = P * m;
#pragma unroll 1
  for (size_t idx = TID; idx < total; idx += (size_t)gridDim.x * BLOCK) {
    const size_t c = idx / mc, i = idx - c * mc;
    if (c < K) {
#pragma unroll
      for (int q = 0; q < 8; ++q) bases[(size_t)q * total + idx] = vk_xy[(size_t)q * K + c];
      binf[idx] = (vk_inf && vk_inf[c]) ? 1 : 0;
    } else {
      const size_t src = (c - K) * m + s0 + i;
#pragma unroll
      for (int q = 0; q < 8; ++q) bases[(size_t)q * total + idx] = proof_xy[(size_t)q * pn + src];
      binf[idx] = (proof_inf && proof_inf[src]) ? 1 : 0;
    }
  }
#pragma unroll 1
  for (size_t i = TID; i < mc; i += (size_t)gridDim.x * BLOCK) {
    const size_t z = pslot_wzeta(log_e, W) * m + s0 + i, o = pslot_womega(log_e, W) * m + s0 + i;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      pbases[(size_t)q * 2 * mc + i] = proof_xy[(size_t)q * pn + z];
      pbases[(size_t)q * 2 * mc + mc + i] = proof_xy[(size_t)q * pn + o];
    }
    pbinf[i] = (proof_inf && proof_inf[z]) ? 1 : 0;
    pbinf[mc + i] = (proof_inf && proof_inf[o]) ? 1 : 0;
    store_plain(psc, 2 * mc, i, 0, fr_one());
    store_plain(psc, 2 * mc, mc + i, 0, elem(u, m, s0 + i));
  }
}
// the rows of a chunk, [8][mc] + flags each, to columns s0 .. s0 + mc - 1 of the caller's [8][m] + flags
__global__ void __launch_bounds__(BLOCK) k_pv_scatter(const u64* p1, const uint8_t* f1, const u64* p2, const uint8_t* f2, size_t m, size_t s0, size_t mc, u64* o1,
                                                      uint8_t* of1, u64* o2, uint8_t* of2) {
#pragma unroll 1
  for (size_t s = TID; s < mc; s += (size_t)gridDim.x * BLOCK) {
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      o1[(size_t)w * m + s0 + s] = p1[(size_t)w * mc + s];
      o2[(size_t)w * m + s0 + s] = p2[(size_t)w * mc + s];
    }
    of1[s0 + s] = f1[s];
    of2[s0 + s] = f2[s];
  }
}
// ok_i = 0 where zeta_i lies in the domain
__global__ void __launch_bounds__(BLOCK) k_pv_veto(const uint8_t* status, size_t m, uint8_t* ok) {
#pragma unroll 1
  for (size_t i = TID; i < m; i += (size_t)gridDim.x * BLOCK)
    if (status[i] & STATUS_ZETA_IN_DOMAIN) ok[i] = 0;
}

// ------------------------------------------------------------------ the weighted form's scalar side ----------
// Per proof i, a lane each, launched with exactly ceil(m / BLOCK) blocks: rho_i = weights_i mod r; rho_i k_(c,i) for the proof's own terms
// into sc_own [4][(W + E + 3) m] at the place of the point in proof_xy; rho_i and rho_i u_i into sc_open [4][2 m] at i and m + i beside
// W_zeta and W_omega in obases [8][2 m] / obinf; and per column -- the 2 W + 2 key terms rho_i k_(c,i), then rho_i y_i, then 1 for a proof
// with rho_i != 0 whose zeta lies in the domain -- the block's partial sum into partial [4][columns parts] at column parts + block.
__global__ void __launch_bounds__(BLOCK) k_pv_weighted_prep(const u64* k, const u64* y, const uint8_t* status, const u64* weights, const u64* u, const u64* proof_xy,
                                                            const uint8_t* proof_inf, size_t m, int log_e, int W, u64* sc_own, u64* sc_open, u64* obases,
                                                            uint8_t* obinf, u64* partial) {
  __shared__ u32 part[BLOCK][8];
  const size_t i = TID, K = key_points(W), P = proof_points(log_e, W), kn = (K + P) * m, pn = P * m, parts = gridDim.x, cols = weighted_columns(W);
  const bool on = i < m;
  const Fp rho = on ? elem(weights, m, i) : fr_zero();
  if (on) {
#pragma unroll 1
    for (size_t c = 0; c < P; ++c) store_plain(sc_own, pn, c * m + i, 0, fr_mul(rho, load_plain(k, kn, (K + c) * m + i, 0)));
    const size_t z = pslot_wzeta(log_e, W) * m + i, o = pslot_womega(log_e, W) * m + i;
    store_plain(sc_open, 2 * m, i, 0, rho);
    store_plain(sc_open, 2 * m, m + i, 0, fr_mul(rho, elem(u, m, i)));
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      obases[(size_t)q * 2 * m + i] = proof_xy[(size_t)q * pn + z];
      obases[(size_t)q * 2 * m + m + i] = proof_xy[(size_t)q * pn + o];
    }
    obinf[i] = (proof_inf && proof_inf[z]) ? 1 : 0;
    obinf[m + i] = (proof_inf && proof_inf[o]) ? 1 : 0;
  }
#pragma unroll 1
  for (size_t c = 0; c < cols; ++c) {
    Fp acc = fr_zero();
    if (on) {
      if (c < K) acc = fr_mul(rho, load_plain(k, kn, c * m + i, 0));
      else if (c == column_s(W)) acc = fr_mul(rho, load_plain(y, m, i, 0));
      else acc = ((status[i] & STATUS_ZETA_IN_DOMAIN) && !fp_is_zero(rho)) ? fr_one() : fr_zero();
    }
    const Fp s = block_sum(acc, part);
    if (threadIdx.x == 0) store_plain(partial, cols * parts, c * parts + blockIdx.x, 0, s);
  }
}
// a block per column: the sum of its partials -- a key column into ksum [4][2 W + 2], s into s_out [4][1], the count into bad [4][1]
__global__ void __launch_bounds__(BLOCK) k_pv_join(const u64* partial, size_t parts, int W, u64* ksum, u64* s_out, u64* bad) {
  __shared__ u32 part[BLOCK][8];
  const size_t c = blockIdx.x, K = key_points(W);
  const Fp s = column_sum(partial, weighted_columns(W), parts, c, part);
  if (threadIdx.x == 0) {
    if (c < K) store_plain(ksum, K, c, 0, s);
    else store_plain(c == column_s(W) ? s_out : bad, 1, 0, 0, s);
  }
}
// The two literal pairs as one SoA pair list of stride 2: lane 0 copies (m1 - s G1gen, G2gen), lane 1 writes (-m2, tau_g2): the same x, the
// negated y (reduced like Fp::new), the same flag
__global__ void __launch_bounds__(64) k_pv_pairs(const u64* m1s, const uint8_t* m1sinf, const u64* m2, const uint8_t* m2inf, const u64* tau, u64* pxy, uint8_t* pinf,
                                                 u64* qxy, uint8_t* qinf) {
  const size_t i = TID;
  if (i >= 2) return;
  if (i == 0) store_closing_pair(0, load_fp(m1s, 1, 0, 0), load_fp(m1s, 1, 0, 4), m1sinf[0] != 0, tau, pxy, pinf, qxy, qinf);
  else store_closing_pair(1, load_fp(m2, 1, 0, 0), load_fp(m2, 1, 0, 4), m2inf[0] != 0, tau, pxy, pinf, qxy, qinf);
}
// is_one = 0 when a live proof's zeta lay in the domain
__global__ void __launch_bounds__(64) k_pv_veto_one(const u64* bad, uint8_t* is_one) {
  if (TID == 0 && !fp_is_zero(load_plain(bad, 1, 0, 0))) is_one[0] = 0;
}

static unsigned lane_grid(size_t lanes, long long max_blocks) { return (unsigned)grid(lane_tiles(lanes), max_blocks); }

// the arrays of a call beyond In, for the aliasing table and the gather
struct Points {
  const u64 *tau, *vk_xy, *proof_xy, *weights;
  const uint8_t *vk_inf, *proof_inf;
};
// the checks every entry point shares, in the header's order: the dimensions, then (m > 0) the required arrays and the sizes
static int32_t check_dims(const In& a, long long max_blocks) {
  ARGCHK(dims_ok(a.log_n, a.log_e, a.W) && pub_ok(a.log_n, a.n_pub) && max_blocks_ok(max_blocks));
  return SYLOW_HIP_OK;
}
static int32_t check_arrays(const In& a, const Points* p) {
  ARGCHK(a.evals && a.shifts && a.beta && a.gamma && a.alpha && a.zeta && a.v && a.u && (a.pub || !a.n_pub));
  ARGCHK(!p || (p->vk_xy && p->proof_xy));
  ARGCHK(evals_bytes(a.W, a.m) != SAT && scalars_bytes(pub_count(a.n_pub, a.m)) != SAT && scalars_bytes(term_count(a.log_e, a.W, a.m)) != SAT &&
         proof_bytes(a.log_e, a.W, a.m) != SAT);
  return SYLOW_HIP_OK;
}
// every output against every input and the outputs after it; a NULL array takes no part
template <size_t NO> static bool apart(const In& a, const Points* p, const host::Range (&outs)[NO]) {
  const size_t one = scalars_bytes(a.m);
  const host::Range in[15] = {{(uintptr_t)a.evals, evals_bytes(a.W, a.m)}, {(uintptr_t)(a.n_pub ? a.pub : nullptr), scalars_bytes(pub_count(a.n_pub, a.m))},
                              {(uintptr_t)a.shifts, scalars_bytes((size_t)a.W)}, {(uintptr_t)a.beta, one}, {(uintptr_t)a.gamma, one}, {(uintptr_t)a.alpha, one},
                              {(uintptr_t)a.zeta, one}, {(uintptr_t)a.v, one}, {(uintptr_t)a.u, one},
                              {(uintptr_t)(p ? p->tau : nullptr), tau_bytes()}, {(uintptr_t)(p ? p->vk_xy : nullptr), key_bytes(a.W)},
                              {(uintptr_t)(p ? p->vk_inf : nullptr), key_points(a.W)}, {(uintptr_t)(p ? p->proof_xy : nullptr), proof_bytes(a.log_e, a.W, a.m)},
                              {(uintptr_t)(p ? p->proof_inf : nullptr), proof_count(a.log_e, a.W, a.m)}, {(uintptr_t)(p ? p->weights : nullptr), one}};
  return host::outputs_disjoint(in, outs, disjoint);
}

// proofs s0 .. s0 + c - 1: the denominators and their inverses in den [2][4][n_pub c], then the scalars into k [4][T c], y and status at s0 + i
static int32_t scalars_run(const In& a, size_t s0, size_t c, long long max_blocks, u64* den, u64* k, u64* y, uint8_t* status, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t dn = a.n_pub * c;
  if (dn) {
    k_pv_den<<<dim3(lane_grid(dn, max_blocks)), dim3(BLOCK), 0, st>>>(a.zeta, a.m, s0, c, a.log_n, a.n_pub, den);
    const int32_t rc = sylow_hip_fr_batch_inv(den, den + FR_WORDS * dn, dn, stream);
    if (rc != SYLOW_HIP_OK) return rc;
  }
  k_pv_scalars<<<dim3(lane_grid(c, max_blocks)), dim3(BLOCK), 0, st>>>(a, s0, c, den + FR_WORDS * dn, k, y, status);
  return SYLOW_HIP_OK;
}

// The rows of all m proofs into c_xy, pi_xy [8][m] + flags, y [4][m], status [m], chunk by chunk through one lease laid out for mc proofs
// (fold_layout)
static int32_t fold_run(const In& a, const Points& p, u64* c_xy, uint8_t* c_inf, u64* pi_xy, uint8_t* pi_inf, u64* y, uint8_t* status, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t lim = host::scratch_limit(), mc = proofs_per_chunk(a.log_e, a.W, a.n_pub, a.m, lim ? lim : msmh::default_budget());
  if (!mc) {
    snprintf(sylow_g_err, sizeof(sylow_g_err), "plonk_verify: the scratch limit does not hold one proof (%zu bytes)", fold_chunk_bytes(a.log_e, a.W, a.n_pub, 1));
    return SYLOW_HIP_E_HIP;
  }
  host::Lease ws;
  const FoldLayout l = fold_layout(a.log_e, a.W, a.n_pub, mc);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  const size_t T = terms(a.log_e, a.W);
  u64 *den = ws.at<u64>(l.den), *k = ws.at<u64>(l.k), *bases = ws.at<u64>(l.bases), *pbases = ws.at<u64>(l.pbases), *psc = ws.at<u64>(l.psc), *C = ws.at<u64>(l.C),
      *PI = ws.at<u64>(l.PI);
  uint8_t *binf = ws.at<uint8_t>(l.binf), *pbinf = ws.at<uint8_t>(l.pbinf), *cinf = ws.at<uint8_t>(l.cinf), *pinf = ws.at<uint8_t>(l.pinf);
  for (size_t s0 = 0; s0 < a.m && rc == SYLOW_HIP_OK; s0 += mc) {
    const size_t c = chunk_size(a.m, mc, s0);
    rc = scalars_run(a, s0, c, -1, den, k, y, status, stream);
    if (rc != SYLOW_HIP_OK) break;
    k_pv_gather<<<dim3(lane_grid(T * c, -1)), dim3(BLOCK), 0, st>>>(p.vk_xy, p.vk_inf, p.proof_xy, p.proof_inf, a.u, a.m, s0, c, a.log_e, a.W, bases, binf, pbases,
                                                                     pbinf, psc);
    rc = sylow_hip_g1_lincomb_batch(bases, binf, k, C, cinf, c, T, stream);
    if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_lincomb_batch(pbases, pbinf, psc, PI, pinf, c, PI_TERMS, stream);
    if (rc != SYLOW_HIP_OK) break;
    k_pv_scatter<<<dim3(lane_grid(c, -1)), dim3(BLOCK), 0, st>>>(C, cinf, PI, pinf, a.m, s0, c, c_xy, c_inf, pi_xy, pi_inf);
  }
  return host::finish(rc, ws);
}
}  // namespace pv

extern "C" {
int32_t sylow_pverify_scalars_batch_tuned(const uint64_t* evals, const uint64_t* pub, size_t n_pub, const uint64_t* shifts, const uint64_t* beta,
                                          const uint64_t* gamma, const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, const uint64_t* u,
                                          int32_t log_n, int32_t log_e, int32_t W, size_t m, int64_t max_blocks, uint64_t* k_out, uint64_t* y_out,
                                          uint8_t* status, void* stream) {
  using namespace plonk_verify_plan;
  const pv::In a = {evals, pub, shifts, beta, gamma, alpha, zeta, v, u, n_pub, m, log_n, log_e, W};
  int32_t rc = pv::check_dims(a, max_blocks);
  if (rc != SYLOW_HIP_OK || !m) return rc;
  ARGCHK(k_out && y_out && status);
  if ((rc = pv::check_arrays(a, nullptr)) != SYLOW_HIP_OK) return rc;
  const size_t scratch = scalars_scratch_words(n_pub, m);
  ARGCHK(scratch_ok(scratch));
  const host::Range outs[3] = {{(uintptr_t)k_out, scalars_bytes(term_count(log_e, W, m))}, {(uintptr_t)y_out, scalars_bytes(m)}, {(uintptr_t)status, m}};
  ARGCHK(pv::apart(a, nullptr, outs));
  host::Lease ws;
  if (scratch && (rc = ws.acquire(scalars_scratch_bytes(n_pub, m), (hipStream_t)stream)) != SYLOW_HIP_OK) return rc;
  rc = pv::scalars_run(a, 0, m, max_blocks, ws.at<u64>(0), k_out, y_out, status, stream);
  return host::finish(rc, ws);
}
int32_t sylow_pverify_scalars_batch(const uint64_t* evals, const uint64_t* pub, size_t n_pub, const uint64_t* shifts, const uint64_t* beta,
                                    const uint64_t* gamma, const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, const uint64_t* u,
                                    int32_t log_n, int32_t log_e, int32_t W, size_t m, uint64_t* k_out, uint64_t* y_out, uint8_t* status, void* stream) {
  return sylow_pverify_scalars_batch_tuned(evals, pub, n_pub, shifts, beta, gamma, alpha, zeta, v, u, log_n, log_e, W, m, -1, k_out, y_out, status, stream);
}

int32_t sylow_pverify_fold_batch(const uint64_t* vk_xy, const uint8_t* vk_inf, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* evals,
                                 const uint64_t* pub, size_t n_pub, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma,
                                 const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, const uint64_t* u, int32_t log_n, int32_t log_e,
                                 int32_t W, size_t m, uint64_t* c_xy, uint8_t* c_inf, uint64_t* pi_xy, uint8_t* pi_inf, uint64_t* y_out, uint8_t* status,
                                 void* stream) {
  using namespace plonk_verify_plan;
  const pv::In a = {evals, pub, shifts, beta, gamma, alpha, zeta, v, u, n_pub, m, log_n, log_e, W};
  const pv::Points p = {nullptr, vk_xy, proof_xy, nullptr, vk_inf, proof_inf};
  int32_t rc = pv::check_dims(a, -1);
  if (rc != SYLOW_HIP_OK || !m) return rc;
  ARGCHK(c_xy && c_inf && pi_xy && pi_inf && y_out && status);
  if ((rc = pv::check_arrays(a, &p)) != SYLOW_HIP_OK) return rc;
  ARGCHK(fold_chunk_bytes(log_e, W, n_pub, 1) != SAT);
  const host::Range outs[6] = {{(uintptr_t)c_xy, points_bytes(m)}, {(uintptr_t)c_inf, m}, {(uintptr_t)pi_xy, points_bytes(m)}, {(uintptr_t)pi_inf, m},
                               {(uintptr_t)y_out, scalars_bytes(m)}, {(uintptr_t)status, m}};
  ARGCHK(pv::apart(a, &p, outs));
  return pv::fold_run(a, p, c_xy, c_inf, pi_xy, pi_inf, y_out, status, stream);
}

int32_t sylow_pverify_verify_batch(const uint64_t* tau_g2_xy, const uint64_t* vk_xy, const uint8_t* vk_inf, const uint64_t* proof_xy, const uint8_t* proof_inf,
                                   const uint64_t* evals, const uint64_t* pub, size_t n_pub, const uint64_t* shifts, const uint64_t* beta,
                                   const uint64_t* gamma, const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, const uint64_t* u, int32_t log_n,
                                   int32_t log_e, int32_t W, size_t m, uint8_t* ok, uint8_t* status, void* stream) {
  using namespace plonk_verify_plan;
  const pv::In a = {evals, pub, shifts, beta, gamma, alpha, zeta, v, u, n_pub, m, log_n, log_e, W};
  const pv::Points p = {tau_g2_xy, vk_xy, proof_xy, nullptr, vk_inf, proof_inf};
  int32_t rc = pv::check_dims(a, -1);
  if (rc != SYLOW_HIP_OK || !m) return rc;
  ARGCHK(tau_g2_xy && ok && status);
  if ((rc = pv::check_arrays(a, &p)) != SYLOW_HIP_OK) return rc;
  ARGCHK(fold_chunk_bytes(log_e, W, n_pub, 1) != SAT && scratch_ok(verify_words(m)));
  const host::Range outs[2] = {{(uintptr_t)ok, m}, {(uintptr_t)status, m}};
  ARGCHK(pv::apart(a, &p, outs));
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  const VerifyLayout l = verify_layout(m);
  if ((rc = ws.acquire(l.bytes, st)) != SYLOW_HIP_OK) return rc;
  u64 *C = ws.at<u64>(l.C), *PI = ws.at<u64>(l.PI), *y = ws.at<u64>(l.y), *z = ws.at<u64>(l.z);
  uint8_t *cinf = ws.at<uint8_t>(l.cinf), *pinf = ws.at<uint8_t>(l.pinf);
  rc = pv::fold_run(a, p, C, cinf, PI, pinf, y, status, stream);
  if (rc == SYLOW_HIP_OK && hipMemsetAsync(z, 0, FR_WORDS * m * sizeof(u64), st) != hipSuccess) rc = host::fail(hipGetLastError(), "hipMemsetAsync");
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_kzg_verify_batch(tau_g2_xy, C, cinf, z, y, PI, pinf, ok, m, stream);
  if (rc == SYLOW_HIP_OK) pv::k_pv_veto<<<dim3(pv::lane_grid(m, -1)), dim3(BLOCK), 0, st>>>(status, m, ok);
  return host::finish(rc, ws);
}

int32_t sylow_pverify_batch_verify_weighted(const uint64_t* tau_g2_xy, const uint64_t* vk_xy, const uint8_t* vk_inf, const uint64_t* proof_xy,
                                            const uint8_t* proof_inf, const uint64_t* evals, const uint64_t* pub, size_t n_pub, const uint64_t* shifts,
                                            const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v,
                                            const uint64_t* u, const uint64_t* weights, int32_t log_n, int32_t log_e, int32_t W, size_t m,
                                            uint64_t* gt_out, uint8_t* is_one, uint8_t* status, void* stream) {
  using namespace plonk_verify_plan;
  const pv::In a = {evals, pub, shifts, beta, gamma, alpha, zeta, v, u, n_pub, m, log_n, log_e, W};
  const pv::Points p = {tau_g2_xy, vk_xy, proof_xy, weights, vk_inf, proof_inf};
  int32_t rc = pv::check_dims(a, -1);
  if (rc != SYLOW_HIP_OK) return rc;
  ARGCHK(gt_out || is_one);
  if (!m) return sylow_hip_pairing_product_batch(nullptr, nullptr, nullptr, nullptr, 0, 1, gt_out, is_one, stream);
  ARGCHK(tau_g2_xy && weights && status);
  if ((rc = pv::check_arrays(a, &p)) != SYLOW_HIP_OK) return rc;
  const size_t scratch = weighted_words(log_e, W, n_pub, m);
  ARGCHK(scratch_ok(scratch));
  const host::Range outs[3] = {{(uintptr_t)gt_out, gt_bytes()}, {(uintptr_t)is_one, 1}, {(uintptr_t)status, m}};
  ARGCHK(pv::apart(a, &p, outs));
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  const WeightedLayout l = weighted_layout(log_e, W, n_pub, m);
  if ((rc = ws.acquire(l.bytes, st)) != SYLOW_HIP_OK) return rc;
  const size_t K = key_points(W), P = proof_points(log_e, W), parts = weighted_parts(m), cols = weighted_columns(W);
  const auto U = [&](size_t off) { return ws.at<u64>(off); };
  const auto B = [&](size_t off) { return ws.at<uint8_t>(off); };
  u64 *den = U(l.den), *k = U(l.k), *y = U(l.y), *sc_own = U(l.sc_own), *sc_open = U(l.sc_open), *obases = U(l.obases), *partial = U(l.partial), *ksum = U(l.ksum),
      *s = U(l.s), *bad = U(l.bad), *m_own = U(l.m_own), *m2 = U(l.m2), *m_key = U(l.m_key), *m1 = U(l.m1), *sg = U(l.sg), *pxy = U(l.pxy), *qxy = U(l.qxy);
  uint8_t *obinf = B(l.obinf), *f_own = B(l.f_own), *f2 = B(l.f2), *f_key = B(l.f_key), *f1 = B(l.f1), *fsg = B(l.fsg), *pinf = B(l.pinf), *qinf = B(l.qinf);
  rc = pv::scalars_run(a, 0, m, -1, den, k, y, status, stream);
  if (rc == SYLOW_HIP_OK) {
    pv::k_pv_weighted_prep<<<dim3((unsigned)parts), dim3(BLOCK), 0, st>>>(k, y, status, weights, u, proof_xy, proof_inf, m, log_e, W, sc_own, sc_open, obases, obinf,
                                                                          partial);
    pv::k_pv_join<<<dim3((unsigned)cols), dim3(BLOCK), 0, st>>>(partial, parts, W, ksum, s, bad);
    rc = sylow_hip_g1_msm(proof_xy, proof_inf, sc_own, P * m, m_own, f_own, stream);                    // sum_i sum_{c own} (rho_i k_(c,i)) P_(c,i)
  }
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_msm(obases, obinf, sc_open, PI_TERMS * m, m2, f2, stream);   // M2
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_lincomb_batch(vk_xy, vk_inf, ksum, m_key, f_key, 1, K, stream);   // sum_{c shared} (sum_i rho_i k_(c,i)) VK_c
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_add_batch(m_key, f_key, m_own, f_own, m1, f1, 1, stream);   // M1
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_generator_mul_batch(s, sg, fsg, 1, stream);                 // s G1gen
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_sub_batch(m1, f1, sg, fsg, m_own, f_own, 1, stream);        // M1 - s G1gen, over the own terms' sum
  if (rc == SYLOW_HIP_OK) {
    pv::k_pv_pairs<<<1, 64, 0, st>>>(m_own, f_own, m2, f2, tau_g2_xy, pxy, pinf, qxy, qinf);
    rc = sylow_hip_pairing_product_batch(pxy, pinf, qxy, qinf, 2, /*skip_infinity=*/1, gt_out, is_one, stream);
  }
  if (rc == SYLOW_HIP_OK && is_one) pv::k_pv_veto_one<<<1, 64, 0, st>>>(bad, is_one);
  return host::finish(rc, ws);
}
}  // extern "C"
