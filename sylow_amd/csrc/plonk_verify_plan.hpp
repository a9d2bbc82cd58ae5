// plonk_verify_plan.hpp -- the geometry of the batched PLONK verifier (plonk_verify.hip): the terms of a proof's linear combination C and
// their order, the slots of the key and of a proof, the columns of the weighted form's reduction, the chunks of whole proofs under a scratch
// limit and every byte count and scratch offset, plain C++ so that tests/cpp/plonk_verify_plan_test.cpp can compile it with g++ on a box without a GPU.  The
// launch code asks these functions and decides nothing itself.  The evaluation slots, the bounds on log_n, log_e and W and the status bit are
// plonk_open_plan.hpp's: the verifier reads what the prover wrote.
#pragma once
#include "plonk_open_plan.hpp"

namespace plonk_verify_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::disjoint;
using plan_base::elems;
using plan_base::max_blocks_ok;
using plan_base::mul_sat;
using plan_base::words_of;
using plonk_open_plan::FR_WORDS;
using plonk_open_plan::STATUS_ZETA_IN_DOMAIN;
using plonk_open_plan::ceil_div;
using plonk_open_plan::chunk_count;
using plonk_open_plan::chunk_size;
using plonk_open_plan::dims_ok;
using plonk_open_plan::eval_slots;
using plonk_open_plan::evals_bytes;
using plonk_open_plan::evals_count;
using plonk_open_plan::grid;
using plonk_open_plan::lane_tiles;
using plonk_open_plan::scalars_bytes;
using plonk_open_plan::slot_sigma;
using plonk_open_plan::slot_wire;
using plonk_open_plan::slot_zw;
constexpr int PV_BLOCK = plonk_open_plan::PO_BLOCK;      // == BLOCK of common.hpp (plonk_verify.hip asserts it): a lane per proof
constexpr size_t G1_WORDS = 8;                           // an affine G1 point, x then y
constexpr size_t G2_WORDS = 16;

constexpr bool pub_ok(int log_n, size_t n_pub) { return n_pub <= elems(log_n); }

// ---- the key: 2 W + 2 points in the row order of the prover's ctable; a proof: W + E + 3 points, slot-major in proof_xy [8][(W + E + 3) m] ----
constexpr size_t key_points(int wires) { return plonk_open_plan::ctable_rows(wires); }
constexpr size_t proof_points(int log_e, int wires) { return (size_t)wires + elems(log_e) + 3; }
constexpr size_t pslot_wire(int j) { return (size_t)j; }                                         // [w_j], j < W
constexpr size_t pslot_z(int wires) { return (size_t)wires; }                                    // [z]
constexpr size_t pslot_chunk(int wires, size_t e) { return (size_t)wires + 1 + e; }              // [t_e], e < E
constexpr size_t pslot_wzeta(int log_e, int wires) { return (size_t)wires + 1 + elems(log_e); }  // W_zeta
constexpr size_t pslot_womega(int log_e, int wires) { return (size_t)wires + 2 + elems(log_e); } // W_omega

// ---- the terms of C: T = 3 W + E + 5, the key points first, then the proof's own, each group in its own slot order ----------------------------
constexpr size_t terms(int log_e, int wires) { return key_points(wires) + proof_points(log_e, wires); }
constexpr size_t term_selector(int j) { return plonk_open_plan::row_selector(j); }               // a_j
constexpr size_t term_qm(int wires) { return plonk_open_plan::row_qm(wires); }                   // a_0 a_1
constexpr size_t term_qc(int wires) { return plonk_open_plan::row_qc(wires); }                   // 1
constexpr size_t term_sigma(int wires, int j) { return plonk_open_plan::row_sigma(wires, j); }   // v^(W+1+j), j < W - 1; -beta B' at j = W - 1
constexpr size_t term_own(int wires, size_t pslot) { return key_points(wires) + pslot; }         // the term of a proof's slot
constexpr size_t term_wire(int wires, int j) { return term_own(wires, pslot_wire(j)); }          // v^(1+j)
constexpr size_t term_z(int wires) { return term_own(wires, pslot_z(wires)); }                   // alpha A + alpha^2 L1 + u
constexpr size_t term_chunk(int wires, size_t e) { return term_own(wires, pslot_chunk(wires, e)); }          // -ZH zeta^(e n)
constexpr size_t term_wzeta(int log_e, int wires) { return term_own(wires, pslot_wzeta(log_e, wires)); }    // zeta
constexpr size_t term_womega(int log_e, int wires) { return term_own(wires, pslot_womega(log_e, wires)); }  // u zeta w_n
constexpr size_t PI_TERMS = 2;                                                                   // pi = 1 W_zeta + u W_omega

// ---- byte counts of the caller's arrays -------------------------------------------------------------------------------------------------------
constexpr size_t points_bytes(size_t count) { return mul_sat(mul_sat(count, G1_WORDS), sizeof(uint64_t)); }
constexpr size_t key_bytes(int wires) { return points_bytes(key_points(wires)); }
constexpr size_t proof_count(int log_e, int wires, size_t m) { return mul_sat(proof_points(log_e, wires), m); }
constexpr size_t proof_bytes(int log_e, int wires, size_t m) { return points_bytes(proof_count(log_e, wires, m)); }
constexpr size_t term_count(int log_e, int wires, size_t m) { return mul_sat(terms(log_e, wires), m); }
constexpr size_t pub_count(size_t n_pub, size_t m) { return mul_sat(n_pub, m); }
constexpr size_t tau_bytes() { return G2_WORDS * sizeof(uint64_t); }
constexpr size_t gt_bytes() { return 48 * sizeof(uint64_t); }

// ---- the scalars: the n_pub m denominators zeta_i - w_n^j [4][n_pub m], input-major, and their inverses beside them (one shared-inverse
// batch inversion reads the first and writes the second); then a lane per proof ----------------------------------------------------------------
constexpr size_t den_words(size_t n_pub, size_t mc) { return mul_sat(mul_sat(2 * FR_WORDS, n_pub), mc); }
constexpr size_t scalars_scratch_words(size_t n_pub, size_t mc) { return den_words(n_pub, mc); }
constexpr size_t scalars_scratch_bytes(size_t n_pub, size_t mc) { return mul_sat(scalars_scratch_words(n_pub, mc), sizeof(uint64_t)); }
constexpr bool scratch_ok(size_t words) { return plonk_open_plan::scratch_ok(words); }
constexpr size_t flag_words(size_t flags) { Carve c; c.bytes(flags); c.round(); return words_of(c.at); }      // the u64 words `flags` trailing bytes end in, as every layout below ends

// ---- the fold: a chunk of mc whole proofs leases the denominators, the scalars k [4][T mc], the gathered bases [8][T mc] and [8][2 mc], the
// scalars (1, u) [4][2 mc], C and pi [8][mc] each, and the flags of all of them.  sylow_hip_g1_lincomb_batch leases nothing ------------------------
struct FoldLayout { size_t den, k, bases, pbases, psc, C, PI, binf, pbinf, cinf, pinf, bytes; };
constexpr FoldLayout fold_layout(int log_e, int wires, size_t n_pub, size_t mc) {
  const size_t t = term_count(log_e, wires, mc);
  Carve c; FoldLayout l{};
  l.den = c.words(den_words(n_pub, mc));
  l.k = c.words(mul_sat(FR_WORDS, t));
  l.bases = c.words(mul_sat(G1_WORDS, t));
  l.pbases = c.words(mul_sat(G1_WORDS * PI_TERMS, mc));
  l.psc = c.words(mul_sat(FR_WORDS * PI_TERMS, mc));
  l.C = c.words(mul_sat(G1_WORDS, mc));
  l.PI = c.words(mul_sat(G1_WORDS, mc));
  l.binf = c.bytes(t);
  l.pbinf = c.bytes(mul_sat(PI_TERMS, mc));
  l.cinf = c.bytes(mc);
  l.pinf = c.bytes(mc);
  c.round();
  l.bytes = c.at; return l;
}
constexpr size_t fold_chunk_bytes(int log_e, int wires, size_t n_pub, size_t mc) { return fold_layout(log_e, wires, n_pub, mc).bytes; }
// its flag bytes, from the first flag to the end of the last array of them (pinf, mc bytes)
constexpr size_t fold_flags(int log_e, int wires, size_t mc) { return add_sat(fold_layout(log_e, wires, 0, mc).pinf, mc) - fold_layout(log_e, wires, 0, mc).binf; }
constexpr size_t fold_chunk_words(int log_e, int wires, size_t n_pub, size_t mc) { return words_of(fold_chunk_bytes(log_e, wires, n_pub, mc)); }
// whole proofs per chunk under `budget` bytes: 0 when not even one fits (the rule of plonk_open_plan::instances_per_chunk)
constexpr size_t proofs_per_chunk(int log_e, int wires, size_t n_pub, size_t m, size_t budget) {
  if (!m || fold_chunk_bytes(log_e, wires, n_pub, 1) > budget) return 0;
  size_t mc = budget / fold_chunk_bytes(log_e, wires, n_pub, 1);
  if (mc > m) mc = m;
  while (mc > 1 && fold_chunk_bytes(log_e, wires, n_pub, mc) > budget) --mc;
  while (mc < m && fold_chunk_bytes(log_e, wires, n_pub, mc + 1) <= budget) ++mc;
  return mc;
}

// ---- the per-proof flags: the fold's row (C, pi [8][m] each, y and the zeros of z [4][m] each, the two flag arrays) on top of the fold's chunk --
struct VerifyLayout { size_t C, PI, y, z, cinf, pinf, bytes; };
constexpr VerifyLayout verify_layout(size_t m) {
  Carve c; VerifyLayout l{};
  l.C = c.words(mul_sat(G1_WORDS, m));
  l.PI = c.words(mul_sat(G1_WORDS, m));
  l.y = c.words(mul_sat(FR_WORDS, m));
  l.z = c.words(mul_sat(FR_WORDS, m));
  l.cinf = c.bytes(m);
  l.pinf = c.bytes(m);
  c.round();
  l.bytes = c.at; return l;
}
constexpr size_t verify_words(size_t m) { return words_of(verify_layout(m).bytes); }

// ---- the weighted form: the scalars of all m proofs, rho k of the own terms [4][(W + E + 3) m] (the layout of proof_xy: the multi-scalar
// multiplication reads the proofs in place), rho and rho u [4][2 m] beside the gathered opening points [8][2 m], the columns of the two-level
// reduction -- the 2 W + 2 key terms, then s, then the count of live proofs whose zeta lies in the domain -- and five points, the pair list ------
constexpr size_t weighted_columns(int wires) { return key_points(wires) + 2; }
constexpr size_t column_s(int wires) { return key_points(wires); }
constexpr size_t column_bad(int wires) { return key_points(wires) + 1; }
constexpr size_t weighted_parts(size_t m) { return lane_tiles(m); }
constexpr size_t WEIGHTED_POINTS = 5;                    // the own terms' sum, the opening points' sum, the key terms' sum, M1, s G1gen
struct WeightedLayout {
  size_t den, k, y, sc_own, sc_open, obases, partial, ksum, s, bad, m_own, m2, m_key, m1, sg, pxy, qxy;      // u64 arrays
  size_t obinf, f_own, f2, f_key, f1, fsg, pinf, qinf, bytes;                                                // flags, and the total
};
constexpr WeightedLayout weighted_layout(int log_e, int wires, size_t n_pub, size_t m) {
  const size_t cols = weighted_columns(wires);
  Carve c; WeightedLayout l{};
  l.den = c.words(den_words(n_pub, m));
  l.k = c.words(mul_sat(FR_WORDS, term_count(log_e, wires, m)));
  l.y = c.words(mul_sat(FR_WORDS, m));
  l.sc_own = c.words(mul_sat(FR_WORDS, proof_count(log_e, wires, m)));
  l.sc_open = c.words(mul_sat(FR_WORDS * PI_TERMS, m));
  l.obases = c.words(mul_sat(G1_WORDS * PI_TERMS, m));
  l.partial = c.words(mul_sat(mul_sat(FR_WORDS, cols), weighted_parts(m)));
  l.ksum = c.words(FR_WORDS * key_points(wires));
  l.s = c.words(FR_WORDS);
  l.bad = c.words(FR_WORDS);
  l.m_own = c.words(G1_WORDS);
  l.m2 = c.words(G1_WORDS);
  l.m_key = c.words(G1_WORDS);
  l.m1 = c.words(G1_WORDS);
  l.sg = c.words(G1_WORDS);
  l.pxy = c.words(2 * G1_WORDS);
  l.qxy = c.words(2 * G2_WORDS);
  l.obinf = c.bytes(mul_sat(PI_TERMS, m));
  l.f_own = c.bytes(1);
  l.f2 = c.bytes(1);
  l.f_key = c.bytes(1);
  l.f1 = c.bytes(1);
  l.fsg = c.bytes(1);
  l.pinf = c.bytes(2);
  l.qinf = c.bytes(2);
  c.round();
  l.bytes = c.at; return l;
}
constexpr size_t weighted_words(int log_e, int wires, size_t n_pub, size_t m) { return words_of(weighted_layout(log_e, wires, n_pub, m).bytes); }
}  // namespace plonk_verify_plan
