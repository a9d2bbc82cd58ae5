// weighted_plan.hpp -- the geometry of the two weighted one-boolean checks that lease one block each: sylow_hip_kzg_batch_verify_weighted
// (kzg.hip) and sylow_hip_groth16_batch_verify_weighted (groth16.hip).  The parts of their Fr sums and the scratch with its offsets, plain
// C++ so that tests/cpp/weighted_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch code asks these functions and
// decides nothing itself.
#pragma once
#include "plan_base.hpp"

namespace weighted_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::mul_sat;
constexpr size_t WEIGHTED_BLOCK = 256;                // == BLOCK of common.hpp (kzg.hip and groth16.hip assert it)
constexpr size_t FR_WORDS = 4, G1_WORDS = 8, G2_WORDS = 16;
constexpr size_t ceil_div(size_t a, size_t b) { return a / b + (a % b ? 1 : 0); }          // no sum that could wrap

// ---- KZG: sum_i r_i y_i in two levels.  The preparation kernel runs a lane per opening and leaves one partial per block; one block joins.
constexpr size_t kzg_parts(size_t n) { return ceil_div(n, WEIGHTED_BLOCK); }
// scratch: weights mod r [4][n]; the 2n scalars and bases of the first multi-scalar multiplication; the block partials and s; m1, m2,
// s G1gen [8] each; the pair list [8 + 16][2]; then the flags of the 2n bases, of the three points and of the two pairs
struct KzgWeightedLayout { size_t wr, sc, bases, partial, s, m1, m2, sg, pxy, qxy, binf, m1inf, m2inf, sginf, pinf, qinf, bytes; };
constexpr KzgWeightedLayout kzg_weighted_layout(size_t n) {
  Carve c; KzgWeightedLayout l{};
  l.wr = c.words(mul_sat(FR_WORDS, n));
  l.sc = c.words(mul_sat(2 * FR_WORDS, n));
  l.bases = c.words(mul_sat(2 * G1_WORDS, n));
  l.partial = c.words(mul_sat(FR_WORDS, kzg_parts(n)));
  l.s = c.words(FR_WORDS);
  l.m1 = c.words(G1_WORDS);
  l.m2 = c.words(G1_WORDS);
  l.sg = c.words(G1_WORDS);
  l.pxy = c.words(2 * G1_WORDS);
  l.qxy = c.words(2 * G2_WORDS);
  l.binf = c.bytes(mul_sat(2, n));
  l.m1inf = c.bytes(1);
  l.m2inf = c.bytes(1);
  l.sginf = c.bytes(1);
  l.pinf = c.bytes(2);
  l.qinf = c.bytes(2);
  l.bytes = c.at; return l;
}

// ---- Groth16: the column sums s = sum_i r_i and s_j = sum_i r_i x_ij in two levels, so that a few columns still fill the GPU: block
// (column, part) walks its column with a stride of parts * WEIGHTED_BLOCK rows, FR_ROWS_PER_LANE rows to a lane until FR_PARTS_MAX parts
// -- what one joining block takes in one round -- are reached.
constexpr size_t FR_ROWS_PER_LANE = 8, FR_PARTS_MAX = WEIGHTED_BLOCK;
constexpr size_t groth16_parts(size_t n) {
  return ceil_div(n, WEIGHTED_BLOCK * FR_ROWS_PER_LANE) < FR_PARTS_MAX ? ceil_div(n, WEIGHTED_BLOCK * FR_ROWS_PER_LANE) : FR_PARTS_MAX;
}
constexpr size_t groth16_columns(size_t n_inputs) { return add_sat(n_inputs, 1); }          // s, then an s_j per input
constexpr size_t groth16_bases(size_t n_inputs) { return add_sat(n_inputs, 2); }            // IC_0 .. IC_l, then alpha
constexpr size_t groth16_pairs(size_t n) { return add_sat(n, 3); }                          // (r_i A_i, B_i), then beta, gamma, delta
// scratch: weights mod r [4][n], r_i A_i [8][n], bases / scalars / products of the l + 2 per-call terms, sum_i r_i C_i [8], the pair list
// [8 + 16][n + 3], the partials [4][columns * parts]; then the flags of r_i A_i, of the products, of the sum and of the pairs
struct Groth16WeightedLayout { size_t wr, ra, bases, sums, prod, sc, pxy, qxy, partial, ra_inf, prod_inf, sc_inf, pinf, qinf, bytes; };
constexpr Groth16WeightedLayout groth16_weighted_layout(size_t n, size_t n_inputs) {
  const size_t cols = groth16_columns(n_inputs), nb = groth16_bases(n_inputs), m = groth16_pairs(n);
  Carve c; Groth16WeightedLayout l{};
  l.wr = c.words(mul_sat(FR_WORDS, n));
  l.ra = c.words(mul_sat(G1_WORDS, n));
  l.bases = c.words(mul_sat(G1_WORDS, nb));
  l.sums = c.words(mul_sat(FR_WORDS, nb));
  l.prod = c.words(mul_sat(G1_WORDS, nb));
  l.sc = c.words(G1_WORDS);
  l.pxy = c.words(mul_sat(G1_WORDS, m));
  l.qxy = c.words(mul_sat(G2_WORDS, m));
  l.partial = c.words(mul_sat(FR_WORDS, mul_sat(cols, groth16_parts(n))));
  l.ra_inf = c.bytes(n);
  l.prod_inf = c.bytes(nb);
  l.sc_inf = c.bytes(1);
  l.pinf = c.bytes(m);
  l.qinf = c.bytes(m);
  l.bytes = c.at; return l;
}
}  // namespace weighted_plan
