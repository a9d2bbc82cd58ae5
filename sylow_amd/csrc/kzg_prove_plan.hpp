// kzg_prove_plan.hpp -- the geometry of the KZG quotient kernels and the route of a commitment (kzg_prove.hip): every decision, byte
// count and scratch offset between an entry point and its kernels, plain C++ so that tests/cpp/kzg_prove_plan_test.cpp can compile it with g++ on a box without a GPU.  The
// launch code asks these functions and decides nothing itself.
#pragma once
#include "plan_base.hpp"

namespace kzg_plan {
using plan_base::Carve;
using plan_base::mul_sat;
using plan_base::words_of;
// ---- the quotient: q(X) = (f(X) - f(z)) / (X - z) as the recurrence h_len = 0, h_k = f_k + z h_{k+1} --------------------------------
// A lane owns KZG_POLY_LANE_COEFFS consecutive coefficients, a block of KZG_POLY_BLOCK lanes a chunk of KZG_POLY_CHUNK; the chunks of one
// polynomial are joined by ONE carry level: a block per polynomial walks the chunk totals from the top in tiles of KZG_POLY_BLOCK chunks
// and hands the running carry from tile to tile, so the carry pass has no capacity of its own.
constexpr int KZG_POLY_BLOCK = 256;              // == BLOCK of common.hpp (kzg_prove.hip asserts it)
constexpr int KZG_POLY_LANE_COEFFS = 8;          // L: a power of two (the scan's multipliers are z^(L 2^s), a chain of squarings)
constexpr size_t KZG_POLY_CHUNK = 2048;          // CH = KZG_POLY_BLOCK * KZG_POLY_LANE_COEFFS
static_assert(KZG_POLY_CHUNK == (size_t)KZG_POLY_BLOCK * KZG_POLY_LANE_COEFFS, "a chunk is a block of lanes");
static_assert((KZG_POLY_LANE_COEFFS & (KZG_POLY_LANE_COEFFS - 1)) == 0 && (KZG_POLY_BLOCK & (KZG_POLY_BLOCK - 1)) == 0, "powers of two");
constexpr size_t KZG_QUOT_GRID_CAP = (size_t)1 << 20;   // blocks of one launch; more work than that is walked with a grid stride

constexpr size_t quot_chunks(size_t len) { return (len + KZG_POLY_CHUNK - 1) / KZG_POLY_CHUNK; }
// (polynomial, chunk) pairs of a batch: the work items of the two chunk kernels.  m len <= 2^64 - 1 is the caller's array; no product here
// is larger than it
constexpr size_t quot_items(size_t len, size_t m) { return quot_chunks(len) * m; }
constexpr size_t quot_grid(size_t items) { return items < KZG_QUOT_GRID_CAP ? items : KZG_QUOT_GRID_CAP; }
// 0: every polynomial is one chunk -- ONE launch, no totals, no carries; 1: totals, the carry level, then the chunks again
constexpr int quot_carry_levels(size_t len) { return quot_chunks(len) > 1 ? 1 : 0; }
// serial tiles of the carry level per polynomial
constexpr size_t quot_carry_tiles(size_t len) { return (quot_chunks(len) + KZG_POLY_BLOCK - 1) / KZG_POLY_BLOCK; }
// the scratch the quotient leases: the chunk totals and the carries, [4][m chunks] each; none for one chunk
struct QuotLayout { size_t totals, carries, bytes; };
constexpr QuotLayout quot_layout(size_t len, size_t m) {
  Carve c; QuotLayout l{};
  l.totals = c.words(quot_carry_levels(len) ? mul_sat(4, quot_items(len, m)) : 0);
  l.carries = c.words(quot_carry_levels(len) ? mul_sat(4, quot_items(len, m)) : 0);
  l.bytes = c.at; return l;
}
constexpr size_t quot_scratch_words(size_t len, size_t m) { return words_of(quot_layout(len, m).bytes); }
// bytes of m polynomials of len coefficients: the quotients of an opening, or the coefficients behind evaluations, in scratch
constexpr size_t coeffs_bytes(size_t len, size_t m) { return mul_sat(mul_sat(32, len), m); }

// ---- the commitment: out_j = sum_k f_jk srs_k ----------------------------------------------------------------------------------------
enum class Route {
  SHORT,       // every (polynomial, term) pair a lane of ONE sylow_hip_g1_scalar_mul_batch, then the segmented sum; in chunks of whole polynomials
  BUCKET,      // sylow_hip_g1_msm_tuned(min_n = 0) per polynomial: the bucket method
  MSM_EACH,    // sylow_hip_g1_msm per polynomial with its own defaults: the short route's fallback when ONE polynomial does not fit the budget
};
// Bytes the short route takes per (polynomial, term) pair: the window table sylow_hip_g1_scalar_mul_batch leases (1 KB), the scalar mod r
// (32), the replicated base (64), the product (64 + its flag, padded to 8) and the segmented sum's partials (at most one projective point, 96)
constexpr size_t KZG_SHORT_BYTES_PER_TERM = 1024 + 32 + 64 + 64 + 8 + 96;
// len * KZG_SHORT_BYTES_PER_TERM, saturated (len itself is bounded by the caller's array; the product need not be)
constexpr size_t short_bytes_per_poly(size_t len) {
  return len > (size_t)-1 / KZG_SHORT_BYTES_PER_TERM ? (size_t)-1 : len * KZG_SHORT_BYTES_PER_TERM;
}
// polynomials one chunk of the short route holds under `budget` bytes: 0 when not even one fits
constexpr size_t short_polys_per_chunk(size_t len, size_t m, size_t budget) {
  return budget / short_bytes_per_poly(len) < m ? budget / short_bytes_per_poly(len) : m;
}
struct CommitPlan {
  Route route;
  size_t polys_per_chunk;      // SHORT only: whole polynomials per chunk, >= 1
};
// min_len: the smallest len that takes the bucket route (the caller resolved a negative argument to the default); budget: the scratch
// limit in force, or the default
constexpr CommitPlan commit_plan(size_t len, size_t m, size_t min_len, size_t budget) {
  return len >= min_len ? CommitPlan{Route::BUCKET, 0}
         : short_polys_per_chunk(len, m, budget) == 0 ? CommitPlan{Route::MSM_EACH, 0}
                                                      : CommitPlan{Route::SHORT, short_polys_per_chunk(len, m, budget)};
}
// ---- the scratch of the commitment's routes ------------------------------------------------------------------------------------------------
// a multi-scalar multiplication per polynomial: the m sums [8] each, one polynomial's scalars mod r [4][len] unless they are canonical as
// they lie, and the m flags
struct MsmEachLayout { size_t pts, sc, inf, bytes; };
constexpr MsmEachLayout msm_each_layout(size_t len, size_t m, bool canonical) {
  Carve c; MsmEachLayout l{};
  l.pts = c.words(mul_sat(8, m));
  l.sc = c.words(canonical ? 0 : mul_sat(4, len));
  l.inf = c.bytes(m);
  l.bytes = c.at; return l;
}
// the short route, n = per_chunk * len pairs: the scalars [4][n], the bases and the products [8][n] each, the segmented sum's w_acc words
// (g1h::sum_segments_scratch_words of the larger of a whole and the last chunk), the chunk's sums [8][per_chunk] unless the one chunk writes
// the caller's array; then the flags of the products [n] and of the sums [per_chunk]
struct ShortLayout { size_t sc, bases, prod, acc, part, prod_inf, part_inf, bytes; };
constexpr ShortLayout short_layout(size_t len, size_t per_chunk, size_t w_acc, bool direct) {
  const size_t n = mul_sat(per_chunk, len);
  Carve c; ShortLayout l{};
  l.sc = c.words(mul_sat(4, n));
  l.bases = c.words(mul_sat(8, n));
  l.prod = c.words(mul_sat(8, n));
  l.acc = c.words(w_acc);
  l.part = c.words(direct ? 0 : mul_sat(8, per_chunk));
  l.prod_inf = c.bytes(n);
  l.part_inf = c.bytes(per_chunk);
  l.bytes = c.at; return l;
}
}  // namespace kzg_plan
