// kzg_points_plan.hpp -- the geometry of the KZG opening of ONE polynomial at SEVERAL points under one proof (kzg_points.hip): the items of
// the scan passes, grids, scratch sizes and offsets (saturating) and the chunks of the verifier's G2 half.  Plain C++ so that
// tests/cpp/kzg_points_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch code asks these functions and decides nothing
// itself.  The lane and chunk geometry of the scan is kzg_prove_plan.hpp's: the kernels here run the same scan once per point.
#pragma once
#include "kzg_prove_plan.hpp"
#include "plan_base.hpp"

namespace kzgpt_plan {
using plan_base::Carve;
using plan_base::add_sat;
using plan_base::mul_sat;
using plan_base::words_of;
using plan_base::SAT;                                  // "does not fit size_t": the entry point refuses it before any lease
constexpr size_t KZGPT_MAX_POINTS = 64;                 // k of one call, at most: a data-availability cell
constexpr int KZGPT_BLOCK = 256;                        // == BLOCK of common.hpp (kzg_points.hip asserts it)
constexpr int KZGPT_ROW_BLOCK = 64;                     // the Fr half of the verifier: ONE wavefront per row, lane i on point i
static_assert((size_t)KZGPT_ROW_BLOCK >= KZGPT_MAX_POINTS, "a lane per point");
constexpr size_t KZGPT_GRID_CAP = (size_t)1 << 20;      // blocks of one launch; more work than that is walked with a grid stride

constexpr bool points_ok(size_t k) { return k >= 1 && k <= KZGPT_MAX_POINTS; }

// ---- rows and items ------------------------------------------------------------------------------------------------------------------
// (polynomial, point) pairs: the elements of z, y and the weights, [4][m k], pair (j, i) at index j k + i
constexpr size_t pairs(size_t m, size_t k) { return mul_sat(m, k); }
constexpr size_t chunks(size_t len) { return kzg_plan::quot_chunks(len); }
// 0: every polynomial is one chunk -- ONE launch after the weights; 1: totals, the carry level, then the chunks
constexpr int carry_levels(size_t len) { return kzg_plan::quot_carry_levels(len); }
// (polynomial, point, chunk) triples: the work items of the totals pass and the slots of totals and carries
constexpr size_t scan_items(size_t len, size_t m, size_t k) { return mul_sat(pairs(m, k), chunks(len)); }
// (polynomial, chunk) pairs: the work items of the chunk kernel, which walks the k points itself and stores the quotient ONCE
constexpr size_t chunk_items(size_t len, size_t m) { return mul_sat(m, chunks(len)); }
constexpr size_t block_grid(size_t items) { return items < KZGPT_GRID_CAP ? items : KZGPT_GRID_CAP; }
// one lane per element, blocks of KZGPT_BLOCK
constexpr size_t lane_grid(size_t n) {
  return n / KZGPT_BLOCK + (n % KZGPT_BLOCK ? 1 : 0) < KZGPT_GRID_CAP ? n / KZGPT_BLOCK + (n % KZGPT_BLOCK ? 1 : 0) : KZGPT_GRID_CAP;
}

// ---- scratch, in u64 words -----------------------------------------------------------------------------------------------------------
// the weights: the denominators [4][m k] that sylow_hip_fr_batch_inv reads (its output must not overlap them)
constexpr size_t weights_scratch_words(size_t m, size_t k) { return mul_sat(4, pairs(m, k)); }
constexpr size_t weights_scratch_bytes(size_t m, size_t k) { return mul_sat(weights_scratch_words(m, k), 8); }
// the quotient: denominators and weights [4][m k] each, then totals and carries [4][items] each (none for one chunk)
struct PointsQuotLayout { size_t den, a, totals, carries, bytes; };
constexpr PointsQuotLayout points_quot_layout(size_t len, size_t m, size_t k) {
  Carve c; PointsQuotLayout l{};
  l.den = c.words(mul_sat(4, pairs(m, k)));
  l.a = c.words(mul_sat(4, pairs(m, k)));
  l.totals = c.words(carry_levels(len) ? mul_sat(4, scan_items(len, m, k)) : 0);
  l.carries = c.words(carry_levels(len) ? mul_sat(4, scan_items(len, m, k)) : 0);
  l.bytes = c.at; return l;
}
constexpr size_t quot_scratch_words(size_t len, size_t m, size_t k) { return words_of(points_quot_layout(len, m, k).bytes); }
// bytes of coeffs and of q_out, for the overlap check and the opening's quotient in scratch
constexpr size_t poly_bytes(size_t len, size_t m) { return kzg_plan::coeffs_bytes(len, m); }
// the Fr half: denominators and weights [4][n k] each
struct PolysLayout { size_t den, a, bytes; };
constexpr PolysLayout polys_layout(size_t n, size_t k) {
  Carve c; PolysLayout l{};
  l.den = c.words(mul_sat(4, pairs(n, k)));
  l.a = c.words(mul_sat(4, pairs(n, k)));
  l.bytes = c.at; return l;
}
constexpr size_t polys_scratch_words(size_t n, size_t k) { return words_of(polys_layout(n, k).bytes); }

// ---- the verifier ---------------------------------------------------------------------------------------------------------------------
// Bytes a (row, term) pair of the G2 half takes: the window tables sylow_hip_g2_scalar_mul_batch leases (1 KB per lane of a lane pair), the
// scalar (32), the replicated base (128), the product (128 + its flag, padded to 8) and the segmented sum's partials (at most one projective
// point, 192)
constexpr size_t KZGPT_G2_BYTES_PER_TERM = 2048 + 32 + 128 + 128 + 8 + 192;
// whole rows one chunk of the G2 half holds under `budget` bytes, at least one
constexpr size_t g2_rows_per_chunk(size_t n, size_t k, size_t budget) {
  return budget / ((k + 1) * KZGPT_G2_BYTES_PER_TERM) == 0 ? (n ? 1 : 0)
         : budget / ((k + 1) * KZGPT_G2_BYTES_PER_TERM) < n ? budget / ((k + 1) * KZGPT_G2_BYTES_PER_TERM)
                                                           : n;
}
// Layout of the verifier's lease, u64 words first, bytes after them.  Z [n][4][k+1] | R [n][4][k] | R(tau) G1gen [8][n] | F [8][n] |
// Z(tau) G2gen [16][n] | one chunk's G2 sum [16][rows] | its scalars [4][rows (k+1)] and bases [16][rows (k+1)] | pairs: p [8][2n], q [16][2n],
// pair_offsets [n+1] || distinct [n] | is_one [n] | flags of R(tau) G1gen, F, Z(tau) G2gen, the chunk's sum [n] each | pair flags p, q [2n] each
struct VerifyLayout {
  size_t z, r, rc, f, zg, part, sc, bases, p, q, offs;                                          // byte offsets of the u64 arrays
  size_t distinct, is_one, rc_inf, f_inf, zg_inf, part_inf, p_inf, q_inf, bytes;                // of the flags behind them, and the total
};
constexpr VerifyLayout verify_layout(size_t n, size_t k, size_t rows) {
  Carve c; VerifyLayout v{};
  v.z = c.words(mul_sat(mul_sat(4, n), k + 1));
  v.r = c.words(mul_sat(mul_sat(4, n), k));
  v.rc = c.words(mul_sat(8, n));
  v.f = c.words(mul_sat(8, n));
  v.zg = c.words(mul_sat(16, n));
  v.part = c.words(mul_sat(16, rows));
  v.sc = c.words(mul_sat(mul_sat(4, rows), k + 1));
  v.bases = c.words(mul_sat(mul_sat(16, rows), k + 1));
  v.p = c.words(mul_sat(16, n));
  v.q = c.words(mul_sat(32, n));
  v.offs = c.words(add_sat(n, 1));
  v.distinct = c.bytes(n);
  v.is_one = c.bytes(n);
  v.rc_inf = c.bytes(n);
  v.f_inf = c.bytes(n);
  v.zg_inf = c.bytes(n);
  v.part_inf = c.bytes(n);
  v.p_inf = c.bytes(mul_sat(2, n));
  v.q_inf = c.bytes(mul_sat(2, n));
  v.bytes = c.at; return v;
}
// bytes of the whole lease; SAT when it does not fit
constexpr size_t verify_scratch_bytes(size_t n, size_t k, size_t rows) { return verify_layout(n, k, rows).bytes; }
}  // namespace kzgpt_plan
