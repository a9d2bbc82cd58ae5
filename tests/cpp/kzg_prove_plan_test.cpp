// CPU-only check of the KZG prover's planner (sylow_amd/csrc/kzg_prove_plan.hpp): the quotient's geometry and the commitment's route on a
// grid of (len, m, budget).  Every expected value below is written out by hand from the rules in the header's comments (a lane owns 8
// coefficients, a block 256 lanes, 1288 bytes per short-route pair); nothing on the expected side is computed from the header.
// Built with -fsanitize=address,undefined by tests/test_kzg_prove_plan.py: host code only.
#include "../../sylow_amd/csrc/kzg_prove_plan.hpp"

#include <cstdint>
#include <cstdio>

using namespace kzg_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static const char* name(Route r) { return r == Route::SHORT ? "SHORT" : r == Route::BUCKET ? "BUCKET" : "MSM_EACH"; }

static void quotient_geometry() {
  EXPECT(KZG_POLY_BLOCK == 256 && KZG_POLY_LANE_COEFFS == 8 && KZG_POLY_CHUNK == 2048, "constants");
  const size_t chunks[][2] = {{1, 1}, {2, 1}, {7, 1}, {8, 1}, {9, 1}, {2047, 1}, {2048, 1}, {2049, 2}, {4096, 2}, {4097, 3}, {1u << 20, 512}, {(1u << 20) + 1, 513}};
  for (const auto& c : chunks) EXPECT(quot_chunks(c[0]) == c[1], "quot_chunks(%zu) = %zu", c[0], quot_chunks(c[0]));
  EXPECT(quot_items(2049, 5) == 10 && quot_items(2048, 5) == 5 && quot_items(1, 0) == 0, "items");
  EXPECT(quot_grid(10) == 10 && quot_grid(1048576) == 1048576 && quot_grid(1048577) == 1048576 && quot_grid(0) == 0, "grid");
  // one chunk: one launch, no scratch; more: one carry level, totals + carries of 4 words per (polynomial, chunk)
  EXPECT(quot_carry_levels(1) == 0 && quot_carry_levels(2048) == 0 && quot_carry_levels(2049) == 1 && quot_carry_levels(1u << 20) == 1, "levels");
  EXPECT(quot_scratch_words(2048, 5) == 0 && quot_scratch_words(2049, 5) == 80 && quot_scratch_words(4097, 1) == 24, "scratch");
  // the carry level walks tiles of 256 chunks: 256 chunks are one tile, one chunk more is two
  EXPECT(quot_carry_tiles(2049) == 1 && quot_carry_tiles(524288) == 1 && quot_carry_tiles(524289) == 2 && quot_carry_tiles(1048577) == 3, "tiles");
  // m len = 2^33 three ways: nothing wraps at 32 bits
  const size_t two33 = (size_t)1 << 33;
  EXPECT(quot_items(8192, (size_t)1 << 20) == 4194304 && quot_grid(quot_items(8192, (size_t)1 << 20)) == 1048576, "2^13 x 2^20");
  EXPECT(quot_scratch_words(8192, (size_t)1 << 20) == 33554432, "2^13 x 2^20 scratch");
  EXPECT(quot_items(1, two33) == 8589934592ull && quot_grid(quot_items(1, two33)) == 1048576 && quot_scratch_words(1, two33) == 0, "1 x 2^33");
  EXPECT(quot_chunks(two33) == 4194304 && quot_carry_tiles(two33) == 16384 && quot_scratch_words(two33, 1) == 33554432, "2^33 x 1");
  EXPECT(quot_chunks(two33 + 1) == 4194305, "2^33 + 1");
}

static void commit_routes() {
  EXPECT(KZG_SHORT_BYTES_PER_TERM == 1288, "%zu", KZG_SHORT_BYTES_PER_TERM);
  EXPECT(short_bytes_per_poly(1) == 1288 && short_bytes_per_poly(16) == 20608 && short_bytes_per_poly(257) == 331016, "bytes per polynomial");
  EXPECT(short_bytes_per_poly(SIZE_MAX / 2) == SIZE_MAX && short_bytes_per_poly(SIZE_MAX) == SIZE_MAX, "saturates");
  // budgets of exactly k polynomials and one byte less, at (len, m) = (16, 64): 20608 bytes each
  const size_t per[][2] = {{20608 * 1, 1}, {20608 * 2 - 1, 1}, {20608 * 10, 10}, {20608 * 10 - 1, 9}, {20608 * 63, 63}, {20608 * 64 - 1, 63}, {20608 * 64, 64},
                           {20608 * 65, 64}, {(size_t)1 << 30, 64}, {20607, 0}, {0, 0}};
  for (const auto& p : per) EXPECT(short_polys_per_chunk(16, 64, p[0]) == p[1], "short_polys_per_chunk(16, 64, %zu) = %zu", p[0], short_polys_per_chunk(16, 64, p[0]));
  EXPECT(short_polys_per_chunk(SIZE_MAX / 2, 3, SIZE_MAX - 1) == 0, "a saturated polynomial never fits");
  const size_t GB = (size_t)1 << 30, MIN = (size_t)1 << 18;
  struct Case { size_t len, m, min_len, budget; Route route; size_t per_chunk; };
  const Case cases[] = {
      {1, 1, MIN, GB, Route::SHORT, 1},
      {16, 64, MIN, GB, Route::SHORT, 64},
      {16, 64, MIN, 20608 * 10, Route::SHORT, 10},
      {16, 64, MIN, 20607, Route::MSM_EACH, 0},                 // not even one polynomial fits: each through sylow_hip_g1_msm
      {262143, 2, MIN, GB, Route::SHORT, 2},                    // min_len - 1: 337 640 184 bytes each, three fit a GB
      {262143, 10, MIN, GB, Route::SHORT, 3},
      {262144, 10, MIN, GB, Route::BUCKET, 0},                  // min_len
      {262144, 10, MIN, 1, Route::BUCKET, 0},                   // the bucket route is not this plan's budget to check
      {1000000, 4, (size_t)1 << 21, GB, Route::MSM_EACH, 0},    // 1 288 000 000 bytes > 1 GB
      {1, 7, 0, GB, Route::BUCKET, 0},                          // min_len = 0: always
      {300, 3, 1, GB, Route::BUCKET, 0},
      {299, 3, 300, GB, Route::SHORT, 3},
      {300, 3, 300, GB, Route::BUCKET, 0},
      {1, (size_t)1 << 33, MIN, GB, Route::SHORT, 833650},      // 2^30 / 1288 pairs per chunk
      {8192, (size_t)1 << 20, MIN, GB, Route::SHORT, 101},      // 10 551 296 bytes each
  };
  for (const Case& c : cases) {
    const CommitPlan p = commit_plan(c.len, c.m, c.min_len, c.budget);
    EXPECT(p.route == c.route && p.polys_per_chunk == c.per_chunk, "commit_plan(%zu, %zu, %zu, %zu) = %s / %zu", c.len, c.m, c.min_len, c.budget, name(p.route),
           p.polys_per_chunk);
  }
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {
    const QuotLayout l = quot_layout(2049, 5);
    const Region r[] = {WORDS(l, totals, 40), WORDS(l, carries, 40)};
    EXPECT(layout_ok("quotient", r, l.bytes) && l.carries == 320 && l.bytes == 640, "quotient: %zu", l.bytes);
    EXPECT(quot_layout(2048, 5).bytes == 0 && quot_layout(2048, 5).carries == 0 && quot_layout(2049, SIZE_MAX / 2).bytes == SIZE_MAX, "one chunk leases nothing; saturates");
    EXPECT(coeffs_bytes(3, 5) == 4 * 3 * 5 * 8 && coeffs_bytes(1, 1) == 32 && coeffs_bytes((size_t)1 << 59, 1) == SIZE_MAX, "4 len m words of quotients or coefficients");
  }
  {  // a multi-scalar multiplication per polynomial: (8 m + (canonical ? 0 : 4 len)) words + m bytes
    const MsmEachLayout l = msm_each_layout(3, 5, false);
    const Region r[] = {WORDS(l, pts, 40), WORDS(l, sc, 12), BYTES(l, inf, 5)};
    EXPECT(layout_ok("msm each", r, l.bytes) && l.sc == 320 && l.inf == 416 && l.bytes == (8 * 5 + 4 * 3) * 8 + 5, "msm each: %zu", l.bytes);
    const MsmEachLayout c = msm_each_layout(3, 5, true);
    const Region q[] = {WORDS(c, pts, 40), WORDS(c, sc, 0), BYTES(c, inf, 5)};
    EXPECT(layout_ok("msm each, canonical", q, c.bytes) && c.sc == 320 && c.inf == 320 && c.bytes == 8 * 5 * 8 + 5, "canonical: %zu", c.bytes);
    EXPECT(msm_each_layout(3, 1, false).inf == 160 && msm_each_layout(3, 1, false).bytes == (8 + 12) * 8 + 1 && msm_each_layout(SIZE_MAX, 1, false).bytes == SIZE_MAX, "m = 1; saturates");
  }
  {  // the short route: (4 n + 8 n + 8 n + w_acc + (direct ? 0 : 8 per_chunk)) words + n + per_chunk bytes.  2 polynomials of 3 terms a chunk, w_acc = 7
    const ShortLayout l = short_layout(3, 2, 7, false);
    const Region r[] = {WORDS(l, sc, 24), WORDS(l, bases, 48), WORDS(l, prod, 48), WORDS(l, acc, 7), WORDS(l, part, 16), BYTES(l, prod_inf, 6), BYTES(l, part_inf, 2)};
    EXPECT(layout_ok("short", r, l.bytes) && l.bases == 192 && l.prod == 576 && l.acc == 960 && l.part == 1016 && l.prod_inf == 1144 && l.part_inf == 1150 &&
               l.bytes == (24 + 48 + 48 + 7 + 16) * 8 + 6 + 2, "short: %zu", l.bytes);
  }
  {  // one chunk: the segmented sum writes the caller's array, no sums in scratch
    const ShortLayout l = short_layout(3, 2, 7, true);
    const Region r[] = {WORDS(l, sc, 24), WORDS(l, bases, 48), WORDS(l, prod, 48), WORDS(l, acc, 7), WORDS(l, part, 0), BYTES(l, prod_inf, 6), BYTES(l, part_inf, 2)};
    EXPECT(layout_ok("short, direct", r, l.bytes) && l.part == 1016 && l.prod_inf == 1016 && l.part_inf == 1022 && l.bytes == (24 + 48 + 48 + 7) * 8 + 6 + 2, "direct: %zu", l.bytes);
    const ShortLayout d = short_layout(3, 5, 0, true);
    const Region q[] = {WORDS(d, sc, 60), WORDS(d, bases, 120), WORDS(d, prod, 120), WORDS(d, acc, 0), WORDS(d, part, 0), BYTES(d, prod_inf, 15), BYTES(d, part_inf, 5)};
    EXPECT(layout_ok("short, one stage", q, d.bytes) && d.acc == 2400 && d.prod_inf == 2400 && d.part_inf == 2415 && d.bytes == 300 * 8 + 15 + 5, "one stage: %zu", d.bytes);
    EXPECT(short_layout(SIZE_MAX, 2, 0, false).bytes == SIZE_MAX, "saturates");
  }
}

int main() {
  quotient_geometry();
  commit_routes();
  layouts();
  if (fails) { printf("%d of %zu checks failed\n", fails, checked); return 1; }
  printf("OK %zu checks\n", checked);
  return 0;
}
