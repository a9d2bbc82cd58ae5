// CPU-only check of the planner of the several-point KZG opening (sylow_amd/csrc/kzg_points_plan.hpp): the limit on k, rows and items, grids
// at 0, 1 and the caps, every scratch size at its edges and where it saturates, the chunks of the verifier's G2 half under a byte budget and
// the layout of the verifier's lease.  Every expected value below is written out by hand from the rules in the header's comments (a chunk is
// 2048 coefficients, 2^20 blocks at most, 2536 bytes per (row, term) pair of the G2 half); nothing on the expected side is computed from the
// header.  Built with -fsanitize=address,undefined by tests/test_kzg_points_plan.py: host code only.
#include "../../sylow_amd/csrc/kzg_points_plan.hpp"

#include <cstdint>
#include <cstdio>

using namespace kzgpt_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static const size_t TOP = SIZE_MAX, M20 = (size_t)1 << 20;

static void limits() {
  EXPECT(KZGPT_MAX_POINTS == 64 && KZGPT_BLOCK == 256 && KZGPT_ROW_BLOCK == 64 && KZGPT_GRID_CAP == 1048576, "constants");
  EXPECT(!points_ok(0) && points_ok(1) && points_ok(64) && !points_ok(65) && !points_ok(TOP), "1 <= k <= 64");
  EXPECT(mul_sat(0, TOP) == 0 && mul_sat(TOP, 0) == 0 && mul_sat(TOP, 1) == TOP && mul_sat(TOP, 2) == SAT, "sat_mul at the ends");
  EXPECT(mul_sat((size_t)1 << 32, (size_t)1 << 32) == SAT && mul_sat((size_t)1 << 32, ((size_t)1 << 32) - 1) == 0xFFFFFFFF00000000ull, "sat_mul at 2^64");
  EXPECT(add_sat(0, 0) == 0 && add_sat(TOP, 0) == TOP && add_sat(TOP, 1) == SAT && add_sat(TOP - 1, 1) == SAT && add_sat(1, 2) == 3, "sat_add");
}

static void items() {
  EXPECT(pairs(5, 3) == 15 && pairs(0, 64) == 0 && pairs(TOP, 64) == SAT && pairs(TOP / 64, 64) == 0xFFFFFFFFFFFFFFC0ull, "(polynomial, point) pairs");
  const size_t ch[][2] = {{0, 0}, {1, 1}, {2047, 1}, {2048, 1}, {2049, 2}, {4096, 2}, {4097, 3}, {M20, 512}, {M20 + 1, 513}};
  for (const auto& c : ch) EXPECT(chunks(c[0]) == c[1], "chunks(%zu) = %zu", c[0], chunks(c[0]));
  EXPECT(carry_levels(1) == 0 && carry_levels(2048) == 0 && carry_levels(2049) == 1 && carry_levels(M20) == 1, "one carry level past one chunk");
  EXPECT(scan_items(2048, 5, 3) == 15 && scan_items(2049, 5, 3) == 30 && scan_items(M20, 1, 16) == 8192, "(polynomial, point, chunk) triples");
  EXPECT(scan_items(M20, TOP / 64, 64) == SAT && scan_items(2048, 0, 64) == 0, "triples saturate");
  EXPECT(chunk_items(2048, 5) == 5 && chunk_items(2049, 5) == 10 && chunk_items(M20, TOP) == SAT, "(polynomial, chunk) pairs");
  EXPECT(block_grid(0) == 0 && block_grid(1) == 1 && block_grid(M20 - 1) == M20 - 1 && block_grid(M20) == M20 && block_grid(M20 + 1) == M20 && block_grid(SAT) == M20,
         "a block per item up to the cap");
  const size_t lg[][2] = {{0, 0}, {1, 1}, {255, 1}, {256, 1}, {257, 2}, {(size_t)1 << 28, M20}, {((size_t)1 << 28) + 1, M20}, {((size_t)1 << 28) - 256, M20 - 1}, {TOP, M20}};
  for (const auto& l : lg) EXPECT(lane_grid(l[0]) == l[1], "lane_grid(%zu) = %zu", l[0], lane_grid(l[0]));
}

static void scratch() {
  EXPECT(weights_scratch_words(5, 3) == 60 && weights_scratch_words(1, 1) == 4 && weights_scratch_words(TOP / 4, 4) == SAT, "denominators [4][mk]");
  EXPECT(quot_scratch_words(2048, 5, 3) == 120, "one chunk: denominators and weights only, %zu", quot_scratch_words(2048, 5, 3));
  EXPECT(quot_scratch_words(2049, 5, 3) == 360, "two chunks: + totals and carries [4][30] each, %zu", quot_scratch_words(2049, 5, 3));
  EXPECT(quot_scratch_words(M20, 1, 16) == 65664, "2^20 coefficients at 16 points: 128 + 8 * 8192 words, %zu", quot_scratch_words(M20, 1, 16));
  EXPECT(quot_scratch_words(1, 1, 1) == 8 && quot_scratch_words(2049, TOP / 128, 64) == SAT && quot_scratch_words(M20, TOP / 64, 64) == SAT, "edges and saturation");
  EXPECT(poly_bytes(33, 5) == 5280 && poly_bytes(1, 1) == 32 && poly_bytes((size_t)1 << 59, 1) == SAT && poly_bytes((size_t)1 << 30, (size_t)1 << 30) == SAT, "32 len m bytes");
  EXPECT(polys_scratch_words(7, 4) == 224 && polys_scratch_words(TOP / 8, 8) == SAT, "the Fr half: 8 words per pair");
}

static void g2_chunks() {
  EXPECT(KZGPT_G2_BYTES_PER_TERM == 2536, "2048 + 32 + 128 + 128 + 8 + 192");
  EXPECT(g2_rows_per_chunk(10, 3, 0) == 1 && g2_rows_per_chunk(0, 3, 0) == 0 && g2_rows_per_chunk(0, 3, TOP) == 0, "at least one row; none of none");
  EXPECT(g2_rows_per_chunk(10, 3, 3 * 4 * 2536) == 3 && g2_rows_per_chunk(10, 3, 3 * 4 * 2536 - 1) == 2 && g2_rows_per_chunk(10, 3, TOP) == 10, "k + 1 = 4 terms per row");
  EXPECT(g2_rows_per_chunk(10, 3, 10 * 4 * 2536) == 10 && g2_rows_per_chunk(10, 3, 10 * 4 * 2536 - 1) == 9, "the whole batch exactly");
  EXPECT(g2_rows_per_chunk(5, 64, 164839) == 1 && g2_rows_per_chunk(5, 64, 164840) == 1 && g2_rows_per_chunk(5, 64, 329680) == 2, "65 terms per row at k = 64");
  EXPECT(g2_rows_per_chunk(7, 1, 2 * 2536 * 7) == 7 && g2_rows_per_chunk(7, 1, 2 * 2536 * 6 + 5071) == 6, "k = 1");
}

static void verify_lease() {
  const VerifyLayout v = verify_layout(3, 2, 2);
  // the offsets are bytes now: 8 times the words the u64 arrays had, and the flags behind the 456 words
  EXPECT(v.z == 0 && v.r == 8 * 36 && v.rc == 8 * 60 && v.f == 8 * 84 && v.zg == 8 * 108 && v.part == 8 * 156 && v.sc == 8 * 188 && v.bases == 8 * 212,
         "words: %zu %zu %zu %zu %zu %zu %zu", v.r, v.rc, v.f, v.zg, v.part, v.sc, v.bases);
  EXPECT(v.p == 8 * 308 && v.q == 8 * 356 && v.offs == 8 * 452 && v.distinct == 8 * 456, "the pair list: %zu %zu %zu %zu", v.p, v.q, v.offs, v.distinct);
  const size_t w = 8 * 456;
  EXPECT(v.distinct == w + 0 && v.is_one == w + 3 && v.rc_inf == w + 6 && v.f_inf == w + 9 && v.zg_inf == w + 12 && v.part_inf == w + 15 && v.p_inf == w + 18 &&
             v.q_inf == w + 24 && v.bytes == w + 30,
         "flags: %zu", v.bytes);
  const Region r[] = {WORDS(v, z, 36), WORDS(v, r, 24), WORDS(v, rc, 24), WORDS(v, f, 24), WORDS(v, zg, 48), WORDS(v, part, 32), WORDS(v, sc, 24), WORDS(v, bases, 96),
                      WORDS(v, p, 48), WORDS(v, q, 96), WORDS(v, offs, 4), BYTES(v, distinct, 3), BYTES(v, is_one, 3), BYTES(v, rc_inf, 3), BYTES(v, f_inf, 3),
                      BYTES(v, zg_inf, 3), BYTES(v, part_inf, 3), BYTES(v, p_inf, 6), BYTES(v, q_inf, 6)};
  EXPECT(layout_ok("verify", r, v.bytes), "3 rows at 2 points in chunks of 2");
  EXPECT(verify_scratch_bytes(3, 2, 2) == 456 * 8 + 30, "%zu", verify_scratch_bytes(3, 2, 2));
  const VerifyLayout one = verify_layout(1, 1, 1);
  EXPECT(one.r == 8 * 8 && one.rc == 8 * 12 && one.f == 8 * 20 && one.zg == 8 * 28 && one.part == 8 * 44 && one.sc == 8 * 60 && one.bases == 8 * 68 && one.p == 8 * 100 &&
             one.q == 8 * 116 && one.offs == 8 * 148 && one.distinct == 8 * 150 && one.bytes == 8 * 150 + 10,
         "one row of one point: %zu words", one.distinct / 8);
  const Region q[] = {WORDS(one, z, 8), WORDS(one, r, 4), WORDS(one, rc, 8), WORDS(one, f, 8), WORDS(one, zg, 16), WORDS(one, part, 16), WORDS(one, sc, 8), WORDS(one, bases, 32),
                      WORDS(one, p, 16), WORDS(one, q, 32), WORDS(one, offs, 2), BYTES(one, distinct, 1), BYTES(one, is_one, 1), BYTES(one, rc_inf, 1), BYTES(one, f_inf, 1),
                      BYTES(one, zg_inf, 1), BYTES(one, part_inf, 1), BYTES(one, p_inf, 2), BYTES(one, q_inf, 2)};
  EXPECT(layout_ok("verify of one", q, one.bytes), "one row of one point");
  EXPECT(verify_scratch_bytes(TOP / 8, 64, 1) == SAT && verify_scratch_bytes(TOP, 1, TOP) == SAT && verify_scratch_bytes((size_t)1 << 58, 1, 1) == SAT, "saturation");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // 5 polynomials of two chunks at 3 points: 15 pairs, 30 triples
    const PointsQuotLayout l = points_quot_layout(2049, 5, 3);
    const Region r[] = {WORDS(l, den, 60), WORDS(l, a, 60), WORDS(l, totals, 120), WORDS(l, carries, 120)};
    EXPECT(layout_ok("quotient", r, l.bytes) && l.a == 480 && l.totals == 960 && l.carries == 1920 && l.bytes == 2880, "quotient: %zu", l.bytes);
  }
  {  // one chunk: no totals and no carries
    const PointsQuotLayout l = points_quot_layout(2048, 5, 3);
    const Region r[] = {WORDS(l, den, 60), WORDS(l, a, 60), WORDS(l, totals, 0), WORDS(l, carries, 0)};
    EXPECT(layout_ok("quotient, one chunk", r, l.bytes) && l.a == 480 && l.carries == 960 && l.bytes == 960, "one chunk: %zu", l.bytes);
    EXPECT(points_quot_layout(1, 1, 1).a == 32 && points_quot_layout(1, 1, 1).bytes == 64 && points_quot_layout(2049, TOP / 128, 64).bytes == SAT, "one pair; saturates");
  }
  {
    const PolysLayout l = polys_layout(7, 4);
    const Region r[] = {WORDS(l, den, 112), WORDS(l, a, 112)};
    EXPECT(layout_ok("polys", r, l.bytes) && l.a == 896 && l.bytes == 1792 && polys_layout(1, 1).a == 32 && polys_layout(1, 1).bytes == 64 && polys_layout(TOP / 8, 8).bytes == SAT,
           "polys: %zu", l.bytes);
    EXPECT(weights_scratch_bytes(5, 3) == 480 && weights_scratch_bytes(TOP / 4, 4) == SAT, "the weights: one region");
  }
}

int main() {
  limits();
  items();
  scratch();
  g2_chunks();
  verify_lease();
  layouts();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
