// CPU-only check of the planner of the folded KZG openings (sylow_amd/csrc/kzg_multi_plan.hpp): group offsets, the tiles and grids of the
// linear combination at 0, 1 and the caps, the scratch sizes, and the padded layout of ragged groups under a byte budget.  Every expected
// value below is written out by hand from the rules in the header's comments (a tile is 256 columns, 16 products per reduction, 65536 x 1024
// blocks at most, 1296 bytes per padded slot); nothing on the expected side is computed from the header.
// Built with -fsanitize=address,undefined by tests/test_kzg_multi_plan.py: host code only.
#include "../../sylow_amd/csrc/kzg_multi_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace kzgm_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static void groups() {
  const uint64_t ok[] = {0, 0, 3, 3, 4, 9, 9}, dec[] = {0, 3, 2, 9}, late[] = {1, 3, 9}, shortfall[] = {0, 3, 8}, one[] = {0, 9}, none[] = {0, 0, 0};
  EXPECT(groups_ok(ok, 6, 9), "ragged, empty groups first, in the middle and last");
  EXPECT(!groups_ok(dec, 3, 9), "decreasing");
  EXPECT(!groups_ok(late, 2, 9), "does not start at 0");
  EXPECT(!groups_ok(shortfall, 2, 9) && !groups_ok(ok, 6, 10), "does not end at m");
  EXPECT(!groups_ok(nullptr, 1, 1), "NULL");
  EXPECT(groups_ok(one, 1, 9) && groups_ok(none, 2, 0), "one group; only empty groups");
  EXPECT(longest_group(ok, 0, 6) == 5 && longest_group(ok, 0, 4) == 3 && longest_group(ok, 0, 1) == 0 && longest_group(ok, 3, 3) == 0, "longest");
  EXPECT(KZGM_OFFSET_ARGS == 256 && sizeof(uint64_t) * KZGM_OFFSET_ARGS == 2048, "2 KB of arguments");
  const size_t launches[][2] = {{0, 1}, {1, 1}, {255, 1}, {256, 2}, {511, 2}, {512, 3}, {1025, 5}};
  for (const auto& l : launches) EXPECT(offset_launches(l[0]) == l[1] && offset_words(l[0]) == l[0] + 1, "offset_launches(%zu) = %zu", l[0], offset_launches(l[0]));
}

static void lincomb_geometry() {
  EXPECT(KZGM_BLOCK == 256 && KZGM_LINCOMB_TILE == 256 && KZGM_LINCOMB_FLUSH == 16, "constants");
  EXPECT(KZGM_GRID_X_CAP == 65536 && KZGM_GRID_Y_CAP == 1024 && KZGM_LANE_GRID_CAP == 1048576, "caps");
  const size_t tiles[][2] = {{0, 0}, {1, 1}, {2, 1}, {255, 1}, {256, 1}, {257, 2}, {513, 3}, {1u << 20, 4096}, {(1u << 20) + 1, 4097}, {(size_t)1 << 24, 65536}};
  for (const auto& t : tiles) EXPECT(lincomb_tiles(t[0]) == t[1], "lincomb_tiles(%zu) = %zu", t[0], lincomb_tiles(t[0]));
  EXPECT(lincomb_tiles(SIZE_MAX) == ((size_t)1 << 56), "no wrap at the top: %zu", lincomb_tiles(SIZE_MAX));
  EXPECT(lincomb_grid_x(0) == 0 && lincomb_grid_x(1) == 1 && lincomb_grid_x((size_t)1 << 24) == 65536 && lincomb_grid_x(((size_t)1 << 24) + 1) == 65536, "grid x");
  EXPECT(lincomb_grid_x(((size_t)1 << 24) - 256) == 65535 && lincomb_grid_x((size_t)1 << 33) == 65536, "grid x at the cap");
  EXPECT(lincomb_grid_y(0) == 0 && lincomb_grid_y(1) == 1 && lincomb_grid_y(1023) == 1023 && lincomb_grid_y(1024) == 1024 && lincomb_grid_y(1025) == 1024, "grid y");
  const size_t rounds[][2] = {{0, 0}, {1, 1}, {15, 1}, {16, 1}, {17, 2}, {32, 2}, {33, 3}};
  for (const auto& r : rounds) EXPECT(lincomb_rounds(r[0]) == r[1], "lincomb_rounds(%zu) = %zu", r[0], lincomb_rounds(r[0]));
  EXPECT(lane_grid(0) == 0 && lane_grid(1) == 1 && lane_grid(256) == 1 && lane_grid(257) == 2 && lane_grid((size_t)1 << 28) == 1048576 &&
         lane_grid(((size_t)1 << 28) + 1) == 1048576 && lane_grid((size_t)1 << 40) == 1048576, "lane grid");
  EXPECT(group_grid(0) == 0 && group_grid(7) == 7 && group_grid(1048577) == 1048576, "group grid");
}

static void scratch() {
  EXPECT(sat_mul(0, SIZE_MAX) == 0 && sat_mul(SIZE_MAX, 0) == 0 && sat_mul(2, SIZE_MAX / 2 + 1) == SIZE_MAX && sat_mul(3, 5) == 15, "sat_mul");
  EXPECT(sat_add(SIZE_MAX, 1) == SIZE_MAX && sat_add(SIZE_MAX - 1, 1) == SIZE_MAX && sat_add(2, 3) == 5, "sat_add");
  // G + 1 offsets, 8 m words of powers and z, 4 G len words of F, 4 G of y_F
  EXPECT(open_scratch_words(1, 1, 1) == 2 + 8 + 4 + 4, "%zu", open_scratch_words(1, 1, 1));
  EXPECT(open_scratch_words(2049, 14, 2) == 3 + 112 + 16392 + 8, "%zu", open_scratch_words(2049, 14, 2));
  EXPECT(open_scratch_words(1u << 20, 32, 2) == 3 + 256 + 8388608 + 8, "32 G len bytes of F: %zu", open_scratch_words(1u << 20, 32, 2));
  EXPECT(open_scratch_words((size_t)1 << 40, 1, (size_t)1 << 40) == SIZE_MAX && open_scratch_words(1, SIZE_MAX / 4, 1) == SIZE_MAX, "saturates");
  EXPECT(combine_scratch_words(14, 2) == 3 + 56 && combine_scratch_words(SIZE_MAX / 2, 1) == SIZE_MAX, "combine");
  EXPECT(verify_scratch_words(1) == 13 && verify_scratch_words(8) == 97 && verify_scratch_words(9) == 110, "verify");
}

static const char* name(Route r) { return r == Route::SEGMENTS ? "SEGMENTS" : "MSM"; }

static void combine_chunks() {
  EXPECT(KZGM_BYTES_PER_SLOT == 1296, "%zu", KZGM_BYTES_PER_SLOT);
  const size_t GB = (size_t)1 << 30, MIN = (size_t)1 << 18;
  // ragged: sizes 0, 3, 1, 0, 5, 2, 0
  const uint64_t gs[] = {0, 0, 3, 4, 4, 9, 11, 11};
  struct Case { size_t g0, msm_min, budget; Route route; size_t g_end, terms; };
  const Case cases[] = {
      {0, MIN, GB, Route::SEGMENTS, 7, 5},                      // everything in one chunk, padded to the longest group: 7 x 5 slots
      {0, MIN, 1296 * 35, Route::SEGMENTS, 7, 5},               // exactly 35 slots
      {0, MIN, 1296 * 35 - 1, Route::SEGMENTS, 6, 5},           // one byte less: the last group waits (6 x 5 = 30 slots)
      {6, MIN, 1296 * 35 - 1, Route::SEGMENTS, 7, 1},           // an empty group alone still takes one padding slot
      {0, MIN, 1296 * 12, Route::SEGMENTS, 4, 3},               // 4 x 3 = 12; the group of 5 would make 5 x 5 = 25
      {4, MIN, 1296 * 12, Route::SEGMENTS, 6, 5},               // 2 x 5 = 10; a third group would make 15
      {4, MIN, 1296 * 4, Route::MSM, 5, 5},                     // 5 slots do not fit 4: the group goes through g1_msm on its own
      {0, 5, GB, Route::SEGMENTS, 4, 3},                        // the group of 5 is at the crossover: the chunk ends before it
      {4, 5, GB, Route::MSM, 5, 5},
      {5, 5, GB, Route::SEGMENTS, 7, 2},
      {1, 3, GB, Route::MSM, 2, 3},                             // at the crossover exactly
      {1, 4, GB, Route::SEGMENTS, 4, 3},
      {0, 1, GB, Route::SEGMENTS, 1, 1},                        // msm_min = 1: every non-empty group alone, empty ones as one padded slot
      {3, 1, GB, Route::SEGMENTS, 4, 1},
      {0, MIN, 0, Route::SEGMENTS, 1, 1},                       // no budget at all: an empty group still goes (one slot), a real one takes MSM
      {1, MIN, 0, Route::MSM, 2, 3},
  };
  for (const Case& c : cases) {
    const CombineChunk p = combine_chunk(gs, 7, c.g0, c.msm_min, c.budget);
    EXPECT(p.route == c.route && p.g_end == c.g_end && p.terms == c.terms, "combine_chunk(g0 = %zu, min = %zu, budget = %zu) = %s / %zu / %zu", c.g0, c.msm_min,
           c.budget, name(p.route), p.g_end, p.terms);
  }
  // every walk covers each group exactly once and ends at G, whatever the budget
  for (size_t budget : {(size_t)0, (size_t)1296, (size_t)1296 * 7, (size_t)1296 * 12, GB}) {
    size_t g0 = 0, steps = 0;
    while (g0 < 7) {
      const CombineChunk p = combine_chunk(gs, 7, g0, 4, budget);
      EXPECT(p.g_end > g0 && p.g_end <= 7 && p.terms >= 1, "progress at %zu under %zu", g0, budget);
      if (p.route == Route::SEGMENTS) EXPECT(p.terms >= longest_group(gs, g0, p.g_end), "the padding covers the longest group");
      g0 = p.g_end;
      ++steps;
    }
    EXPECT(g0 == 7 && steps <= 7, "walk under %zu", budget);
  }
  // 64 groups of 8 under the default budget: one chunk of 512 slots; a heap array, so that the sanitizer sees a read past G + 1 offsets
  std::vector<uint64_t> even(65);
  for (size_t g = 0; g <= 64; ++g) even[g] = 8 * g;
  const CombineChunk p = combine_chunk(even.data(), 64, 0, MIN, GB);
  EXPECT(p.route == Route::SEGMENTS && p.g_end == 64 && p.terms == 8, "64 x 8");
  EXPECT(groups_ok(even.data(), 64, 512) && longest_group(even.data(), 0, 64) == 8, "64 x 8 offsets");
  // a group of 2^33 terms: nothing wraps at 32 bits
  const uint64_t big[] = {0, (uint64_t)1 << 33};
  const CombineChunk b = combine_chunk(big, 1, 0, MIN, GB);
  EXPECT(b.route == Route::MSM && b.g_end == 1 && b.terms == ((size_t)1 << 33), "2^33");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {
    const OpenLayout l = open_layout(2049, 14, 2);
    const Region r[] = {WORDS(l, gs, 3), WORDS(l, pow, 56), WORDS(l, zs, 56), WORDS(l, f, 16392), WORDS(l, yf, 8)};
    EXPECT(layout_ok("open", r, l.bytes) && l.pow == 24 && l.zs == 472 && l.f == 920 && l.yf == 132056 && l.bytes == 132120, "open: %zu", l.bytes);
    const OpenLayout one = open_layout(1, 1, 1);
    const Region q[] = {WORDS(one, gs, 2), WORDS(one, pow, 4), WORDS(one, zs, 4), WORDS(one, f, 4), WORDS(one, yf, 4)};
    EXPECT(layout_ok("open of one", q, one.bytes) && one.pow == 16 && one.f == 80 && one.yf == 112 && one.bytes == 144, "one: %zu", one.bytes);
    EXPECT(open_layout((size_t)1 << 40, 1, (size_t)1 << 40).bytes == SIZE_MAX, "saturates");
  }
  {
    const CombineLayout l = combine_layout(14, 2);
    const Region r[] = {WORDS(l, gs, 3), WORDS(l, pow, 56)};
    EXPECT(layout_ok("combine", r, l.bytes) && l.pow == 24 && l.bytes == 472 && combine_layout(1, 1).pow == 16 && combine_layout(1, 1).bytes == 48, "combine: %zu", l.bytes);
    EXPECT(combine_layout(SIZE_MAX / 2, 1).bytes == SIZE_MAX && offset_bytes(2) == 24 && offset_bytes(SIZE_MAX / 4) == SIZE_MAX, "saturates");
  }
  {  // a chunk of the combined commitments: (4 n + 8 n + 8 n + w_acc + 8 n_seg) words + 2 n + n_seg bytes.  3 groups of 2 terms, w_acc = 5
    const ChunkLayout l = chunk_layout(6, 3, 5);
    const Region r[] = {WORDS(l, sc, 24), WORDS(l, bases, 48), WORDS(l, prod, 48), WORDS(l, acc, 5), WORDS(l, part, 24), BYTES(l, flags, 6), BYTES(l, prod_inf, 6),
                        BYTES(l, part_inf, 3)};
    EXPECT(layout_ok("chunk", r, l.bytes) && l.bases == 192 && l.prod == 576 && l.acc == 960 && l.part == 1000 && l.flags == 1192 && l.prod_inf == 1198 && l.part_inf == 1204 &&
               l.bytes == (24 + 48 + 48 + 5 + 24) * 8 + 12 + 3, "segments: %zu", l.bytes);
  }
  {  // one group of 5 terms through the multi-scalar multiplication: no words for a segmented sum
    const ChunkLayout l = chunk_layout(5, 1, 0);
    const Region r[] = {WORDS(l, sc, 20), WORDS(l, bases, 40), WORDS(l, prod, 40), WORDS(l, acc, 0), WORDS(l, part, 8), BYTES(l, flags, 5), BYTES(l, prod_inf, 5),
                        BYTES(l, part_inf, 1)};
    EXPECT(layout_ok("chunk msm", r, l.bytes) && l.acc == 800 && l.part == 800 && l.flags == 864 && l.prod_inf == 869 && l.part_inf == 874 && l.bytes == 108 * 8 + 10 + 1,
           "msm: %zu", l.bytes);
    EXPECT(chunk_layout(SIZE_MAX / 4, 1, 0).bytes == SIZE_MAX, "saturates");
  }
  {
    const VerifyLayout l = verify_layout(9);
    const Region r[] = {WORDS(l, cf, 72), WORDS(l, yf, 36), BYTES(l, cf_inf, 9)};
    EXPECT(layout_ok("verify", r, l.bytes) && l.yf == 576 && l.cf_inf == 864 && l.bytes == 880, "verify: %zu", l.bytes);
    const VerifyLayout one = verify_layout(1);
    const Region q[] = {WORDS(one, cf, 8), WORDS(one, yf, 4), BYTES(one, cf_inf, 1)};
    EXPECT(layout_ok("verify of one", q, one.bytes) && one.yf == 64 && one.cf_inf == 96 && one.bytes == 104 && verify_layout(SIZE_MAX / 8).bytes == SIZE_MAX, "one: %zu", one.bytes);
  }
}

int main() {
  groups();
  lincomb_geometry();
  scratch();
  combine_chunks();
  layouts();
  if (fails) { printf("%d of %zu checks failed\n", fails, checked); return 1; }
  printf("OK %zu checks\n", checked);
  return 0;
}
