// CPU-only check of the Poseidon planner (sylow_amd/csrc/poseidon_plan.hpp): widths and depths, the parameter table, lane groups, tiles and
// grids, the levels of a tree inside nodes_out (they tile [0, n - 1) exactly for depth 1 .. 28), the route choice and the saturating sizes.
// Every expected value below is written out by hand from the rules in the header's comments (a block of 256 lanes, a group of the next
// power of two >= t lanes, a grid of at most 2^20 blocks, an element of 4 words); nothing on the expected side is computed from the header.
// Built with -fsanitize=address,undefined by tests/test_poseidon_plan.py: host code only.
#include "../../sylow_amd/csrc/poseidon_plan.hpp"

#include <cstdint>
#include <cstdio>

using namespace poseidon_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void widths_and_tables() {
  EXPECT(T_MIN == 2 && T_MAX == 17 && DEPTH_MIN == 1 && DEPTH_MAX == 28 && POS_BLOCK == 256 && POS_WAVE == 64 && MERKLE_T == 3 && FULL_HALF == 4, "constants");
  EXPECT(!width_ok(1) && width_ok(2) && width_ok(17) && !width_ok(18) && !width_ok(0) && !width_ok(-3), "width_ok");
  EXPECT(!inputs_ok(0) && inputs_ok(1) && inputs_ok(16) && !inputs_ok(17), "inputs_ok");
  EXPECT(!depth_ok(0) && depth_ok(1) && depth_ok(28) && !depth_ok(29) && !depth_ok(-1), "depth_ok");
  const int rp[16] = {56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68};
  for (int t = 2; t <= 17; ++t) {
    EXPECT(partial_rounds(t) == rp[t - 2] && rounds(t) == rp[t - 2] + 8, "rounds(%d)", t);
    EXPECT(matrix_elem(t) == (size_t)(rp[t - 2] + 8) * t && table_elems(t) == (size_t)(rp[t - 2] + 8) * t + (size_t)t * t, "table(%d)", t);
    EXPECT(table_words(t) == 4 * table_elems(t) && table_bytes(t) == 32 * table_elems(t), "table words(%d)", t);
  }
  EXPECT(table_words(3) == 816 && table_words(2) == 528 && table_words(17) == 6324, "three tables by hand");
}

static void groups_and_grids() {
  // {t, lanes of a group, groups of a block}
  const int g[][3] = {{2, 2, 128}, {3, 4, 64}, {4, 4, 64}, {5, 8, 32}, {8, 8, 32}, {9, 16, 16}, {16, 16, 16}, {17, 32, 8}};
  for (const auto& c : g) EXPECT(group_lanes(c[0]) == c[1] && groups_per_block(c[0]) == c[2], "group(%d) = %d, %d", c[0], group_lanes(c[0]), groups_per_block(c[0]));
  for (int t = 2; t <= 17; ++t) {
    const int G = group_lanes(t);
    EXPECT(G >= t && G / 2 < t && (G & (G - 1)) == 0 && POS_WAVE % G == 0, "a group of %d is the next power of two and sits inside a wavefront", t);
  }
  // {t, items, route, tiles}
  const size_t tl[][4] = {{3, 0, 0, 0},   {3, 1, 0, 1},   {3, 256, 0, 1}, {3, 257, 0, 2}, {3, 769, 0, 4},  {3, 1, 1, 1},    {3, 64, 1, 1},  {3, 65, 1, 2},
                          {3, 769, 1, 13}, {17, 8, 1, 1}, {17, 9, 1, 2},  {2, 128, 1, 1}, {2, 129, 1, 2},  {5, 32, 1, 1},   {5, 33, 1, 2},  {9, 17, 1, 2}};
  for (const auto& c : tl) EXPECT(tiles((int)c[0], c[1], (int)c[2]) == c[3], "tiles(%zu, %zu, %zu) = %zu", c[0], c[1], c[2], tiles((int)c[0], c[1], (int)c[2]));
  EXPECT(grid(0, -1) == 1 && grid(1, -1) == 1 && grid(13, -1) == 13 && grid(13, 2) == 2 && grid(13, 13) == 13 && grid(13, 99) == 13, "grid");
  EXPECT(grid((size_t)1 << 20, -1) == (size_t)1 << 20 && grid(((size_t)1 << 20) + 1, -1) == (size_t)1 << 20 && grid((size_t)1 << 40, 1ll << 30) == (size_t)1 << 20, "the cap");
  EXPECT(max_blocks_ok(-1) && max_blocks_ok(1) && !max_blocks_ok(0), "the pin");
}

static void levels() {
  EXPECT(level_offset(3, 1) == 0 && level_offset(3, 2) == 4 && level_offset(3, 3) == 6 && level_nodes(3, 1) == 4 && level_nodes(3, 3) == 1 && node_count(3) == 7, "depth 3 by hand");
  EXPECT(level_offset(1, 1) == 0 && level_nodes(1, 1) == 1 && node_count(1) == 0 + 1, "depth 1: the root alone");
  EXPECT(level_offset(10, 10) == 1022 && level_offset(10, 9) == 1020 && level_offset(10, 1) == 0 && level_offset(10, 2) == 512, "depth 10 by hand");
  for (int depth = 1; depth <= 28; ++depth) {
    size_t at = 0, n = (size_t)1 << depth;
    for (int k = 1; k <= depth; ++k) {
      EXPECT(level_offset(depth, k) == at, "level %d of depth %d starts where level %d ended", k, depth, k - 1);
      EXPECT(level_nodes(depth, k) == n >> k, "level %d of depth %d has n / 2^k nodes", k, depth);
      at += n >> k;
    }
    EXPECT(at == n - 1 && node_count(depth) == n - 1 && level_offset(depth, depth) == n - 2, "the levels of depth %d tile [0, n - 1) and the root is last", depth);
  }
  EXPECT(level_items(10, 1, 3) == 1536 && level_items(10, 10, 3) == 3 && level_items(28, 1, (size_t)-1) == SAT, "items of a level, saturated");
}

static void routes() {
  EXPECT(ROUTE_NARROW == 0 && ROUTE_WIDE == 1 && route_ok(-1) && route_ok(-9) && route_ok(0) && route_ok(1) && !route_ok(2), "route_ok");
  EXPECT(NARROW_T_MAX >= MERKLE_T && NARROW_T_MAX <= T_MAX, "the trees have both routes");
  for (int t = 2; t <= 17; ++t) {
    EXPECT(narrow_ok(t) == (t <= NARROW_T_MAX), "narrow_ok(%d)", t);
    if (!narrow_ok(t)) {
      EXPECT(choose_route(t, 1, 0, -1) == ROUTE_WIDE && choose_route(t, (size_t)1 << 30, -1, 0) == ROUTE_WIDE, "a width past the narrow limit runs wide at every n, whatever the pin");
      continue;
    }
    EXPECT(choose_route(t, 1, 0, -1) == ROUTE_NARROW && choose_route(t, (size_t)1 << 30, 1, -1) == ROUTE_WIDE, "a pin holds (%d)", t);
    const size_t d = wide_max_default(t);
    EXPECT(choose_route(t, d, -1, -1) == ROUTE_WIDE && choose_route(t, d + 1, -1, -1) == ROUTE_NARROW, "the default seam of %d at %zu", t, d);
    EXPECT(choose_route(t, 1, -1, 0) == ROUTE_NARROW && choose_route(t, 4, -1, 4) == ROUTE_WIDE && choose_route(t, 5, -1, 4) == ROUTE_NARROW, "wide_max 0 and 4");
    EXPECT(choose_route(t, (size_t)1 << 20, -1, 1 << 20) == ROUTE_WIDE && choose_route(t, ((size_t)1 << 20) + 1, -1, 1 << 20) == ROUTE_NARROW, "wide_max 2^20");
  }
}

static void sizes() {
  EXPECT(fr_bytes(1) == 32 && fr_bytes(0) == 0 && state_bytes(3, 5) == 480 && leaves_bytes(3, 2) == 512 && nodes_bytes(3, 2) == 448 && path_bytes(20, 3) == 1920, "by hand");
  EXPECT(index_bytes(7) == 56 && n_roots_ok(1, 9) && n_roots_ok(9, 9) && !n_roots_ok(2, 9) && !n_roots_ok(0, 9) && n_roots_ok(1, 1), "indices and roots");
  const size_t big = (size_t)1 << 60;
  EXPECT(fr_bytes(big) == SAT && state_bytes(17, big) == SAT && leaves_bytes(28, (size_t)1 << 32) == SAT && nodes_bytes(28, (size_t)1 << 32) == SAT, "saturated");
  EXPECT(path_bytes(28, big) == SAT && index_bytes((size_t)-1) == SAT && leaves_bytes(28, 1) == (size_t)1 << 33, "saturated paths; the largest tree fits");
}

int main() {
  widths_and_tables();
  groups_and_grids();
  levels();
  routes();
  sizes();
  if (fails) { printf("%d of %zu checks failed\n", fails, checked); return 1; }
  printf("OK %zu checks\n", checked);
  return 0;
}
