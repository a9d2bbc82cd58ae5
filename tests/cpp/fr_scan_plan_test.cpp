// CPU-only check of the planner of the scans over Fr and of PLONK's permutation grand product (sylow_amd/csrc/fr_scan_plan.hpp).  Every
// expected value is written out by hand from the rules in the header's comments (a lane owns 8 elements, a block 256 lanes, a chunk 2048;
// phase 2 walks a row's chunk totals a tile at a time; phase 3 takes the chunks after the first; 32 bytes per total and a byte per item for
// the ratio scan).  The walks are walked as the kernels walk them.  Built with -fsanitize=address,undefined by tests/test_fr_scan_plan.py:
// host code only.
#include "../../sylow_amd/csrc/fr_scan_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace fr_scan_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static void constants_and_pins() {
  EXPECT(SCAN_BLOCK == 256 && SCAN_LANE_ELEMS == 8 && SCAN_CHUNK == 2048 && SCAN_TOTALS_TILE_MAX == 256 && SCAN_TOTALS_TILE_DEFAULT == 256, "constants");
  EXPECT(PLONK_WIRES_MAX == 32 && PLONK_LOG_N_MAX == 28 && OP_SUM == 0 && OP_PRODUCT == 1 && STATUS_ZERO_DEN == 1 && STATUS_NOT_CLOSED == 2, "constants");
  EXPECT(op_ok(0) && op_ok(1) && !op_ok(2) && !op_ok(-1) && flag_ok(0) && flag_ok(1) && !flag_ok(2) && !flag_ok(-1), "op and exclusive");
  // the pins refused: max_blocks = 0; totals_tile = 0 and above the maximum
  EXPECT(!max_blocks_ok(0) && max_blocks_ok(-1) && max_blocks_ok(1) && max_blocks_ok(1ll << 40), "max_blocks");
  EXPECT(!tile_ok(0) && tile_ok(-1) && tile_ok(-7) && tile_ok(1) && tile_ok(2) && tile_ok(256) && !tile_ok(257) && !tile_ok(1ll << 33), "totals_tile");
  EXPECT(tile_of(-1) == 256 && tile_of(1) == 1 && tile_of(2) == 2 && tile_of(256) == 256, "tile_of");
  EXPECT(plonk_ok(0, 1) && plonk_ok(28, 32) && !plonk_ok(29, 1) && !plonk_ok(-1, 1) && !plonk_ok(3, 0) && !plonk_ok(3, 33) && !plonk_ok(3, -1), "log_n and W");
  EXPECT(grid(10, -1) == 10 && grid(0, -1) == 1 && grid(1048577, -1) == 1048576 && grid(10, 1) == 1 && grid(10, 3) == 3 && grid(2, 3) == 2 && grid(5, 1ll << 40) == 5, "grid");
}

// every element of a row belongs to one lane of one item, below the lane's live count; tail chunks have ceil(k / 8) live lanes
static void items_and_live_lanes() {
  const size_t ch[][2] = {{1, 1}, {7, 1}, {8, 1}, {9, 1}, {2047, 1}, {2048, 1}, {2049, 2}, {6153, 4}, {10241, 6}, {526337, 258}, {(size_t)1 << 28, 131072}};
  for (const auto& c : ch) EXPECT(chunks(c[0]) == c[1], "chunks(%zu) = %zu", c[0], chunks(c[0]));
  EXPECT(items(6153, 3) == 12 && items(1, 5) == 5 && items(2049, 0) == 0 && items((size_t)1 << 28, 64) == 8388608 && items(SIZE_MAX, (size_t)1 << 20) == SIZE_MAX, "items");
  EXPECT(item_row(7, 4) == 1 && item_chunk(7, 4) == 3 && item_row(0, 4) == 0 && item_chunk(4, 4) == 0 && item_row(11, 4) == 2, "(row, chunk)");
  EXPECT(lane_base(0, 0) == 0 && lane_base(0, 1) == 8 && lane_base(0, 255) == 2040 && lane_base(1, 0) == 2048 && lane_base(131071, 255) == ((size_t)1 << 28) - 8, "lane_base");
  struct Live { size_t n, c; int live; };
  const Live lv[] = {{1, 0, 1}, {7, 0, 1}, {8, 0, 1}, {9, 0, 2}, {2047, 0, 256}, {2048, 0, 256}, {2049, 0, 256}, {2049, 1, 1}, {6153, 2, 256}, {6153, 3, 2}, {10241, 5, 1}};
  for (const Live& l : lv) EXPECT(live_lanes(l.n, l.c) == l.live, "live_lanes(%zu, %zu) = %d", l.n, l.c, live_lanes(l.n, l.c));
  EXPECT(scan_steps(1) == 0 && scan_steps(2) == 1 && scan_steps(3) == 2 && scan_steps(255) == 8 && scan_steps(256) == 8, "scan_steps");
  for (const size_t len : {(size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)2047, (size_t)2048, (size_t)2049, (size_t)6153}) {
    std::vector<int> seen(len, 0);
    for (size_t c = 0; c < chunks(len); ++c) {
      const int live = live_lanes(len, c);
      EXPECT(live >= 1 && live <= SCAN_BLOCK, "live");
      for (int t = 0; t < SCAN_BLOCK; ++t) {
        bool owns = false;
        for (int i = 0; i < SCAN_LANE_ELEMS; ++i)
          if (lane_base(c, t) + (size_t)i < len) { ++seen[lane_base(c, t) + (size_t)i]; owns = true; }
        EXPECT(owns == (t < live), "lane %d of chunk %zu of %zu", t, c, len);
      }
    }
    bool once = true;
    for (const int s : seen) once = once && s == 1;
    EXPECT(once, "every element of %zu once", len);
  }
}

// phase 2 as k_scan_totals walks it: every total visited once, in order, by a lane below the step's count, for 0, 1, tile - 1, tile and
// tile + 1 chunks under totals_tile = 1, 2, the default and the maximum
static void tile_walk() {
  for (const long long pin : {1ll, 2ll, -1ll, (long long)SCAN_TOTALS_TILE_MAX}) {
    const int tile = tile_of(pin);
    for (const size_t n_chunks : {(size_t)0, (size_t)1, (size_t)(tile - 1), (size_t)tile, (size_t)(tile + 1), (size_t)(3 * tile + 1)}) {
      std::vector<int> seen(n_chunks, 0);
      size_t next = 0, steps = 0;
      for (size_t step = 0; step < tile_steps(n_chunks, tile); ++step, ++steps) {
        const size_t first = tile_first(step, tile);
        const int cnt = tile_count(n_chunks, first, tile);
        EXPECT(first < n_chunks && first == next && cnt >= 1 && cnt <= tile && cnt <= SCAN_BLOCK, "step %zu of %zu chunks at tile %d", step, n_chunks, tile);
        for (int t = 0; t < cnt; ++t) ++seen[first + (size_t)t];
        next = first + (size_t)cnt;
      }
      bool once = next == n_chunks;
      for (const int s : seen) once = once && s == 1;
      EXPECT(once && steps == (n_chunks + (size_t)tile - 1) / (size_t)tile, "%zu chunks at tile %d: every total once in %zu steps", n_chunks, tile, steps);
    }
  }
  EXPECT(tile_steps(131072, 256) == 512 && tile_steps(131072, 1) == 131072 && tile_steps(6, 2) == 3 && tile_steps(6, 256) == 1, "steps");
  EXPECT(totals_grid(3, -1) == 3 && totals_grid(3, 1) == 1 && totals_grid(64, 16) == 16, "a block per row");
}

// the one-chunk route and phase 3's items: the chunks after the first of every row, once, and the elements of a chunk once
static void routes_and_apply() {
  EXPECT(!upper_phases(1) && !upper_phases(2048) && upper_phases(2049) && upper_phases((size_t)1 << 28), "a row of one chunk needs only phase 1");
  EXPECT(apply_items(2048, 9) == 0 && apply_items(2049, 9) == 9 && apply_items(6153, 3) == 9 && apply_items(10241, 1) == 5, "apply items");
  for (const size_t len : {(size_t)2049, (size_t)6153, (size_t)10241}) {
    const size_t m = 3, n_chunks = chunks(len);
    std::vector<int> seen(m * len, 0);
    for (size_t it = 0; it < apply_items(len, m); ++it) {
      const size_t j = apply_row(it, n_chunks), c = apply_chunk(it, n_chunks);
      EXPECT(j < m && c >= 1 && c < n_chunks, "item %zu", it);
      for (int i = 0; i < SCAN_LANE_ELEMS; ++i)
        for (int t = 0; t < SCAN_BLOCK; ++t)
          if (apply_elem(c, i, t) < len) ++seen[j * len + apply_elem(c, i, t)];
    }
    bool ok = true;
    for (size_t j = 0; j < m; ++j)
      for (size_t k = 0; k < len; ++k) ok = ok && seen[j * len + k] == (k >= SCAN_CHUNK ? 1 : 0);
    EXPECT(ok, "every element past chunk 0 of %zu once", len);
  }
}

static void bytes_and_scratch() {
  EXPECT(rows_bytes(5, 3) == 480 && rows_bytes(2049, 1) == 65568 && rows_bytes((size_t)1 << 28, 64) == ((size_t)1 << 39) && scalars_bytes(3) == 96, "bytes");
  EXPECT(rows_bytes(SIZE_MAX / 16, 1) == SIZE_MAX && rows_bytes((size_t)1 << 40, (size_t)1 << 40) == SIZE_MAX && scalars_bytes(SIZE_MAX / 2) == SIZE_MAX, "saturates");
  // nothing for one chunk; 32 bytes per item, and a byte per item more for the ratio scan
  EXPECT(scan_scratch_bytes(2048, 100, false) == 0 && scan_scratch_bytes(2048, 100, true) == 0 && totals_words(2048, 100) == 0, "one chunk leases nothing");
  EXPECT(scan_scratch_bytes(2049, 1, false) == 64 && scan_scratch_bytes(2049, 1, true) == 66 && scan_scratch_bytes(6153, 3, true) == 12 * 33, "scratch");
  EXPECT(totals_words(6153, 3) == 48 && scan_scratch_bytes((size_t)1 << 28, 1, false) == 131072 * 32, "scratch");
  EXPECT(scan_scratch_bytes(SIZE_MAX, (size_t)1 << 20, false) == SIZE_MAX && scan_scratch_bytes((size_t)1 << 60, (size_t)1 << 60, true) == SIZE_MAX, "saturates");
  EXPECT(scratch_ok(0) && scratch_ok(SIZE_MAX / 2) && !scratch_ok(SIZE_MAX) && !scratch_ok(SIZE_MAX / 2 + 1), "refused before the lease");
  // PLONK: the table of n / 2 roots (none at n = 1), then num and den [m][4][n]
  EXPECT(root_words(0) == 0 && root_words(1) == 4 && root_words(3) == 16 && root_words(28) == ((size_t)1 << 29), "roots");
  EXPECT(identity_items(0, 1) == 1 && identity_items(3, 3) == 1 && identity_items(8, 1) == 1 && identity_items(8, 3) == 3 && identity_items(3, 32) == 1 &&
             identity_items(4, 32) == 2 && identity_items(4, 17) == 2, "identity tiles");
  EXPECT(identity_bytes(3, 2) == 512 && identity_scratch_bytes(0) == 0 && identity_scratch_bytes(3) == 128, "identity bytes");
  EXPECT(terms_tiles(0) == 1 && terms_tiles(8) == 1 && terms_tiles(9) == 2 && terms_items(9, 3) == 6 && terms_items(12, 2) == 32, "terms items");
  EXPECT(wires_bytes(3, 2, 3) == 1536 && terms_words(3, 2) == 64, "wires");
  EXPECT(permutation_scratch_bytes(0, 1) == 64 && permutation_scratch_bytes(3, 2) == (16 + 128) * 8 && permutation_scratch_bytes(12, 2) == (8192 + 65536) * 8, "scratch");
  EXPECT(permutation_scratch_bytes(28, (size_t)1 << 40) == SIZE_MAX && wires_bytes(28, 32, (size_t)1 << 40) == SIZE_MAX, "saturates");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand

static void layouts() {
  {  // 4 chunks x 3 rows = 12 items: totals [4][12], then a flag byte per item
    const ScanLayout l = scan_layout(6153, 3, true);
    const Region r[] = {WORDS(l, totals, 48), BYTES(l, zflag, 12)};
    EXPECT(layout_ok("ratio scan", r, l.bytes) && l.totals == 0 && l.zflag == 384 && l.bytes == 396, "ratio scan: %zu %zu", l.zflag, l.bytes);
  }
  {
    const ScanLayout l = scan_layout(6153, 3, false);
    const Region r[] = {WORDS(l, totals, 48), BYTES(l, zflag, 0)};
    EXPECT(layout_ok("plain scan", r, l.bytes) && l.zflag == 384 && l.bytes == 384, "plain scan: %zu", l.bytes);
  }
  {  // one chunk: nothing
    const ScanLayout l = scan_layout(2048, 100, true);
    const Region r[] = {WORDS(l, totals, 0), BYTES(l, zflag, 0)};
    EXPECT(layout_ok("one chunk", r, l.bytes) && l.bytes == 0, "one chunk: %zu", l.bytes);
  }
  EXPECT(scan_layout(SIZE_MAX, (size_t)1 << 20, true).bytes == SIZE_MAX, "saturates");
  {  // n = 8, m = 2: the 4 roots, then num and den [2][4][8]
    const PermutationLayout l = permutation_layout(3, 2);
    const Region r[] = {WORDS(l, roots, 16), WORDS(l, num, 64), WORDS(l, den, 64)};
    EXPECT(layout_ok("permutation", r, l.bytes) && l.num == 128 && l.den == 640 && l.bytes == 1152, "permutation: %zu %zu %zu", l.num, l.den, l.bytes);
  }
  {  // n = 1: no roots
    const PermutationLayout l = permutation_layout(0, 1);
    const Region r[] = {WORDS(l, roots, 0), WORDS(l, num, 4), WORDS(l, den, 4)};
    EXPECT(layout_ok("permutation n = 1", r, l.bytes) && l.num == 0 && l.den == 32 && l.bytes == 64, "n = 1: %zu", l.bytes);
  }
  EXPECT(permutation_layout(28, (size_t)1 << 40).bytes == SIZE_MAX, "saturates");
}

int main() {
  constants_and_pins();
  items_and_live_lanes();
  tile_walk();
  routes_and_apply();
  bytes_and_scratch();
  layouts();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
