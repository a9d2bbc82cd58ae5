// CPU-only check of the planner of the batched cell check (sylow_amd/csrc/kzg_cells_plan.hpp): the limits, the route rule, the keys and
// entries of both routes, the keyed multiply-accumulate walked on the host exactly as the kernel walks it -- every (key, column) owned by
// one lane under every slice count, the slices of a group a partition of it, every index into the permutation, the LDS slots and the
// outputs inside its array for groups of 0, 1, 15, 16, 17 and 33 rows, never more than 16 products between two folds -- the Horner chunks
// and their exponents, the grids, and the scratch sums where size_t overflows.  Expected values are written out by hand from the rules in
// the header's comments.  Built with -fsanitize=address,undefined by tests/test_kzg_cells_plan.py: host code only.
#include "../../sylow_amd/csrc/kzg_cells_plan.hpp"
#include "../../include/sylow_hip_kzg_cells.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace kzg_cells_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static const size_t TOP = SIZE_MAX;

static void limits() {
  EXPECT(CELLS_BLOCK == 256 && (1 << CELLS_BLOCK_LOG) == CELLS_BLOCK && CELLS_WAVE == 64 && CELLS_LOG_N_MAX == 27, "constants");
  EXPECT(SYLOW_HIP_KZG_CELLS_LOG_N_MAX == CELLS_LOG_N_MAX, "the header's limit is the plan's");
  EXPECT(logs_ok(0, 0) && logs_ok(7, 6) && logs_ok(27, 0) && logs_ok(0, 27) && logs_ok(13, 14), "the legal corners");
  EXPECT(!logs_ok(28, 0) && !logs_ok(0, 28) && !logs_ok(14, 14) && !logs_ok(-1, 3) && !logs_ok(3, -1) && !logs_ok(INT32_MAX, 1) && !logs_ok(1, INT32_MAX), "the illegal ones");
  EXPECT(max_blocks_ok(-1) && max_blocks_ok(1) && !max_blocks_ok(0), "a cap of no block is refused");
  EXPECT(disjoint_or_empty(0, 8, 8, 8) && !disjoint_or_empty(0, 9, 8, 8) && !disjoint_or_empty(4, 1, 0, 8) && disjoint_or_empty(4, 0, 0, 8), "byte ranges; an empty range overlaps nothing");
  EXPECT(grid(0, -1) == 1 && grid(5, -1) == 5 && grid(5, 2) == 2 && grid(TOP, -1) == CELLS_GRID_CAP && grid(TOP, 1) == 1 && grid(3, INT64_MAX) == 3, "grids");
  EXPECT(blocks_of(0) == 0 && blocks_of(1) == 1 && blocks_of(256) == 1 && blocks_of(257) == 2 && blocks_of(TOP) == TOP / 256 + 1, "blocks of lanes, no wrap");
  EXPECT(vals_bytes(6, 8192) == (size_t)8192 * 64 * 32 && vals_bytes(27, TOP) == SAT && point_bytes(3) == 192 && scalar_bytes(TOP) == SAT && index_bytes(TOP) == SAT, "bytes");
}

static void routes_and_keys() {
  EXPECT(route_ok(-1) && route_ok(0) && route_ok(1) && !route_ok(2), "routes");
  EXPECT(route_of(-1, 7, 127) == ROUTE_ROWS && route_of(-1, 7, 128) == ROUTE_COLUMNS && route_of(-1, 0, 1) == ROUTE_COLUMNS && route_of(0, 0, 99) == ROUTE_ROWS &&
             route_of(1, 7, 1) == ROUTE_COLUMNS,
         "by columns from rows = c on; a pin wins");
  EXPECT(n_keys(ROUTE_COLUMNS, 7, 64) == 192 && n_keys(ROUTE_ROWS, 7, 64) == 64 && n_keys(ROUTE_COLUMNS, 27, TOP) == SAT, "cell keys first, on the column route only");
  EXPECT(entries(ROUTE_COLUMNS, 10) == 20 && entries(ROUTE_ROWS, 10) == 10 && entries(ROUTE_COLUMNS, TOP) == SAT, "two entries per row by columns");
  for (int route = 0; route < 2; ++route) {
    bool ok = true;
    for (size_t e = 0; e < entries(route, 13); ++e) ok = ok && entry_row(e, route, 13) == e % 13;
    EXPECT(ok, "an entry names its row on route %d", route);
  }
  EXPECT(in_range(127, 7) && !in_range(128, 7) && in_range(0, 0) && !in_range(1, 0) && !in_range(UINT64_MAX, 27), "idx < c");
  EXPECT(scan_rounds(0) == 0 && scan_rounds(256) == 1 && scan_rounds(257) == 2, "rounds of the scan");
  EXPECT(root_words(0) == 0 && root_words(7) == 256 && !root_negated(0, 0) && root_negated(1, 1) && root_slot(1, 1) == 0, "the roots");
  for (int log_c = 1; log_c <= 10; ++log_c) {
    bool ok = true;
    for (size_t i = 0; i < elems(log_c); ++i) ok = ok && root_slot(i, log_c) < elems(log_c - 1) && root_slot(i, log_c) == i % elems(log_c - 1);
    EXPECT(ok, "every slot inside the table of c / 2 at log_c = %d", log_c);
  }
}

// the kernel's walk over groups of the given sizes: who stores what, which permutation entries are read, how many products between folds
static void walk(int log_cols, const std::vector<size_t>& sizes, size_t slices) {
  const size_t keys = sizes.size(), cols = elems(log_cols), tiles = mac_tiles(keys, log_cols), items = mac_items(keys, log_cols, slices);
  std::vector<size_t> start(keys + 1, 0);
  for (size_t k = 0; k < keys; ++k) start[k + 1] = start[k] + sizes[k];
  const size_t total = start[keys];
  std::vector<int> stored(slices * keys * cols, 0);
  std::vector<int> read(total * cols, 0);                    // how often (permutation entry, column) entered a product
  bool slots_ok = true, perm_ok = true, flush_ok = true, staged_ok = true;
  const int stage = 1 << mac_stage_log(log_cols);
  for (size_t item = 0; item < items; ++item) {
    const size_t s = mac_slice(item, tiles), tile = mac_tile(item, tiles);
    size_t most = 0;
    for (int t = 0; t < CELLS_BLOCK; ++t) {
      const size_t key = mac_key(tile * CELLS_BLOCK + t, log_cols);
      if (key < keys) {
        const size_t len = sizes[key], span = slice_begin(len, s + 1, slices) - slice_begin(len, s, slices);
        most = span > most ? span : most;
      }
    }
    std::vector<int> pending(CELLS_BLOCK, 0);
    for (size_t base = 0; base < most; base += stage) {
      std::vector<long> slot(CELLS_BLOCK, -1);               // what each LDS slot holds this round
      for (int t = 0; t < CELLS_BLOCK; ++t) {
        const size_t flat = tile * CELLS_BLOCK + t, key = mac_key(flat, log_cols);
        if (key >= keys) continue;
        const size_t g0 = start[key] + slice_begin(sizes[key], s, slices), g1 = start[key] + slice_begin(sizes[key], s + 1, slices);
        const int q = mac_team_lane(t, log_cols), sl = mac_slot(t, log_cols) + q;
        if (q < stage && g0 + base + q < g1) {
          slots_ok = slots_ok && sl >= 0 && sl < mac_slots(log_cols) && mac_slots(log_cols) <= CELLS_BLOCK && slot[sl] == -1;
          perm_ok = perm_ok && g0 + base + q < total;
          slot[sl] = (long)(g0 + base + q);
        }
      }
      for (int t = 0; t < CELLS_BLOCK; ++t) {
        const size_t flat = tile * CELLS_BLOCK + t, key = mac_key(flat, log_cols), col = mac_col(flat, log_cols);
        if (key >= keys) continue;
        const size_t g0 = start[key] + slice_begin(sizes[key], s, slices), g1 = start[key] + slice_begin(sizes[key], s + 1, slices);
        if (g0 + base >= g1) continue;
        const int cnt = g1 - (g0 + base) < (size_t)stage ? (int)(g1 - (g0 + base)) : stage;
        for (int i = 0; i < cnt; ++i) {
          const long e = slot[mac_slot(t, log_cols) + i];
          staged_ok = staged_ok && e == (long)(g0 + base + i);     // the team's slot holds the entry this lane expects
          if (e >= 0 && (size_t)e < total) ++read[(size_t)e * cols + col];
        }
        pending[t] += cnt;
        flush_ok = flush_ok && pending[t] <= MAC_FLUSH;
        if (mac_folds(pending[t], log_cols)) pending[t] = 0;
      }
    }
    for (int t = 0; t < CELLS_BLOCK; ++t) {
      const size_t flat = tile * CELLS_BLOCK + t, key = mac_key(flat, log_cols);
      if (key < keys) ++stored[(s * keys + key) * cols + mac_col(flat, log_cols)];
    }
  }
  bool once = true, all_read = true;
  for (int v : stored) once = once && v == 1;
  for (int v : read) all_read = all_read && v == 1;
  EXPECT(once, "every (slice, key, column) stored once: log_cols %d, %zu keys, %zu slices", log_cols, keys, slices);
  EXPECT(all_read, "every (row of a group, column) in exactly one product: log_cols %d, %zu slices", log_cols, slices);
  EXPECT(slots_ok && perm_ok && staged_ok && flush_ok, "slots %d perm %d staged %d flush %d: log_cols %d, %zu slices", slots_ok, perm_ok, staged_ok, flush_ok, log_cols, slices);
}

static void mac_kernel() {
  EXPECT(MAC_FLUSH == 16 && mac_lds_bytes() == 256 * 40 + 8, "256 slots of a weight and a row number, and the longest slice");
  // {log_cols, lanes of a team, rows of a round, slots}
  const int tm[][4] = {{0, 1, 1, 256}, {1, 2, 2, 256}, {3, 8, 8, 256}, {4, 16, 16, 256}, {6, 64, 16, 64}, {8, 256, 16, 16}, {10, 256, 16, 16}};
  for (const auto& r : tm)
    EXPECT((1 << mac_team_log(r[0])) == r[1] && (1 << mac_stage_log(r[0])) == r[2] && mac_slots(r[0]) == r[3], "teams at log_cols = %d", r[0]);
  EXPECT(mac_tiles(128, 6) == 32 && mac_tiles(1, 0) == 1 && mac_tiles(0, 3) == 0 && mac_tiles(3, 10) == 12 && mac_tiles(TOP, 1) == SAT / 256 + 1, "tiles");
  const std::vector<size_t> sizes = {0, 1, 15, 16, 17, 33, 0, 140};
  for (int log_cols : {0, 1, 2, 3, 4, 6, 8, 9})
    for (size_t slices : {(size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)8, (size_t)64}) walk(log_cols, sizes, slices);
  walk(0, std::vector<size_t>(300, 3), 2);                   // more keys than one tile of single columns
  walk(2, {}, 1);
  for (size_t len : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)33, (size_t)1000003})
    for (size_t slices : {(size_t)1, (size_t)2, (size_t)3, (size_t)7, (size_t)64}) {
      bool ok = slice_begin(len, 0, slices) == 0 && slice_begin(len, slices, slices) == len;
      for (size_t s = 0; s < slices; ++s) {
        const size_t span = slice_begin(len, s + 1, slices) - slice_begin(len, s, slices);
        ok = ok && slice_begin(len, s, slices) <= slice_begin(len, s + 1, slices) && (span == len / slices || span == len / slices + 1);
      }
      EXPECT(ok, "the slices of %zu rows partition them into %zu parts", len, slices);
    }
  // the flagship: 128 keys of 64 columns are 32 tiles; groups of 64 rows are cut in 4; a device full of tiles is not cut; short groups are not cut
  EXPECT(mac_slices(128, 6, 8192) == 4 && mac_slices(128, 6, 65536) == 32 && mac_slices(128, 6, 128) == 1 && mac_slices(0, 0, 5) == 1, "slices of S");
  EXPECT(mac_slices(64, 0, 8192) == 8 && mac_slices(1, 0, 128) == 8 && mac_slices(4, 2, 300) == 4 && mac_slices((size_t)1 << 20, 0, (size_t)1 << 30) == 1, "slices of W");
  EXPECT(mac_slices(1, 0, TOP) == (size_t)MAC_SLICES_MAX && !joins(1) && joins(2), "the cap");
  EXPECT(partial_words(128, 6, 1) == 0 && partial_words(128, 6, 4) == 4 * 4 * 8192 && partial_words(TOP, 6, 2) == SAT, "partials only where a launch joins them");
  EXPECT(s_key_stride(6) == 256 && s_word_stride(6) == 64 && w_key_stride() == 1 && w_word_stride(5) == 5, "[c][4][l] and [4][n_com]");
}

static void horner() {
  // {log_c, lanes of a t, cells of a chunk}
  const size_t hc[][3] = {{0, 1, 1}, {1, 2, 1}, {3, 8, 1}, {4, 16, 1}, {7, 16, 8}, {10, 16, 64}};
  for (const auto& r : hc) EXPECT(((size_t)1 << horner_lanes_log((int)r[0])) == r[1] && horner_chunk((int)r[0]) == r[2], "chunks at log_c = %zu", r[0]);
  for (int log_c : {0, 2, 5, 7})
    for (int log_l : {0, 1, 6}) {
      const size_t c = elems(log_c), l = elems(log_l), n = c * l;
      std::vector<int> seen(c * l, 0);
      bool ok = horner_items(log_c, log_l) == (l << horner_lanes_log(log_c));
      for (size_t item = 0; item < horner_items(log_c, log_l); ++item) {
        const size_t t = horner_t(item, log_c), q = horner_q(item, log_c);
        ok = ok && t < l && horner_g_exp(t, log_c, log_l) == (n - t) % n && horner_join_exp(t, q, log_c, log_l) == ((n - t) % n) * horner_first(q, log_c) % n;
        ok = ok && (item ^ q) == (t << horner_lanes_log(log_c));   // the lanes of a t are adjacent
        for (size_t k = 0; k < horner_chunk(log_c); ++k) ++seen[(horner_first(q, log_c) + k) * l + t];
      }
      for (int v : seen) ok = ok && v == 1;
      EXPECT(ok, "every a_i[t] in one chunk, exponents mod n: (%d, %d)", log_c, log_l);
    }
  EXPECT(horner_join_exp(1, 15, 13, 14) < elems(27) && horner_g_exp(0, 13, 14) == 0, "exponents stay below n");
}

static void scratch() {
  // by columns at (7, 6), 8192 rows, 64 commitments: 256 roots, 2 * 16384 entries, 3 * 192 + 1 key words, W partials 8 * 256, S and a, S partials 4 * 32768
  EXPECT(fold_scratch_words(ROUTE_COLUMNS, 7, 6, 8192, 64) == 256 + 32768 + 577 + 2048 + 65536 + 131072, "by columns: %zu", fold_scratch_words(ROUTE_COLUMNS, 7, 6, 8192, 64));
  // by rows at (7, 6), 16 rows, 4 commitments: 256 roots, 2 * 16 entries, 3 * 4 + 1, no partials, 16 interpolants of 256 words
  EXPECT(fold_scratch_words(ROUTE_ROWS, 7, 6, 16, 4) == 256 + 32 + 13 + 0 + 4096, "by rows: %zu", fold_scratch_words(ROUTE_ROWS, 7, 6, 16, 4));
  EXPECT(fold_scratch_bytes(ROUTE_ROWS, 7, 6, 16, 4) == 8 * fold_scratch_words(ROUTE_ROWS, 7, 6, 16, 4), "bytes");
  EXPECT(fold_scratch_words(ROUTE_COLUMNS, 0, 0, TOP, 1) == SAT && fold_scratch_words(ROUTE_ROWS, 0, 27, TOP / 2, 1) == SAT && fold_scratch_words(ROUTE_ROWS, 0, 0, 1, TOP) == SAT,
         "sums saturate");
  EXPECT(!scratch_ok(fold_scratch_bytes(ROUTE_COLUMNS, 0, 0, TOP, 1)) && !scratch_ok(SAT) && scratch_ok(SAT / 2) && scratch_ok(0), "and are refused");
  EXPECT(terms(TOP, 1) == SAT && terms(3, 4) == 7, "terms");
  // the reduction at l = 4, 3 rows, 2 commitments: W 8, A 16, r and rz 24, 5 terms of 12 words, two points; bytes: 5 flags and 8
  EXPECT(reduce_scratch_words(2, 3, 2) == 8 + 16 + 24 + 60 + 16 && reduce_scratch_bytes(2, 3, 2) == 8 * 124 + 13, "the reduction: %zu", reduce_scratch_words(2, 3, 2));
  EXPECT(reduce_scratch_bytes(2, TOP, 2) == SAT && reduce_scratch_bytes(2, 2, TOP) == SAT && reduce_scratch_bytes(2, 0, 0) == 8 * 32 + 8, "saturated, and empty");
  EXPECT(verify_scratch_bytes() == 8 * (16 + 16 + 32 + 1), "F, P, two pairs, one word of flags");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // by columns, every region there: 256 roots; 16384 entries; 192 keys; W in 8 slices; S, its transform, S in 4 slices
    const FoldLayout l = fold_layout(ROUTE_COLUMNS, 7, 6, 8192, 64);
    const Region r[] = {WORDS(l, roots, 256), WORDS(l, keys, 16384), WORDS(l, perm, 16384), WORDS(l, cnt, 192), WORDS(l, start, 193), WORDS(l, next, 192),
                        WORDS(l, wpart, 2048), WORDS(l, body, 32768), WORDS(l, a, 32768), WORDS(l, spart, 131072)};
    EXPECT(layout_ok("fold by columns", r, l.bytes) && l.keys == 2048 && l.perm == 133120 && l.cnt == 264192 && l.start == 265728 && l.next == 267272, "groups: %zu", l.next);
    EXPECT(l.wpart == 268808 && l.body == 285192 && l.a == 547336 && l.spart == 809480 && l.bytes == 1858056, "by columns: %zu", l.bytes);
  }
  {  // by rows: the interpolants [16][4][64] are the body, and nothing is behind them
    const FoldLayout l = fold_layout(ROUTE_ROWS, 7, 6, 16, 4);
    const Region r[] = {WORDS(l, roots, 256), WORDS(l, keys, 16), WORDS(l, perm, 16), WORDS(l, cnt, 4), WORDS(l, start, 5), WORDS(l, next, 4), WORDS(l, wpart, 0),
                        WORDS(l, body, 4096), WORDS(l, a, 0), WORDS(l, spart, 0)};
    EXPECT(layout_ok("fold by rows", r, l.bytes) && l.keys == 2048 && l.cnt == 2304 && l.start == 2336 && l.next == 2376 && l.body == 2408 && l.bytes == 35176, "by rows: %zu", l.bytes);
  }
  {  // by columns, small: c = 4, l = 2, 3 rows, 2 commitments, no launch joins slices
    const FoldLayout l = fold_layout(ROUTE_COLUMNS, 2, 1, 3, 2);
    const Region r[] = {WORDS(l, roots, 8), WORDS(l, keys, 6), WORDS(l, perm, 6), WORDS(l, cnt, 6), WORDS(l, start, 7), WORDS(l, next, 6), WORDS(l, wpart, 0),
                        WORDS(l, body, 32), WORDS(l, a, 32), WORDS(l, spart, 0)};
    EXPECT(layout_ok("fold small", r, l.bytes) && l.keys == 64 && l.start == 208 && l.next == 264 && l.body == 312 && l.a == 568 && l.bytes == 824, "small: %zu", l.bytes);
  }
  {  // c = 1, l = 1, one row, no commitment: no roots and no keys
    const FoldLayout l = fold_layout(ROUTE_ROWS, 0, 0, 1, 0);
    const Region r[] = {WORDS(l, roots, 0), WORDS(l, keys, 1), WORDS(l, perm, 1), WORDS(l, cnt, 0), WORDS(l, start, 1), WORDS(l, next, 0), WORDS(l, wpart, 0),
                        WORDS(l, body, 4), WORDS(l, a, 0), WORDS(l, spart, 0)};
    EXPECT(layout_ok("fold of one", r, l.bytes) && l.perm == 8 && l.start == 16 && l.body == 24 && l.bytes == 56, "one row: %zu", l.bytes);
  }
  EXPECT(fold_layout(ROUTE_COLUMNS, 0, 0, TOP, 1).bytes == SAT && fold_layout(ROUTE_ROWS, 0, 0, 1, TOP).bytes == SAT, "saturate");
  {  // l = 4, 3 rows, 2 commitments: 5 flags of the bases, one each of the two points, in 5 + 8 bytes
    const ReduceLayout l = reduce_layout(2, 3, 2);
    const Region r[] = {WORDS(l, w, 8), WORDS(l, a, 16), WORDS(l, r, 12), WORDS(l, rz, 12), WORDS(l, sc, 20), WORDS(l, bases, 40), WORDS(l, m1, 8), WORDS(l, at, 8),
                        BYTES(l, binf, 5), BYTES(l, m1inf, 1), BYTES(l, atinf, 1)};
    EXPECT(layout_ok("reduce", r, l.bytes) && l.a == 64 && l.r == 192 && l.sc == 384 && l.bases == 544 && l.m1 == 864 && l.binf == 992 && l.m1inf == 997 && l.atinf == 998 &&
               l.bytes == 1005, "reduce: %zu", l.bytes);
  }
  {  // no row and no commitment
    const ReduceLayout l = reduce_layout(2, 0, 0);
    const Region r[] = {WORDS(l, w, 0), WORDS(l, a, 16), WORDS(l, r, 0), WORDS(l, rz, 0), WORDS(l, sc, 0), WORDS(l, bases, 0), WORDS(l, m1, 8), WORDS(l, at, 8),
                        BYTES(l, binf, 0), BYTES(l, m1inf, 1), BYTES(l, atinf, 1)};
    EXPECT(layout_ok("reduce of none", r, l.bytes) && l.a == 0 && l.m1 == 128 && l.binf == 256 && l.atinf == 257 && l.bytes == 264, "empty: %zu", l.bytes);
  }
  EXPECT(reduce_layout(2, TOP, 2).bytes == SAT && reduce_layout(2, 2, TOP).bytes == SAT, "saturate");
  {
    const VerifyLayout l = verify_layout();
    const Region r[] = {WORDS(l, f, 8), WORDS(l, p, 8), WORDS(l, pxy, 16), WORDS(l, qxy, 32), BYTES(l, finf, 1), BYTES(l, pinf_one, 1), BYTES(l, pinf, 2),
                        BYTES(l, qinf, 2), BYTES(l, flag, 1), BYTES(l, one, 1)};
    EXPECT(layout_ok("verify", r, l.bytes) && l.p == 64 && l.pxy == 128 && l.qxy == 256 && l.finf == 512 && l.pinf == 514 && l.qinf == 516 && l.flag == 518 && l.one == 519 &&
               l.bytes == 520, "verify: %zu", l.bytes);
  }
}

int main() {
  limits();
  routes_and_keys();
  mac_kernel();
  horner();
  scratch();
  layouts();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
