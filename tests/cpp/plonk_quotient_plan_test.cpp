// CPU-only check of the planner of PLONK's quotient polynomial (sylow_amd/csrc/plonk_quotient_plan.hpp).  Every expected value is written out
// by hand from the rules in the header's comments (2 W + 3 rows of N points and E inverses; a lane per point, 256 points per tile; the
// degree bound D and the tail from D - n + 1 on; W + 1 columns per instance, one more with public inputs; a chunk leases the shift, the
// roots, W + 4 constants per instance and two buffers, and the forward transform leases its table and one buffer more).  The walks are walked
// as the kernels walk them.  Built with -fsanitize=address,undefined by tests/test_plonk_quotient_plan.py: host code only.
#include "../../sylow_amd/csrc/plonk_quotient_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace plonk_quotient_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static void constants_and_pins() {
  EXPECT(PQ_BLOCK == 256 && PQ_FLUSH == 16 && PQ_COSET_SHIFT == 5 && PQ_WIRES_MIN == 2 && PQ_WIRES_MAX == 32 && PQ_LOG_MAX == 28 && STATUS_NOT_DIVISIBLE == 1, "constants");
  EXPECT(PQ_SHIFT_WORDS == 4 && PQ_CHALLENGE_SLOTS == 4 && FR_WORDS == 4, "constants");
  EXPECT(dims_ok(0, 0, 2) && dims_ok(26, 2, 32) && dims_ok(0, 28, 3) && dims_ok(28, 0, 3), "the legal corners");
  EXPECT(!dims_ok(27, 2, 3) && !dims_ok(-1, 2, 3) && !dims_ok(3, -1, 3) && !dims_ok(3, 2, 1) && !dims_ok(3, 2, 33) && !dims_ok(3, 2, 0) && !dims_ok(29, 0, 3) &&
             !dims_ok(0, 29, 3) && !dims_ok(2147483647, 2147483647, 3),
         "refused");
  // the pin refused: max_blocks = 0
  EXPECT(!max_blocks_ok(0) && max_blocks_ok(-1) && max_blocks_ok(1) && max_blocks_ok(1ll << 40), "max_blocks");
  EXPECT(grid(10, -1) == 10 && grid(0, -1) == 1 && grid(1048577, -1) == 1048576 && grid(10, 1) == 1 && grid(10, 3) == 3 && grid(2, 3) == 2 && grid(5, 1ll << 40) == 5, "grid");
}

static void table_layout() {
  EXPECT(table_rows(2) == 7 && table_rows(3) == 9 && table_rows(32) == 67, "2 W + 3 rows");
  EXPECT(row_selector(0) == 0 && row_selector(2) == 2 && row_qm(3) == 3 && row_qc(3) == 4 && row_sigma(3, 0) == 5 && row_sigma(3, 2) == 7 && row_l1(3) == 8, "W = 3");
  EXPECT(row_l1(2) == table_rows(2) - 1 && row_sigma(32, 31) == 65 && row_l1(32) == 66, "the last row is L_1");
  EXPECT(row_words(3, 2) == 128 && row_words(0, 0) == 4 && row_words(26, 2) == ((size_t)1 << 30), "4 N words");
  EXPECT(zinv_offset_words(3, 2, 3) == 9 * 128 && table_words(3, 2, 3) == 9 * 128 + 16 && table_bytes(3, 2, 3) == (9 * 128 + 16) * 8, "the tail behind the rows");
  EXPECT(table_words(0, 0, 2) == 7 * 4 + 4 && table_words(0, 2, 2) == 7 * 16 + 16, "n = 1");
  EXPECT(selectors_bytes(3, 3) == 5 * 4 * 8 * 8 && sigma_bytes(3, 3) == 3 * 4 * 8 * 8, "the caller's arrays");
  // prepare: coefficients [9][4][8], L_1 [4][8], padded [9][4][32], 16 roots of 4 words, the shift
  EXPECT(prepare_coeff_words(3, 3) == 288 && prepare_scratch_words(3, 2, 3) == 288 + 32 + 1152 + 64 + 4 && prepare_scratch_bytes(3, 2, 3) == 1540 * 8, "prepare");
  EXPECT(prepare_scratch_words(0, 0, 2) == 28 + 4 + 28 + 0 + 4, "n = N = 1: no roots");
}

// every point of every instance belongs to one lane of one item; the tail tile of a short domain has fewer live lanes
static void items_and_tail_tiles() {
  EXPECT(tiles(0, 0) == 1 && tiles(3, 2) == 1 && tiles(6, 2) == 1 && tiles(7, 2) == 2 && tiles(9, 2) == 8 && tiles(26, 2) == ((size_t)1 << 20), "tiles");
  EXPECT(items(9, 2, 3) == 24 && items(3, 2, 5) == 5 && items(9, 2, 0) == 0 && items(26, 2, SIZE_MAX) == SIZE_MAX, "items");
  EXPECT(item_instance(17, 8) == 2 && item_tile(17, 8) == 1 && item_instance(7, 8) == 0 && item_tile(8, 8) == 0 && point(3, 5) == 773 && point(0, 255) == 255, "(instance, tile)");
  for (const int lb : {0, 2, 5, 8, 9, 11}) {
    const int log_e = lb >= 2 ? 2 : 0, log_n = lb - log_e;
    const size_t N = elems(lb), m = 3, nt = tiles(log_n, log_e);
    std::vector<int> seen(m * N, 0);
    for (const long long pin : {-1ll, 1ll, 5ll}) {
      const size_t g = grid(items(log_n, log_e, m), pin);
      for (size_t block = 0; block < g; ++block)
        for (size_t it = block; it < items(log_n, log_e, m); it += g)
          for (int t = 0; t < PQ_BLOCK; ++t) {
            const size_t s = item_instance(it, nt), i = point(item_tile(it, nt), t);
            EXPECT(s < m, "instance");
            if (i < N) ++seen[s * N + i];
          }
    }
    bool once = true;
    for (const int v : seen) once = once && v == 3;
    EXPECT(once, "every point of 2^%d once per walk", lb);
  }
  // z(w_n X): E points on, wrapped inside N; the inverse of X^n - 1 by i mod E
  EXPECT(next_point(0, 3, 2) == 4 && next_point(27, 3, 2) == 31 && next_point(28, 3, 2) == 0 && next_point(31, 3, 2) == 3 && next_point(0, 0, 0) == 0, "wrap");
  EXPECT(next_point(2047, 9, 2) == 3 && next_point(255, 9, 2) == 259 && next_point(5, 3, 0) == 6 && next_point(7, 3, 0) == 0, "across tiles");
  EXPECT(zinv_slot(0, 2) == 0 && zinv_slot(7, 2) == 3 && zinv_slot(2047, 2) == 3 && zinv_slot(9, 3) == 1 && zinv_slot(9, 0) == 0, "i mod E");
}

static void degree_bound_and_tail() {
  // D = max((len_z - 1) + W max(len_w - 1, 1), 2 (len_w - 1) + n - 1, n + len_z - 2)
  EXPECT(degree_bound(3, 3, 8, 8) == 28 && degree_bound(3, 3, 10, 11) == 37 && degree_bound(0, 2, 1, 1) == 2 && degree_bound(3, 2, 1, 20) == 26, "D");
  EXPECT(degree_bound(2, 2, 9, 1) == 19 && degree_bound(4, 2, 1, 1) == 15 && degree_bound(3, 2, 2, 1) == 9 && degree_bound(3, 2, 3, 1) == 11, "D");
  EXPECT(lens_ok(3, 2, 1, 1) && lens_ok(3, 2, 32, 32) && !lens_ok(3, 2, 0, 8) && !lens_ok(3, 2, 8, 0) && !lens_ok(3, 2, 33, 8) && !lens_ok(3, 2, 8, 33), "1 .. N");
  // blinded W = 3 over E = 4: D - n = 3 n + 5 < 4 n from n = 8 on
  EXPECT(!degree_ok(2, 2, 3, 6, 7) && degree_ok(3, 2, 3, 10, 11) && !degree_ok(3, 2, 3, 32, 5) && degree_ok(20, 2, 3, (1 << 20) + 2, (1 << 20) + 3), "blinded");
  EXPECT(degree_ok(3, 2, 2, 8, 26) && !degree_ok(3, 2, 2, 8, 27), "D - n = N - 1 fits, N does not");
  EXPECT(tail_first(3, 3, 10, 11) == 30 && tail_len(3, 2, 3, 10, 11) == 2 && tail_first(3, 2, 8, 26) == 32 && tail_len(3, 2, 2, 8, 26) == 0, "the tail");
  // D = n - 1: the numerator has fewer than n coefficients, the whole of t must vanish
  EXPECT(tail_first(4, 2, 1, 1) == 0 && degree_ok(4, 2, 2, 1, 1) && tail_len(4, 2, 2, 1, 1) == 64, "D - n = -1");
  EXPECT(tail_tiles(0) == 0 && tail_tiles(1) == 1 && tail_tiles(256) == 1 && tail_tiles(257) == 2 && tail_items(257, 3) == 6 && tail_items(0, 3) == 0, "tail tiles");
}

// the chunks of whole instances: 0, 1, m - 1 and m per chunk, and "not even one fits"
static void chunks_and_scratch() {
  EXPECT(columns(3, false) == 4 && columns(3, true) == 5 && col_z(3) == 3 && col_pi(3) == 4 && columns(32, true) == 34, "columns");
  EXPECT(const_slots(3) == 7 && consts_words(3, 2) == 56 && consts_words(32, 1) == 144 && consts_words(3, SIZE_MAX / 2) == SIZE_MAX, "constants");
  EXPECT(coeff_bytes(10, 6) == 1920 && coeff_bytes(SIZE_MAX / 8, 2) == SIZE_MAX && ext_bytes(3, 2, 6) == 6144 && ext_bytes(26, 2, SIZE_MAX / 4) == SIZE_MAX, "bytes");
  EXPECT(scalars_bytes(3) == 96 && scalars_bytes(SIZE_MAX / 2) == SIZE_MAX && pad_tiles(9, 2, 4, 3) == 96 && pad_tiles(26, 2, SIZE_MAX / 2, 4) == SIZE_MAX, "bytes");
  EXPECT(evals_scratch_bytes(3, 2, 3, 2) == (64 + 56) * 8 && evals_scratch_bytes(0, 0, 2, 1) == 24 * 8 && evals_scratch_bytes(3, 2, 3, SIZE_MAX / 2) == SIZE_MAX, "evals");
  EXPECT(scratch_ok(0) && scratch_ok(SIZE_MAX / 2) && !scratch_ok(SIZE_MAX) && !scratch_ok(SIZE_MAX / 2 + 1), "refused before the lease");
  // log_n = 3, log_e = 2, W = 3, no public inputs: a buffer of an instance is 4 columns of 128 words
  EXPECT(chunk_buffer_words(3, 2, 4, 1) == 512 && chunk_buffer_words(3, 2, 5, 3) == 1920, "a buffer");
  EXPECT(chunk_words(3, 2, 3, 4, 1) == 4 + 64 + 28 + 1024 && chunk_bytes(3, 2, 3, 4, 2) == (4 + 64 + 56 + 2048) * 8, "the lease of a chunk");
  // the forward transform of 32 points has two steps: it leases 4 + 64 words and one buffer more
  EXPECT(ntt_plan::steps(5, ntt_plan::NTT_STAGES_DEFAULT, false, true) == 2, "a shifted transform of 32 points");
  const size_t one = (4 + 64 + 28 + 1024 + 4 + 64 + 512) * 8, two = (4 + 64 + 56 + 2048 + 4 + 64 + 1024) * 8;
  EXPECT(chunk_budget_bytes(3, 2, 3, 4, 1) == one && chunk_budget_bytes(3, 2, 3, 4, 2) == two, "the peak of a chunk: %zu %zu", chunk_budget_bytes(3, 2, 3, 4, 1), one);
  const size_t m = 5;
  EXPECT(instances_per_chunk(3, 2, 3, 4, m, one - 1) == 0 && instances_per_chunk(3, 2, 3, 4, m, 0) == 0, "not even one fits");
  EXPECT(instances_per_chunk(3, 2, 3, 4, m, one) == 1 && instances_per_chunk(3, 2, 3, 4, m, two - 1) == 1 && instances_per_chunk(3, 2, 3, 4, m, two) == 2, "one, two");
  EXPECT(instances_per_chunk(3, 2, 3, 4, m, chunk_budget_bytes(3, 2, 3, 4, m - 1)) == m - 1 && instances_per_chunk(3, 2, 3, 4, m, chunk_budget_bytes(3, 2, 3, 4, m) - 1) == m - 1, "m - 1");
  EXPECT(instances_per_chunk(3, 2, 3, 4, m, chunk_budget_bytes(3, 2, 3, 4, m)) == m && instances_per_chunk(3, 2, 3, 4, m, SIZE_MAX) == m, "all of them");
  EXPECT(instances_per_chunk(3, 2, 3, 4, 0, SIZE_MAX) == 0, "m = 0");
  // every instance in one chunk, once, whatever the chunk size
  for (const size_t mc : {(size_t)1, (size_t)2, m - 1, m, m + 3}) {
    std::vector<int> seen(m, 0);
    size_t count = 0;
    for (size_t s0 = 0; s0 < m; s0 += mc, ++count)
      for (size_t s = 0; s < chunk_size(m, mc, s0); ++s) ++seen[s0 + s];
    bool once = count == chunk_count(m, mc);
    for (const int v : seen) once = once && v == 1;
    EXPECT(once, "chunks of %zu", mc);
  }
  EXPECT(chunk_count(5, 0) == 0 && chunk_count(5, 2) == 3 && chunk_size(5, 2, 4) == 1 && chunk_size(5, 2, 2) == 2, "chunks");
  // saturating sums
  EXPECT(chunk_buffer_words(26, 2, SIZE_MAX / 2, 4) == SIZE_MAX && chunk_words(26, 2, 3, 4, SIZE_MAX / 8) == SIZE_MAX && chunk_bytes(26, 2, 3, 4, (size_t)1 << 33) == SIZE_MAX &&
             chunk_budget_bytes(26, 2, 3, 4, (size_t)1 << 33) == SIZE_MAX,
         "saturates");
  EXPECT(instances_per_chunk(26, 2, 3, 4, (size_t)1 << 40, (size_t)1 << 30) == 0 && chunk_budget_bytes(20, 2, 3, 4, 1) > ((size_t)1 << 30), "2^20 rows do not fit 1 GB");
}

// The scratch limits tests/test_gpu_plonk_prover_routes.py sets for the full route, one row each, the same numbers as that file's
// QUOTIENT_LIMITS (tests/test_plonk_prover_route_limits.py compares the two): log_n, log_e, W, columns, m, the limit in bytes, the instances
// of a full chunk.  Each limit holds that many instances and not one more by the plan's own functions, and cuts m into the chunks beside it.
static const size_t ROUTE_LIMITS[][7] = {
    {9, 2, 3, 4, 3, 2200000, 2},                 // f_two
    {9, 2, 3, 5, 3, 2200000, 2},                 // f_two_pi
};
static const std::vector<size_t> ROUTE_CHUNKS[] = {{2, 1}, {2, 1}};
static void limits_of_the_route_tests() {
  static_assert(sizeof(ROUTE_LIMITS) / sizeof(ROUTE_LIMITS[0]) == sizeof(ROUTE_CHUNKS) / sizeof(ROUTE_CHUNKS[0]), "a chunk sequence per limit");
  for (size_t i = 0; i < sizeof(ROUTE_LIMITS) / sizeof(ROUTE_LIMITS[0]); ++i) {
    const size_t* r = ROUTE_LIMITS[i];
    const int log_n = (int)r[0], log_e = (int)r[1], W = (int)r[2];
    const size_t cols = r[3], m = r[4], limit = r[5], k = r[6];
    EXPECT(dims_ok(log_n, log_e, W) && (cols == columns(W, false) || cols == columns(W, true)), "row %zu: the route takes the shape", i);
    EXPECT(instances_per_chunk(log_n, log_e, W, cols, m, limit) == k, "row %zu: %zu", i, instances_per_chunk(log_n, log_e, W, cols, m, limit));
    EXPECT(k < m && chunk_budget_bytes(log_n, log_e, W, cols, k) <= limit && limit < chunk_budget_bytes(log_n, log_e, W, cols, k + 1), "row %zu: %zu <= %zu < %zu", i,
           chunk_budget_bytes(log_n, log_e, W, cols, k), limit, chunk_budget_bytes(log_n, log_e, W, cols, k + 1));
    std::vector<size_t> sizes;
    for (size_t s0 = 0; s0 < m; s0 += k) sizes.push_back(chunk_size(m, k, s0));
    EXPECT(sizes == ROUTE_CHUNKS[i] && chunk_count(m, k) == sizes.size(), "row %zu: %zu chunks", i, sizes.size());
    // the second buffer of the last chunk starts behind a first buffer of ONE instance, not of two
    EXPECT(chunk_buffer_words(log_n, log_e, cols, sizes.back()) * 2 == chunk_buffer_words(log_n, log_e, cols, k), "row %zu: the smaller last chunk", i);
  }
  // what that file's shapes were chosen for.  (f) blinded rows of 514 and 515 coefficients end inside the third tile of eight, and the status
  // reads 506 coefficients from 1542 on: two tiles, the first lane not at a multiple of 256
  EXPECT(tiles(9, 2) == 8 && degree_ok(9, 2, 3, 514, 515) && tail_first(9, 3, 514, 515) == 1542 && tail_first(9, 3, 514, 515) % PQ_BLOCK == 6, "(f)");
  EXPECT(tail_len(9, 2, 3, 514, 515) == 506 && tail_tiles(tail_len(9, 2, 3, 514, 515)) == 2 && 2 * PQ_BLOCK < 514 && 515 < 3 * PQ_BLOCK, "(f)");
  // (g) W = 17 needs E = 32 at n = 16; two tiles.  W = 2 over E = 8 at n = 32: one tile
  EXPECT(degree_ok(4, 5, 17, 18, 19) && !degree_ok(4, 4, 17, 18, 19) && tiles(4, 5) == 2 && tail_first(4, 17, 18, 19) == 292 && degree_ok(5, 3, 2, 34, 35) && tiles(5, 3) == 1, "(g)");
  // (h) one row, constants: t has two coefficients and the status reads the other two; 300 instances are 1800 constants, 8 blocks of lanes
  EXPECT(degree_ok(0, 2, 2, 1, 1) && tail_first(0, 2, 1, 1) == 2 && tail_len(0, 2, 2, 1, 1) == 2 && tail_tiles(300 * const_slots(2)) == 8 && tail_tiles(300) == 2, "(h)");
  // the rule by hand at (3, E = 4, W = 3): 35000 bytes hold two instances and not three with either column count
  EXPECT(chunk_budget_bytes(3, 2, 3, 5, 2) == 32256 && chunk_budget_bytes(3, 2, 3, 4, 3) == 38624 && instances_per_chunk(3, 2, 3, 4, 5, 35000) == 2 &&
             instances_per_chunk(3, 2, 3, 5, 5, 35000) == 2,
         "two and not three");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // n = 4, E = 2, W = 2: 7 rows.  A layout of the circuit alone: log_n + log_e <= 28, so nothing here can saturate
    const PrepareLayout l = prepare_layout(2, 1, 2);
    const Region r[] = {WORDS(l, g, 4), WORDS(l, roots, 16), WORDS(l, coeff, 112), WORDS(l, l1, 16), WORDS(l, padded, 224)};
    EXPECT(layout_ok("prepare", r, l.bytes) && l.roots == 32 && l.coeff == 160 && l.l1 == 1056 && l.padded == 1184 && l.bytes == 2976, "prepare: %zu", l.bytes);
    const PrepareLayout o = prepare_layout(0, 0, 2);
    const Region q[] = {WORDS(o, g, 4), WORDS(o, roots, 0), WORDS(o, coeff, 28), WORDS(o, l1, 4), WORDS(o, padded, 28)};
    EXPECT(layout_ok("prepare N = 1", q, o.bytes) && o.coeff == 32 && o.l1 == 256 && o.padded == 288 && o.bytes == 512, "N = 1: %zu", o.bytes);
  }
  {
    const EvalsLayout l = evals_layout(2, 1, 2, 3);
    const Region r[] = {WORDS(l, roots, 16), WORDS(l, consts, 72)};
    EXPECT(layout_ok("evals", r, l.bytes) && l.consts == 128 && l.bytes == 704 && evals_layout(0, 0, 2, 1).consts == 0 && evals_layout(0, 0, 2, 1).bytes == 192 &&
               evals_layout(2, 1, 2, SIZE_MAX / 8).bytes == SIZE_MAX, "evals: %zu", l.bytes);
  }
  {  // the full route, 3 columns, chunks of 2 instances; a short last chunk keeps the constants of 2 and packs its buffers behind them
    const ChunkLayout l = chunk_layout(2, 1, 2, 3, 2, 2);
    const Region r[] = {WORDS(l, g, 4), WORDS(l, roots, 16), WORDS(l, consts, 48), WORDS(l, a, 192), WORDS(l, b, 192)};
    EXPECT(layout_ok("chunk", r, l.bytes) && l.roots == 32 && l.consts == 160 && l.a == 544 && l.b == 2080 && l.bytes == 3616 && l.bytes == chunk_bytes(2, 1, 2, 3, 2), "chunk: %zu", l.bytes);
    const ChunkLayout s = chunk_layout(2, 1, 2, 3, 2, 1);
    const Region q[] = {WORDS(s, g, 4), WORDS(s, roots, 16), WORDS(s, consts, 48), WORDS(s, a, 96), WORDS(s, b, 96)};
    EXPECT(layout_ok("short chunk", q, s.bytes) && s.a == 544 && s.b == 1312 && s.bytes == 2080 && s.bytes <= l.bytes, "the last chunk: %zu", s.bytes);
    const ChunkLayout p = chunk_layout(2, 1, 2, 4, 1, 1);
    const Region t[] = {WORDS(p, g, 4), WORDS(p, roots, 16), WORDS(p, consts, 24), WORDS(p, a, 128), WORDS(p, b, 128)};
    EXPECT(layout_ok("chunk of one with public inputs", t, p.bytes) && p.a == 352 && p.b == 1376 && p.bytes == 2400, "one instance: %zu", p.bytes);
    EXPECT(chunk_layout(2, 1, 2, 3, SIZE_MAX / 8, SIZE_MAX / 8).bytes == SIZE_MAX, "saturates");
  }
}

int main() {
  limits_of_the_route_tests();
  constants_and_pins();
  table_layout();
  items_and_tail_tiles();
  degree_bound_and_tail();
  chunks_and_scratch();
  layouts();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
