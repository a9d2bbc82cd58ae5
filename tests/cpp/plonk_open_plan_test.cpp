// CPU-only check of the planner of PLONK's closing rounds (sylow_amd/csrc/plonk_open_plan.hpp).  Every expected value is written out by hand
// from the rules in the header's comments (2 W + 2 rows of n coefficients; 2 W + 1 evaluations an instance; items of (instance, row, chunk
// of 2048 coefficients) over the chunks of the longest row; 3 W + 3 + E rows of the fold and two scalars behind their weights; a lane per
// column, 256 columns per tile; a chunk of the full route leases the points, the partials, the weights, F and the padded z, two values, two
// proofs and their flags, and the opening leases a quotient buffer more).  The walks are walked as the kernels walk them.  Built with
// -fsanitize=address,undefined by tests/test_plonk_open_plan.py: host code only.
#include "../../sylow_amd/csrc/plonk_open_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace plonk_open_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static void constants_and_pins() {
  EXPECT(PO_BLOCK == 256 && PO_FLUSH == 16 && PO_WEIGHT_ROUND == 16 && PO_WIRES_MIN == 2 && PO_WIRES_MAX == 32 && PO_LOG_MAX == 28 && PO_EVAL_CHUNK == 2048, "constants");
  EXPECT(STATUS_R_NOT_ZERO == 1 && STATUS_ZETA_IN_DOMAIN == 2 && FR_WORDS == 4, "constants");
  EXPECT(dims_ok(0, 0, 2) && dims_ok(26, 2, 32) && dims_ok(0, 28, 3) && dims_ok(28, 0, 3), "the legal corners");
  EXPECT(!dims_ok(27, 2, 3) && !dims_ok(-1, 2, 3) && !dims_ok(3, -1, 3) && !dims_ok(3, 2, 1) && !dims_ok(3, 2, 33) && !dims_ok(3, 2, 0) && !dims_ok(29, 0, 3) &&
             !dims_ok(0, 29, 3) && !dims_ok(2147483647, 2147483647, 3),
         "refused");
  EXPECT(!max_blocks_ok(0) && max_blocks_ok(-1) && max_blocks_ok(1) && max_blocks_ok(1ll << 40), "max_blocks");
  EXPECT(grid(10, -1) == 10 && grid(0, -1) == 1 && grid(1048577, -1) == 1048576 && grid(10, 1) == 1 && grid(10, 3) == 3 && grid(2, 3) == 2 && grid(5, 1ll << 40) == 5, "grid");
  EXPECT(lens_ok(5, 1, 1) && lens_ok(5, 32, 32) && !lens_ok(5, 0, 8) && !lens_ok(5, 8, 0) && !lens_ok(5, 33, 8) && !lens_ok(5, 8, 33) && lens_ok(28, 1u << 28, 1), "1 .. N");
  EXPECT(lane_tiles(0) == 0 && lane_tiles(1) == 1 && lane_tiles(256) == 1 && lane_tiles(257) == 2 && ceil_div(7, 2) == 4 && max2(3, 9) == 9, "lanes");
}

static void table_and_slots() {
  EXPECT(ctable_rows(2) == 6 && ctable_rows(3) == 8 && ctable_rows(32) == 66, "2 W + 2 rows");
  EXPECT(row_selector(2) == 2 && row_qm(3) == 3 && row_qc(3) == 4 && row_sigma(3, 0) == 5 && row_sigma(3, 2) == 7 && row_sigma(32, 31) == 65, "W = 3");
  EXPECT(ctable_words(3, 3) == 8 * 32 && ctable_bytes(3, 3) == 2048 && ctable_words(0, 2) == 24 && selectors_bytes(3, 3) == 1280 && sigma_bytes(3, 3) == 768, "bytes");
  EXPECT(eval_slots(3) == 7 && slot_wire(2) == 2 && slot_sigma(3, 0) == 3 && slot_sigma(3, 1) == 4 && slot_zw(3) == 5 && slot_pi(3) == 6 && eval_slots(32) == 65, "2 W + 1 slots");
  EXPECT(evals_count(3, 2) == 14 && evals_bytes(3, 2) == 32 * 7 * 2 && evals_bytes(3, SIZE_MAX / 4) == SIZE_MAX, "evals_out = 32 (2 W + 1) m bytes");
  EXPECT(scalars_bytes(3) == 96 && scalars_bytes(SIZE_MAX / 2) == SIZE_MAX && coeff_bytes(10, 6) == 1920 && coeff_bytes(SIZE_MAX / 8, 2) == SIZE_MAX, "bytes");
  // the weights: 2 W + 2 shared rows, z, W wires, E chunks, the constant term, ZH
  EXPECT(fold_rows(2, 3) == 16 && weight_slots(2, 3) == 18 && wrow_z(3) == 8 && wrow_wire(3, 0) == 9 && wrow_wire(3, 2) == 11 && wrow_chunk(3, 0) == 12 && wrow_chunk(3, 3) == 15, "W = 3, E = 4");
  EXPECT(wslot_const(2, 3) == 16 && wslot_zh(2, 3) == 17 && weight_words(2, 3, 2) == 144 && weight_words(5, 17, 1) == 4 * 88 && weight_words(2, 3, SIZE_MAX / 8) == SIZE_MAX, "slots");
  // the rows only F takes: sigma_0 .. sigma_(W-2) and the wires
  std::vector<size_t> extra;
  for (size_t row = 0; row < fold_rows(2, 3); ++row)
    if (row_is_extra(3, row)) extra.push_back(row);
  EXPECT(extra == (std::vector<size_t>{5, 6, 9, 10, 11}), "W = 3: %zu rows", extra.size());
  size_t count2 = 0;
  for (size_t row = 0; row < fold_rows(2, 2); ++row) count2 += row_is_extra(2, row) ? 1 : 0;
  EXPECT(count2 == 3 && row_is_extra(2, 4) && !row_is_extra(2, 5) && !row_is_extra(2, 6) && row_is_extra(2, 7) && row_is_extra(2, 8) && !row_is_extra(2, 9), "W = 2");
  // the product counts the GPU tests' shapes were chosen for
  EXPECT(products_r(2, 3) == 11 && products_f(2, 3) == 16 && products_r(3, 4) == 16 && products_f(3, 4) == 23 && products_r(2, 2) == 10 && products_f(5, 17) == 86, "products");
  for (const int W : {2, 3, 17, 32}) {
    size_t r = 0, f = 0;
    for (size_t row = 0; row < fold_rows(3, W); ++row) (row_is_extra(W, row) ? f : r) += 1;
    EXPECT(r == products_r(3, W) && r + f == products_f(3, W), "W = %d", W);
  }
}

// every coefficient of every row belongs to one lane of one live item, whatever the pin; an item past the end of its row is dead
static void eval_items_and_chunk_edges() {
  EXPECT(eval_chunks(0) == 1 && eval_chunks(1) == 1 && eval_chunks(2048) == 1 && eval_chunks(2049) == 2 && eval_chunks(2051) == 2 && eval_chunks(4097) == 3, "chunks");
  EXPECT(eval_items(7, 11, 2) == 14 && eval_items(7, 2051, 3) == 42 && eval_items(7, 2051, 0) == 0 && eval_items(65, SIZE_MAX, SIZE_MAX / 2) == SIZE_MAX, "items");
  EXPECT(eval_item_instance(41, 7, 2) == 2 && eval_item_row(41, 7, 2) == 6 && eval_item_chunk(41, 2) == 1 && eval_item_instance(13, 7, 2) == 0 && eval_item_row(14, 7, 2) == 0, "(instance, row, chunk)");
  EXPECT(eval_chunk_live(2050, 0) && eval_chunk_live(2050, 1) && !eval_chunk_live(2048, 1) && !eval_chunk_live(0, 0) && eval_chunk_live(1, 0) && !eval_chunk_live(2050, 2), "live");
  EXPECT(eval_fold_segment(1) == 1 && eval_fold_segment(256) == 1 && eval_fold_segment(257) == 2 && eval_fold_segment(513) == 3 && eval_fold_lanes(513) == 171 &&
             eval_fold_lanes(256) == 256 && eval_fold_lanes(257) == 129 && eval_fold_lanes(2) == 2 && eval_fold_lanes((size_t)1 << 17) == 256,
         "the lanes of the second launch");
  EXPECT(longest_row(11, 2050, 2051) == 2051 && longest_row(3, 1, 1) == 8 && longest_row(0, 3, 2) == 3, "the longest row");
  EXPECT(point_words(3) == 24 && eval_partial_words(7, 11, 2) == 56 && evaluate_scratch_words(3, 3, 10, 11, 2) == 16 + 56 && evaluate_scratch_words(11, 3, 2050, 2051, 3) == 24 + 4 * 42, "scratch");
  EXPECT(evaluate_scratch_words(3, 32, 8, 8, SIZE_MAX / 16) == SIZE_MAX && !scratch_ok(SIZE_MAX) && scratch_ok(0) && scratch_ok(SIZE_MAX / 16) && !scratch_ok(SIZE_MAX / 16 + 1), "saturates");
  const size_t lens[3] = {2050, 2051, 2048}, rows = 3, m = 2, longest = 2051, chunks = eval_chunks(longest), its = eval_items(rows, longest, m);
  for (const long long pin : {-1ll, 1ll, 5ll}) {
    std::vector<int> seen(m * rows * 2051, 0);
    const size_t g = grid(its, pin);
    for (size_t block = 0; block < g; ++block)
      for (size_t it = block; it < its; it += g) {
        const size_t s = eval_item_instance(it, rows, chunks), c = eval_item_row(it, rows, chunks), q = eval_item_chunk(it, chunks);
        EXPECT(s < m && c < rows && q < chunks && it == (s * rows + c) * chunks + q, "item %zu", it);
        if (!eval_chunk_live(lens[c], q)) continue;
        for (size_t k = q * PO_EVAL_CHUNK; k < (q + 1) * PO_EVAL_CHUNK && k < lens[c]; ++k) ++seen[(s * rows + c) * 2051 + k];
      }
    bool once = true;
    for (size_t s = 0; s < m; ++s)
      for (size_t c = 0; c < rows; ++c)
        for (size_t k = 0; k < 2051; ++k) once = once && seen[(s * rows + c) * 2051 + k] == (k < lens[c] ? 1 : 0);
    EXPECT(once, "every coefficient once under the pin %lld", pin);
  }
}

static void fold_tiles_and_lengths() {
  EXPECT(len_r(3, 11) == 11 && len_r(3, 5) == 8 && len_f(3, 10, 11) == 11 && len_f(3, 20, 11) == 20 && len_f(0, 1, 1) == 1, "the lengths of r and F");
  EXPECT(len_out_ok(3, 10, 11, 11, true) && !len_out_ok(3, 10, 11, 10, false) && len_out_ok(3, 20, 11, 11, false) && !len_out_ok(3, 20, 11, 19, true) && len_out_ok(3, 20, 11, 20, true), "len_out");
  EXPECT(tiles(0) == 0 && tiles(1) == 1 && tiles(256) == 1 && tiles(259) == 2 && tiles(2051) == 9 && items(259, 3) == 6 && items(259, 0) == 0 && items(SIZE_MAX, (size_t)1 << 10) == SIZE_MAX, "tiles");
  EXPECT(item_instance(5, 2) == 2 && column(5, 2, 3) == 259 && column(4, 2, 255) == 255 && column(0, 1, 0) == 0, "(instance, column)");
  for (const size_t len : {(size_t)1, (size_t)256, (size_t)259, (size_t)2051}) {
    const size_t m = 3, nt = tiles(len), its = items(len, m);
    for (const long long pin : {-1ll, 1ll, 5ll}) {
      std::vector<int> seen(m * len, 0);
      const size_t g = grid(its, pin);
      for (size_t block = 0; block < g; ++block)
        for (size_t it = block; it < its; it += g)
          for (int t = 0; t < PO_BLOCK; ++t) {
            const size_t s = item_instance(it, nt), k = column(it, nt, t);
            EXPECT(s < m, "instance");
            if (k < len) ++seen[s * len + k];
          }
      bool once = true;
      for (const int v : seen) once = once && v == 1;
      EXPECT(once, "every column of %zu once under the pin %lld", len, pin);
    }
  }
  // linearise: the points, the weights, r(zeta) and the partials of its evaluation; r itself only when the caller takes F alone
  EXPECT(linearise_scratch_words(3, 2, 3, 11, 16, 2, false) == 16 + 144 + 0 + 8 + 8 && linearise_scratch_words(3, 2, 3, 11, 16, 2, true) == 16 + 144 + 88 + 8 + 8, "scratch");
  EXPECT(linearise_scratch_words(11, 2, 3, 2051, 4100, 1, false) == 8 + 72 + 4 * 3 + 4 && linearise_scratch_words(3, 2, 3, 11, 16, SIZE_MAX / 8, true) == SIZE_MAX, "scratch");
}

// the chunks of whole instances: 0, 1, m - 1 and m per chunk, and "not even one fits"
static void chunks_and_scratch() {
  EXPECT(flag_words(1) == 1 && flag_words(4) == 1 && flag_words(5) == 2 && flag_words(0) == 0, "two flags an instance, rounded up to a word");
  // log_n = 3, E = 4, W = 3, len_w = 10, len_z = 11, len_f = 16: per instance 8 + 28 + 72 + 128 + 24 words, and the flags
  EXPECT(open_chunk_words(3, 2, 3, 10, 11, 16, 1) == 260 + 1 && open_chunk_words(3, 2, 3, 10, 11, 16, 2) == 520 + 1 && open_chunk_bytes(3, 2, 3, 10, 11, 16, 5) == (1300 + 2) * 8, "the lease");
  const size_t one = (260 + 64 + 1) * 8, two = (520 + 128 + 1) * 8;
  EXPECT(open_budget_bytes(3, 2, 3, 10, 11, 16, 1) == one && open_budget_bytes(3, 2, 3, 10, 11, 16, 2) == two && one == 2600 && two == 5192, "the peak: the quotient buffer on top");
  const size_t m = 5;
  EXPECT(instances_per_chunk(3, 2, 3, 10, 11, 16, m, one - 1) == 0 && instances_per_chunk(3, 2, 3, 10, 11, 16, m, 0) == 0, "not even one fits: the call is refused");
  EXPECT(instances_per_chunk(3, 2, 3, 10, 11, 16, m, one) == 1 && instances_per_chunk(3, 2, 3, 10, 11, 16, m, 4000) == 1 && instances_per_chunk(3, 2, 3, 10, 11, 16, m, two - 1) == 1 &&
             instances_per_chunk(3, 2, 3, 10, 11, 16, m, two) == 2,
         "one, two");
  EXPECT(instances_per_chunk(3, 2, 3, 10, 11, 16, m, open_budget_bytes(3, 2, 3, 10, 11, 16, m - 1)) == m - 1 &&
             instances_per_chunk(3, 2, 3, 10, 11, 16, m, open_budget_bytes(3, 2, 3, 10, 11, 16, m) - 1) == m - 1,
         "m - 1");
  EXPECT(instances_per_chunk(3, 2, 3, 10, 11, 16, m, open_budget_bytes(3, 2, 3, 10, 11, 16, m)) == m && instances_per_chunk(3, 2, 3, 10, 11, 16, m, SIZE_MAX) == m, "all of them");
  EXPECT(instances_per_chunk(3, 2, 3, 10, 11, 16, 0, SIZE_MAX) == 0, "m = 0");
  // whatever the budget, the chunk fits it and one more instance would not
  for (size_t budget = one; budget < 12 * one; budget += 997) {
    const size_t mc = instances_per_chunk(3, 2, 3, 10, 11, 16, 9, budget);
    EXPECT(mc >= 1 && open_budget_bytes(3, 2, 3, 10, 11, 16, mc) <= budget && (mc == 9 || open_budget_bytes(3, 2, 3, 10, 11, 16, mc + 1) > budget), "budget %zu: %zu", budget, mc);
  }
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
  EXPECT(open_chunk_words(20, 2, 3, 10, 11, SIZE_MAX / 2, 4) == SIZE_MAX && open_chunk_bytes(20, 2, 3, 10, 11, (size_t)1 << 40, (size_t)1 << 30) == SIZE_MAX &&
             open_budget_bytes(20, 2, 3, 10, 11, (size_t)1 << 40, (size_t)1 << 30) == SIZE_MAX,
         "saturates");
  EXPECT(instances_per_chunk(20, 2, 3, (1 << 20) + 2, (1 << 20) + 3, (size_t)1 << 40, 4, (size_t)1 << 30) == 0, "a row that does not fit 1 GB is refused");
  // 2^20 rows, len_f = 2^20 + 4: one instance is below 101 MB, ten fit 1 GB
  EXPECT(open_budget_bytes(20, 2, 3, (1 << 20) + 2, (1 << 20) + 3, (1 << 20) + 4, 1) < ((size_t)101 << 20) &&
             instances_per_chunk(20, 2, 3, (1 << 20) + 2, (1 << 20) + 3, (1 << 20) + 4, 16, (size_t)1 << 30) == 10,
         "2^20 rows: %zu bytes an instance", open_budget_bytes(20, 2, 3, (1 << 20) + 2, (1 << 20) + 3, (1 << 20) + 4, 1));
}

// The scratch limits tests/test_gpu_plonk_prover_routes.py sets for the full route, one row each, the same numbers as that file's OPEN_LIMITS
// (tests/test_plonk_prover_route_limits.py compares the two): log_n, log_e, W, len_w, len_z, len_f, m, the limit in bytes, the instances of a
// full chunk.  Each limit holds that many instances and not one more by the plan's own functions, and cuts m into the chunks beside it.
static const size_t ROUTE_LIMITS[][9] = {
    {3, 2, 3, 10, 11, 16, 5, 6000, 2},           // a_two
    {3, 2, 3, 10, 11, 16, 5, 4000, 1},           // a_one
    {8, 2, 2, 258, 259, 300, 3, 70000, 2},       // b_two
    {0, 2, 2, 3, 4, 4, 300, 164500, 128},        // e_128
};
static const std::vector<size_t> ROUTE_CHUNKS[] = {{2, 2, 1}, {1, 1, 1, 1, 1}, {2, 1}, {128, 128, 44}};
static void limits_of_the_route_tests() {
  static_assert(sizeof(ROUTE_LIMITS) / sizeof(ROUTE_LIMITS[0]) == sizeof(ROUTE_CHUNKS) / sizeof(ROUTE_CHUNKS[0]), "a chunk sequence per limit");
  for (size_t i = 0; i < sizeof(ROUTE_LIMITS) / sizeof(ROUTE_LIMITS[0]); ++i) {
    const size_t* r = ROUTE_LIMITS[i];
    const int log_n = (int)r[0], log_e = (int)r[1], W = (int)r[2];
    const size_t len_w = r[3], len_z = r[4], len_f = r[5], m = r[6], limit = r[7], k = r[8];
    EXPECT(dims_ok(log_n, log_e, W) && lens_ok(log_big(log_n, log_e), len_w, len_z) && len_out_ok(log_n, len_w, len_z, len_f, true), "row %zu: the route takes the shape", i);
    EXPECT(instances_per_chunk(log_n, log_e, W, len_w, len_z, len_f, m, limit) == k, "row %zu: %zu", i, instances_per_chunk(log_n, log_e, W, len_w, len_z, len_f, m, limit));
    EXPECT(k < m && open_budget_bytes(log_n, log_e, W, len_w, len_z, len_f, k) <= limit && limit < open_budget_bytes(log_n, log_e, W, len_w, len_z, len_f, k + 1),
           "row %zu: %zu <= %zu < %zu", i, open_budget_bytes(log_n, log_e, W, len_w, len_z, len_f, k), limit, open_budget_bytes(log_n, log_e, W, len_w, len_z, len_f, k + 1));
    std::vector<size_t> sizes;
    for (size_t s0 = 0; s0 < m; s0 += k) sizes.push_back(chunk_size(m, k, s0));
    EXPECT(sizes == ROUTE_CHUNKS[i] && chunk_count(m, k) == sizes.size(), "row %zu: %zu chunks", i, sizes.size());
  }
  // the rule by hand at the first shape: an instance leases 260 words and the opening 64 more, and the two flags of each round up to a word
  EXPECT(open_budget_bytes(3, 2, 3, 10, 11, 16, 2) == (2 * 324 + 1) * 8 && open_budget_bytes(3, 2, 3, 10, 11, 16, 3) == (3 * 324 + 1) * 8, "k 324 words and the flags");
  // a ragged last chunk runs with stride 1 inside a lease laid out for 2: the second point of an instance lies 4 c words on, not 4 mc
  EXPECT(chunk_size(5, 2, 4) == 1 && point_words(2) == 16 && point_words(1) == 8, "the last chunk of a_two");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // n = 4, W = 3: 7 slots of one chunk each, 2 instances
    const EvaluateLayout l = evaluate_layout(2, 3, 5, 6, 2);
    const Region r[] = {WORDS(l, pts, 16), WORDS(l, partials, 56)};
    EXPECT(layout_ok("evaluate", r, l.bytes) && l.partials == 128 && l.bytes == 576, "evaluate: %zu", l.bytes);
    EXPECT(evaluate_layout(2, 2, 1, 1, 1).partials == 64 && evaluate_layout(2, 2, 1, 1, 1).bytes == 224 && evaluate_layout(2, 3, 5, 6, SIZE_MAX / 8).bytes == SIZE_MAX,
           "one instance; saturates");
  }
  {  // E = 2: 16 weight slots; the caller takes only F, so r (6 coefficients) lies behind the partials
    const LineariseLayout l = linearise_layout(2, 1, 3, 6, 8, 2, true);
    const Region r[] = {WORDS(l, pts, 16), WORDS(l, weights, 128), WORDS(l, rz, 8), WORDS(l, partials, 8), WORDS(l, r_buf, 48)};
    EXPECT(layout_ok("linearise, own r", r, l.bytes) && l.weights == 128 && l.rz == 1152 && l.partials == 1216 && l.r_buf == 1280 && l.bytes == 1664, "own r: %zu", l.bytes);
    const LineariseLayout o = linearise_layout(2, 1, 3, 6, 8, 2, false);
    const Region q[] = {WORDS(o, pts, 16), WORDS(o, weights, 128), WORDS(o, rz, 8), WORDS(o, partials, 8), WORDS(o, r_buf, 0)};
    EXPECT(layout_ok("linearise", q, o.bytes) && o.partials == 1216 && o.r_buf == 1280 && o.bytes == 1280 && linearise_layout(2, 1, 3, 6, 8, SIZE_MAX / 8, true).bytes == SIZE_MAX,
           "r to the caller: %zu", o.bytes);
  }
  {  // the full route, 3 instances a chunk, an SRS of 8 points: 6 flag bytes, padded to 8
    const OpenLayout l = open_layout(2, 1, 3, 5, 6, 8, 3);
    const Region r[] = {WORDS(l, ev.pts, 24), WORDS(l, ev.partials, 84), WORDS(l, weights, 192), WORDS(l, F, 96), WORDS(l, Z, 96), WORDS(l, yf, 12), WORDS(l, yz, 12),
                        WORDS(l, p1, 24), WORDS(l, p2, 24), BYTES(l, f1, 3), BYTES(l, f2, 3)};
    EXPECT(layout_ok("open", r, l.bytes) && l.ev.partials == 192 && l.ev.bytes == 864 && l.weights == 864 && l.F == 2400 && l.Z == 3168 && l.yf == 3936 && l.yz == 4032, "open: %zu", l.yz);
    EXPECT(l.p1 == 4128 && l.p2 == 4320 && l.f1 == 4512 && l.f2 == 4515 && l.bytes == 4520, "open: %zu", l.bytes);
  }
  {
    const OpenLayout l = open_layout(2, 1, 3, 5, 6, 8, 1);
    const Region r[] = {WORDS(l, ev.pts, 8), WORDS(l, ev.partials, 28), WORDS(l, weights, 64), WORDS(l, F, 32), WORDS(l, Z, 32), WORDS(l, yf, 4), WORDS(l, yz, 4),
                        WORDS(l, p1, 8), WORDS(l, p2, 8), BYTES(l, f1, 1), BYTES(l, f2, 1)};
    EXPECT(layout_ok("open of one", r, l.bytes) && l.weights == 288 && l.F == 800 && l.Z == 1056 && l.yf == 1312 && l.p1 == 1376 && l.f1 == 1504 && l.f2 == 1505 && l.bytes == 1512,
           "one instance: %zu", l.bytes);
    EXPECT(open_layout(2, 1, 3, 5, 6, 8, SIZE_MAX / 8).bytes == SIZE_MAX, "saturates");
  }
}

int main() {
  limits_of_the_route_tests();
  constants_and_pins();
  table_and_slots();
  eval_items_and_chunk_edges();
  fold_tiles_and_lengths();
  chunks_and_scratch();
  layouts();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
