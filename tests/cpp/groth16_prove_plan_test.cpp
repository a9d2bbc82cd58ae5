// CPU-only check of the Groth16 prover's planner (sylow_amd/csrc/groth16_prove_plan.hpp): lanes per row, grids, scratch and the witnesses a
// chunk holds.  Every expected value below is written out by hand from the rules in the header's comments (a lane gets at least 8 entries of
// an average row; a block is 256 lanes; an Fr element is 4 words; a chunk's closing sums are 21 G1 points, 7 G2 points and 3 scalars per
// witness, a flag byte per point); nothing on the expected side is computed from the header.
// Built with -fsanitize=address,undefined by tests/test_groth16_prove_plan.py: host code only.
#include "../../sylow_amd/csrc/groth16_prove_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace g16_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static void spmv_geometry() {
  EXPECT(G16_BLOCK == 256 && SPMV_FLUSH == 16 && SPMV_LANES_LOG_MAX == 6 && SPMV_LANE_ENTRIES == 8 && G16_COSET_SHIFT == 5, "constants");
  // average densities 0, 1, 3, 64 and 10^6 over 1000 rows: 1, 1, 1, 8 and 64 lanes per row
  const size_t dens[][2] = {{0, 0}, {1, 0}, {3, 0}, {15, 0}, {16, 1}, {31, 1}, {32, 2}, {64, 3}, {127, 3}, {128, 4}, {256, 5}, {511, 5}, {512, 6}, {1000000, 6}};
  for (const auto& d : dens) EXPECT(spmv_lanes_log(1000, d[0] * 1000) == (int32_t)d[1], "spmv_lanes_log(density %zu) = %d", d[0], spmv_lanes_log(1000, d[0] * 1000));
  EXPECT(spmv_lanes_log(0, 0) == 0 && spmv_lanes_log(0, 12345) == 0 && spmv_lanes_log(1, 300) == 5 && spmv_lanes_log(3, 2999) == 6, "no rows, one row");
  EXPECT(spmv_lanes_log(1000, 15999) == 0 && spmv_lanes_log(1000, 16000) == 1, "the density is nnz / rows rounded down");
  EXPECT(spmv_lanes_log_or_default(-1, 1000, 64000) == 3 && spmv_lanes_log_or_default(0, 1000, 64000) == 0 && spmv_lanes_log_or_default(6, 1000, 0) == 6, "pins");
  EXPECT(spmv_lanes_log_ok(-1) && spmv_lanes_log_ok(0) && spmv_lanes_log_ok(6) && !spmv_lanes_log_ok(7), "legal pins");
  EXPECT(spmv_rows_per_block(0) == 256 && spmv_rows_per_block(3) == 32 && spmv_rows_per_block(6) == 4, "rows per block");
  EXPECT(spmv_row_blocks(1, 0) == 1 && spmv_row_blocks(256, 0) == 1 && spmv_row_blocks(257, 0) == 2 && spmv_row_blocks(257, 3) == 9 && spmv_row_blocks(0, 0) == 0, "row blocks");
  EXPECT(spmv_row_blocks((size_t)1 << 28, 6) == 67108864 && grid_x(67108864) == 1048576 && grid_x(1048575) == 1048575 && grid_x(0) == 1 && grid_x(9) == 9, "grid x");
  EXPECT(grid_y(0) == 1 && grid_y(3) == 3 && grid_y(65534) == 65534 && grid_y(65535) == 65535 && grid_y(65536) == 65535 && grid_y((size_t)1 << 40) == 65535, "grid y");
  EXPECT(batch_words(5, 3) == 60 && batch_words(0, 3) == 0 && batch_words((size_t)1 << 33, (size_t)1 << 20) == (size_t)1 << 55, "batch words");
  EXPECT(batch_words(SIZE_MAX / 2, 3) == SIZE_MAX && batch_words((size_t)1 << 62, 1) == SIZE_MAX, "saturates");
  EXPECT(spmv_scratch_words(1000, 3) == 12000 && lane_blocks(0) == 0 && lane_blocks(256) == 1 && lane_blocks(257) == 2, "scratch, element-wise blocks");
}

static void quotient_scratch() {
  EXPECT(log_n_ok(0) && log_n_ok(28) && !log_n_ok(-1) && !log_n_ok(29), "log_n");
  // two buffers of 3 m arrays of 4 n words, and 4 words for the shift
  EXPECT(quot_buffer_words(0, 1) == 12 && quot_scratch_words(0, 1) == 28, "n = 1");
  EXPECT(quot_buffer_words(3, 2) == 192 && quot_scratch_words(3, 2) == 388, "n = 8, m = 2");
  EXPECT(quot_buffer_words(20, 1) == 12582912 && quot_scratch_words(20, 1) == 25165828, "n = 2^20");
  EXPECT(quot_scratch_words(28, (size_t)1 << 40) == SIZE_MAX, "saturates");
}

static void prove_chunks() {
  EXPECT(close_words(1) == 292 && close_words(3) == 876 && close_flag_bytes(1) == 28 && close_flag_bytes(2) == 56, "the closing sums");
  EXPECT(private_vars(7, 2) == 4 && private_vars(3, 1) == 1 && private_vars(1, 0) == 0, "private variables");
  // (log_n, n_vars, l) = (3, 7, 2): z 28 words, its private part 16, the quotient 4 + 2 * 96, h cut to 7 terms 28, the closing sums 292
  EXPECT(prove_chunk_words(3, 7, 2, 1) == 560 && prove_chunk_bytes(3, 7, 2, 1) == 4512, "one witness: %zu words", prove_chunk_words(3, 7, 2, 1));
  EXPECT(prove_chunk_words(3, 7, 2, 2) == 1116 && prove_chunk_bytes(3, 7, 2, 2) == 8984, "two witnesses: %zu words", prove_chunk_words(3, 7, 2, 2));
  // what the transform of 3 mc arrays leases on top: 4 words, a table of 4 elements, one more buffer
  EXPECT(prove_budget_bytes(3, 7, 2, 1) == 5440 && prove_budget_bytes(3, 7, 2, 2) == 10680 && prove_budget_bytes(3, 7, 2, 3) == 15928, "budget bytes");
  const size_t per[][2] = {{0, 0}, {5439, 0}, {5440, 1}, {10679, 1}, {10680, 2}, {15927, 2}, {15928, 3}, {(size_t)1 << 30, 5}};
  for (const auto& p : per) EXPECT(witnesses_per_chunk(3, 7, 2, 5, p[0]) == p[1], "witnesses_per_chunk(budget %zu) = %zu", p[0], witnesses_per_chunk(3, 7, 2, 5, p[0]));
  EXPECT(witnesses_per_chunk(3, 7, 2, 0, (size_t)1 << 30) == 0 && witnesses_per_chunk(3, 7, 2, 2, (size_t)1 << 30) == 2, "m bounds the chunk");
  // the largest measured shape: 2^20 constraints and variables, 384 MiB of arrays and a 16 MiB table per witness -- two fit the default GB
  EXPECT(prove_chunk_bytes(20, (size_t)1 << 20, 1, 1) == 301992192 && prove_budget_bytes(20, (size_t)1 << 20, 1, 1) == 419432736, "2^20: %zu",
         prove_budget_bytes(20, (size_t)1 << 20, 1, 1));
  EXPECT(witnesses_per_chunk(20, (size_t)1 << 20, 1, 4, (size_t)1 << 30) == 2 && witnesses_per_chunk(20, (size_t)1 << 20, 1, 4, 419432735) == 0, "2^20 under a GB");
  EXPECT(witnesses_per_chunk(28, (size_t)1 << 28, 1, 1, (size_t)1 << 30) == 0 && witnesses_per_chunk(0, 3, 1, 7, (size_t)1 << 30) == 7, "the ends");
  EXPECT(prove_budget_bytes(28, SIZE_MAX / 2, 0, 3) == SIZE_MAX && witnesses_per_chunk(28, SIZE_MAX / 2, 0, 3, SIZE_MAX - 1) == 0, "a saturated witness never fits");
}

// The scratch limits of tests/test_gpu_groth16_prove_routes.py: (log_n, n_vars, n_inputs, m, the limit in bytes, the witnesses of a full chunk
// under it).  tests/test_groth16_prove_route_limits.py reads these rows and compares them with the GPU file's.
static const size_t ROUTE_LIMITS[][6] = {
    {3, 7, 2, 7, 16000, 3},                      // a_three
    {3, 7, 2, 7, 12000, 2},                      // a_two
    {3, 7, 2, 513, 1350000, 257},                // b_257
    {3, 65539, 2, 2, 6000000, 1},                // f_one
};
static const std::vector<size_t> ROUTE_CHUNKS[] = {{3, 3, 1}, {2, 2, 2, 1}, {257, 256}, {1, 1}};
static void limits_of_the_route_tests() {
  static_assert(sizeof(ROUTE_LIMITS) / sizeof(ROUTE_LIMITS[0]) == sizeof(ROUTE_CHUNKS) / sizeof(ROUTE_CHUNKS[0]), "a chunk sequence per limit");
  for (size_t i = 0; i < sizeof(ROUTE_LIMITS) / sizeof(ROUTE_LIMITS[0]); ++i) {
    const size_t* r = ROUTE_LIMITS[i];
    const int32_t log_n = (int32_t)r[0];
    const size_t n_vars = r[1], l = r[2], m = r[3], limit = r[4], mc = r[5];
    EXPECT(log_n_ok(log_n) && l < n_vars, "row %zu: the entry point takes the shape", i);
    EXPECT(witnesses_per_chunk(log_n, n_vars, l, m, limit) == mc, "row %zu: %zu", i, witnesses_per_chunk(log_n, n_vars, l, m, limit));
    EXPECT(mc >= 1 && mc < m && prove_budget_bytes(log_n, n_vars, l, mc) <= limit && limit < prove_budget_bytes(log_n, n_vars, l, mc + 1), "row %zu: %zu <= %zu < %zu", i,
           prove_budget_bytes(log_n, n_vars, l, mc), limit, prove_budget_bytes(log_n, n_vars, l, mc + 1));
    std::vector<size_t> sizes;                   // the loop of sylow_hip_groth16_prove_batch
    for (size_t j0 = 0; j0 < m; j0 += mc) sizes.push_back(m - j0 < mc ? m - j0 : mc);
    EXPECT(sizes == ROUTE_CHUNKS[i], "row %zu: %zu chunks", i, sizes.size());
  }
  // the rule by hand at the first shape: a witness leases 4512 bytes of its own (above) and the transform of its three arrays 8 (4 + 16 + 96)
  // more; what a second and a third add differs by the flags' rounding to a word only
  EXPECT(prove_budget_bytes(3, 7, 2, 3) == 15928 && prove_budget_bytes(3, 7, 2, 4) == 21168 && prove_budget_bytes(3, 7, 2, 257) == 1347904, "n = 8");
  // 2^16 + 3 variables: the witness and its private part are all but 5 KB of a chunk
  EXPECT(prove_budget_bytes(3, 65539, 2, 1) == 4199488 && prove_budget_bytes(3, 65539, 2, 2) == 8398776 && 32 * (65539 + 65536) == 4194400, "n_vars = 2^16 + 3");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {
    const QuotLayout l = quot_layout(3, 2);
    const Region r[] = {WORDS(l, g, 4), WORDS(l, x, 192), WORDS(l, y, 192)};
    EXPECT(layout_ok("quotient", r, l.bytes) && l.x == 32 && l.y == 1568 && l.bytes == 3104, "quotient: %zu", l.bytes);
  }
  {
    const QuotLayout l = quot_layout(0, 1);
    const Region r[] = {WORDS(l, g, 4), WORDS(l, x, 12), WORDS(l, y, 12)};
    EXPECT(layout_ok("quotient n = 1", r, l.bytes) && l.x == 32 && l.y == 128 && l.bytes == 224, "n = 1: %zu", l.bytes);
  }
  EXPECT(quot_layout(28, (size_t)1 << 40).bytes == SIZE_MAX, "saturates");
  {  // n = 8, 7 variables, 2 inputs (4 private), ONE witness: 28 flag bytes, padded to 32
    const ProveLayout l = prove_layout(3, 7, 2, 1);
    const Region r[] = {WORDS(l, zc, 28), WORDS(l, zl, 16), WORDS(l, quot.g, 4), WORDS(l, quot.x, 96), WORDS(l, quot.y, 96), WORDS(l, hq, 28), WORDS(l, raw1, 32),
                        WORDS(l, raw2, 16), WORDS(l, p, 136), WORDS(l, q, 96), WORDS(l, f, 12), BYTES(l, raw1_inf, 4), BYTES(l, raw2_inf, 1), BYTES(l, p_inf, 17),
                        BYTES(l, q_inf, 6)};
    EXPECT(layout_ok("prove", r, l.bytes) && l.zl == 224 && l.quot.g == 352 && l.quot.x == 384 && l.quot.y == 1152 && l.quot.bytes == 1920 && l.hq == 1920, "prove: %zu", l.hq);
    EXPECT(l.raw1 == 2144 && l.p == 2528 && l.f == 4384 && l.raw1_inf == 4480 && l.raw2_inf == 4484 && l.p_inf == 4485 && l.q_inf == 4502 && l.bytes == 4512, "prove: %zu", l.bytes);
  }
  {  // two witnesses: every region twice as long but g
    const ProveLayout l = prove_layout(3, 7, 2, 2);
    const Region r[] = {WORDS(l, zc, 56), WORDS(l, zl, 32), WORDS(l, quot.g, 4), WORDS(l, quot.x, 192), WORDS(l, quot.y, 192), WORDS(l, hq, 56), WORDS(l, raw1, 64),
                        WORDS(l, raw2, 32), WORDS(l, p, 272), WORDS(l, q, 192), WORDS(l, f, 24), BYTES(l, raw1_inf, 8), BYTES(l, raw2_inf, 2), BYTES(l, p_inf, 34),
                        BYTES(l, q_inf, 12)};
    EXPECT(layout_ok("prove 2", r, l.bytes) && l.quot.g == 704 && l.raw1_inf == 8928 && l.bytes == 8984, "two witnesses: %zu", l.bytes);
  }
  {  // n = 1, one variable, no input: no private part and no h
    const ProveLayout l = prove_layout(0, 1, 0, 1);
    const Region r[] = {WORDS(l, zc, 4), WORDS(l, zl, 0), WORDS(l, quot.g, 4), WORDS(l, quot.x, 12), WORDS(l, quot.y, 12), WORDS(l, hq, 0), WORDS(l, raw1, 32),
                        WORDS(l, raw2, 16), WORDS(l, p, 136), WORDS(l, q, 96), WORDS(l, f, 12), BYTES(l, raw1_inf, 4), BYTES(l, raw2_inf, 1), BYTES(l, p_inf, 17),
                        BYTES(l, q_inf, 6)};
    EXPECT(layout_ok("prove n = 1", r, l.bytes) && l.zl == 32 && l.quot.g == 32 && l.hq == 256 && l.raw1 == 256 && l.raw1_inf == 2592 && l.bytes == 2624, "n = 1: %zu", l.bytes);
  }
  EXPECT(prove_layout(20, (size_t)1 << 20, 1, SIZE_MAX / 4).bytes == SIZE_MAX && spmv_scratch_bytes(1000, 3) == 96000 && spmv_scratch_bytes(SIZE_MAX / 4, 2) == SIZE_MAX, "saturate");
}

int main() {
  limits_of_the_route_tests();
  spmv_geometry();
  quotient_scratch();
  prove_chunks();
  layouts();
  if (fails) { printf("%d of %zu checks failed\n", fails, checked); return 1; }
  printf("OK %zu checks\n", checked);
  return 0;
}
