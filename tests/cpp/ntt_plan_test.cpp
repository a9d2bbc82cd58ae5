// CPU-only check of the Fr transform's planner (sylow_amd/csrc/ntt_plan.hpp): passes, the uneven last pass, tiles, items and grids, the table,
// the ping-pong, the scratch and n^-1.  Every expected value below is written out by hand from the rules in the header's comments (a tile is
// 2^10 elements, at most 10 stages per pass, 5 by default, 4 words of constants, a grid of at most 2^20 blocks); nothing on the expected side
// is computed from the header.  Built with -fsanitize=address,undefined by tests/test_ntt_plan.py: host code only.
#include "../../sylow_amd/csrc/ntt_plan.hpp"

#include <cstdint>
#include <cstdio>

using namespace ntt_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static void passes_and_stages() {
  EXPECT(NTT_LOG_N_MAX == 28 && NTT_BLOCK == 256 && NTT_TILE_LOG == 10 && NTT_STAGES_MAX == 10 && NTT_STAGES_DEFAULT == 5 && NTT_CONST_WORDS == 4, "constants");
  EXPECT(stages_ok(-1) && stages_ok(-7) && stages_ok(1) && stages_ok(10) && !stages_ok(0) && !stages_ok(11) && !stages_ok(1 << 30), "stages_ok");
  EXPECT(stages_or_default(-1) == 5 && stages_or_default(3) == 3, "default");
  // {log_n, stages, passes, stages of the last pass}
  const int p[][4] = {{0, 10, 0, 0},  {1, 10, 1, 1},  {10, 10, 1, 10}, {11, 10, 2, 1},  {20, 10, 2, 10}, {21, 10, 3, 1}, {28, 10, 3, 8},
                      {28, 1, 28, 1}, {13, 3, 5, 1},  {12, 3, 4, 3},   {7, 2, 4, 1},    {9, 4, 3, 1},    {5, 5, 1, 5},   {6, 5, 2, 1},
                      {10, 5, 2, 5},  {11, 5, 3, 1},  {20, 5, 4, 5},   {28, 5, 6, 3}};
  for (const auto& c : p) {
    EXPECT(passes(c[0], c[1]) == c[2], "passes(%d, %d) = %d", c[0], c[1], passes(c[0], c[1]));
    if (c[2]) EXPECT(pass_stages(c[0], c[1], c[2] - 1) == c[3], "last pass of (%d, %d) = %d", c[0], c[1], pass_stages(c[0], c[1], c[2] - 1));
    int sum = 0;
    for (int i = 0; i < c[2]; ++i) {
      if (i + 1 < c[2]) EXPECT(pass_stages(c[0], c[1], i) == c[1], "a full pass");
      EXPECT(pass_done_log(c[1], i) == sum, "done before pass %d", i);
      sum += pass_stages(c[0], c[1], i);
    }
    EXPECT(sum == c[0], "the stages of (%d, %d) add up to %d", c[0], c[1], sum);
  }
}

static void tiles_and_grids() {
  // {log_n, stages of the pass, log2 groups per tile, tiles per array}: a tile is 2^10 elements, or the whole array when that is smaller
  const int t[][4] = {{1, 1, 0, 1},  {3, 1, 2, 1},   {10, 10, 0, 1}, {10, 1, 9, 1},  {11, 10, 0, 2}, {11, 1, 9, 2},   {13, 3, 7, 8},
                      {20, 10, 0, 1024}, {21, 1, 9, 2048}, {28, 10, 0, 262144}, {28, 8, 2, 262144}, {9, 4, 5, 1}, {12, 5, 5, 4}};
  for (const auto& c : t) {
    EXPECT(pass_group_log(c[0], c[1]) == c[2], "group_log(%d, %d) = %d", c[0], c[1], pass_group_log(c[0], c[1]));
    EXPECT(pass_tiles(c[0], c[1]) == (size_t)c[3], "tiles(%d, %d) = %zu", c[0], c[1], pass_tiles(c[0], c[1]));
    EXPECT(c[1] + c[2] <= 10, "a tile fits LDS");
  }
  EXPECT(pass_items(20, 10, 1) == 1024 && pass_items(11, 10, 5) == 10 && pass_items(8, 8, 4096) == 4096 && pass_items(3, 3, 0) == 0, "items");
  EXPECT(pass_items(28, 10, (size_t)1 << 30) == (size_t)1 << 48, "items beyond 32 bits");
  EXPECT(grid(10) == 10 && grid(1048576) == 1048576 && grid(1048577) == 1048576 && grid((size_t)1 << 48) == 1048576 && grid(0) == 1, "grid");
  // the element-wise kernel: 256 lanes of 16 elements = 4096 per chunk
  EXPECT(scale_chunks(0) == 1 && scale_chunks(12) == 1 && scale_chunks(13) == 2 && scale_chunks(28) == 65536 && scale_items(13, 3) == 6, "scale");
  EXPECT(scales(0, false, false) && !scales(1, false, false) && scales(1, true, false) && scales(1, false, true) && scales(5, true, true), "scales");
}

static void table_and_scratch() {
  // the table holds n/2 elements of 4 words; a block of the table kernel covers 4096 of them
  const size_t tw[][3] = {{0, 0, 0}, {1, 4, 1}, {2, 8, 1}, {10, 2048, 1}, {11, 4096, 1}, {13, 16384, 1}, {14, 32768, 2}, {21, 4194304, 256}, {28, 536870912, 32768}};
  for (const auto& c : tw) {
    EXPECT(table_words((int)c[0]) == c[1], "table_words(%zu) = %zu", c[0], table_words((int)c[0]));
    EXPECT(table_blocks((int)c[0]) == c[2], "table_blocks(%zu) = %zu", c[0], table_blocks((int)c[0]));
  }
  EXPECT(root_squarings(28) == 0 && root_squarings(0) == 28 && root_squarings(10) == 18, "squarings down from the 2^28-th root");
  // steps: passes + the element-wise kernel (inverse, shifted, or no pass at all); the last step writes out, the one before the buffer
  EXPECT(steps(0, 10, false, false) == 1 && steps(0, 10, true, true) == 1 && steps(10, 10, false, false) == 1 && steps(10, 10, true, false) == 2, "steps");
  EXPECT(steps(11, 10, false, false) == 2 && steps(11, 10, false, true) == 3 && steps(21, 10, true, true) == 4 && steps(13, 3, false, false) == 5, "steps");
  EXPECT(step_writes_out(1, 0) && !step_writes_out(2, 0) && step_writes_out(2, 1) && step_writes_out(3, 0) && !step_writes_out(3, 1) && step_writes_out(3, 2), "ping-pong");
  for (int k = 1; k <= 29; ++k) EXPECT(step_writes_out(k, k - 1) && (k < 2 || !step_writes_out(k, k - 2)), "the last of %d steps writes out", k);
  EXPECT(!needs_buffer(1) && needs_buffer(2) && needs_buffer(29), "buffer");
  // scratch words = 4 + table + (more than one step ? 4 n m : 0) at log_n = 0, 1, S, S + 1, 2 S + 1, 28 for S = 5 and for S = 10
  EXPECT(scratch_words(0, 3, 1) == 4, "log_n 0: %zu", scratch_words(0, 3, 1));
  EXPECT(scratch_words(1, 3, 1) == 8 && scratch_words(1, 3, 2) == 8 + 24, "log_n 1");
  EXPECT(steps(5, 5, false, false) == 1 && steps(6, 5, false, false) == 2 && steps(11, 5, false, false) == 3 && steps(28, 5, true, true) == 7, "steps at S = 5");
  EXPECT(scratch_words(5, 1, 1) == 4 + 64 && scratch_words(6, 1, 2) == 4 + 128 + 256 && scratch_words(6, 3, 2) == 4 + 128 + 768, "log_n S, S + 1 at S = 5");
  EXPECT(scratch_words(10, 1, 1) == 4 + 2048 && scratch_words(10, 2, 2) == 4 + 2048 + 8192, "log_n S");
  EXPECT(scratch_words(11, 1, 2) == 4 + 4096 + 8192 && scratch_words(11, 5, 3) == 4 + 4096 + 40960, "log_n S + 1");
  EXPECT(scratch_words(21, 1, 3) == 4 + 4194304 + 8388608, "log_n 2 S + 1");
  EXPECT(scratch_words(28, 1, 3) == 4 + 536870912 + 1073741824, "log_n 28");
  EXPECT(batch_words(28, 1) == 1073741824 && batch_words(0, 7) == 28 && batch_words(3, 0) == 0, "batch words");
  // saturation: 4 * 2^28 * m wraps 64 bits from m = 2^34 on
  EXPECT(batch_words(28, ((size_t)1 << 34) - 1) == 0xffffffffc0000000ull && batch_words(28, (size_t)1 << 34) == SAT && batch_words(1, SAT / 2) == SAT, "saturated batch");
  EXPECT(scratch_words(28, (size_t)1 << 34, 3) == SAT && scratch_words(28, (size_t)1 << 34, 1) == 4 + 536870912, "saturated scratch");
  EXPECT(mul_sat(SAT, 2) == SAT && mul_sat(SAT, 1) == SAT && mul_sat(0, SAT) == 0 && mul_sat(SAT, 0) == 0 && add_sat(SAT - 1, 2) == SAT && add_sat(1, 2) == 3, "sat");
}

static void n_inverses() {
  // n^-1 mod r, written out: 1, (r + 1) / 2, and 2^-28
  const uint64_t want[][5] = {{0, 1, 0, 0, 0},
                              {1, 0xa1f0fac9f8000001ull, 0x9419f4243cdcb848ull, 0xdc2822db40c0ac2eull, 0x183227397098d014ull},
                              {28, 0xa84aec7fb1e0a6c2ull, 0x101e6275f67aec09ull, 0xa536431afc7cfcf5ull, 0x30644e6fdaecb8fbull}};
  for (const auto& c : want) {
    const Words4 v = n_inverse((int)c[0]);
    EXPECT(v.w[0] == c[1] && v.w[1] == c[2] && v.w[2] == c[3] && v.w[3] == c[4], "n_inverse(%d) = %016llx %016llx %016llx %016llx", (int)c[0],
           (unsigned long long)v.w[3], (unsigned long long)v.w[2], (unsigned long long)v.w[1], (unsigned long long)v.w[0]);
  }
  // every size, word-wise: n^-1 + ((r - 1) >> log_n) = r
  for (int log_n = 0; log_n <= 28; ++log_n) {
    const Words4 v = n_inverse(log_n);
    unsigned __int128 carry = 0;
    bool ok = true;
    const uint64_t rm1[4] = {FR_R.w[0] - 1, FR_R.w[1], FR_R.w[2], FR_R.w[3]};
    for (int i = 0; i < 4; ++i) {
      const uint64_t q = log_n ? (rm1[i] >> log_n) | (i < 3 ? rm1[i + 1] << (64 - log_n) : 0) : rm1[i];
      carry += (unsigned __int128)v.w[i] + q;
      ok = ok && (uint64_t)carry == FR_R.w[i];
      carry >>= 64;
    }
    EXPECT(ok && carry == 0, "n_inverse(%d) + ((r - 1) >> %d) = r", log_n, log_n);
  }
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {
    const ScratchLayout l = scratch_layout(3, 2, 2);
    const Region r[] = {WORDS(l, consts, 4), WORDS(l, table, 16), WORDS(l, buf, 64)};
    EXPECT(layout_ok("two steps", r, l.bytes) && l.table == 32 && l.buf == 160 && l.bytes == 672, "two steps: %zu", l.bytes);
  }
  {  // one step writes out: no buffer
    const ScratchLayout l = scratch_layout(3, 2, 1);
    const Region r[] = {WORDS(l, consts, 4), WORDS(l, table, 16), WORDS(l, buf, 0)};
    EXPECT(layout_ok("one step", r, l.bytes) && l.buf == 160 && l.bytes == 160, "one step: %zu", l.bytes);
  }
  {  // n = 1: no table
    const ScratchLayout l = scratch_layout(0, 1, 1);
    const Region r[] = {WORDS(l, consts, 4), WORDS(l, table, 0), WORDS(l, buf, 0)};
    EXPECT(layout_ok("n = 1", r, l.bytes) && l.table == 32 && l.bytes == 32, "n = 1: %zu", l.bytes);
  }
  EXPECT(scratch_layout(28, SIZE_MAX / 4, 2).bytes == SIZE_MAX, "saturates");
}

int main() {
  passes_and_stages();
  tiles_and_grids();
  table_and_scratch();
  n_inverses();
  layouts();
  if (fails) {
    printf("%d of %zu checks FAILED\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
