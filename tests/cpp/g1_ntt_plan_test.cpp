// CPU-only check of the G1 transform's planner (sylow_amd/csrc/g1_ntt_plan.hpp).  It walks every log_n in 0 .. 28 and every stage with
// max_blocks in {1, 2, default} the way the kernels walk them -- lanes of the grid, a grid stride, the lane-to-butterfly map -- and asserts
// that every input and output index is below n, that each output is written exactly once per stage (every index for log_n <= 12, sampled
// lanes above), that the last step writes `out`, that scratch sums saturate instead of wrapping, and that the window tables depend on the
// grid and not on n.  Expected values are written out from the rules in the header's comments (blocks of 256 lanes, 512 blocks by default,
// 1 KB per lane, 12-word projective points).  Built with -fsanitize=address,undefined by tests/test_g1_ntt_plan.py: host code only.
#include "../../sylow_amd/csrc/g1_ntt_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace g1_ntt_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; if (fails < 40) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
#include "layout_check.hpp"

static const long long PINS[] = {1, 2, -1};

// one butterfly as k_g1_ntt_first / k_g1_ntt_stage address it: work item b of the batch -> (array, j) -> indices
static void walk_item(int log_n, int stage, size_t m, size_t b, std::vector<uint8_t>* seen_out, std::vector<uint8_t>* seen_j, size_t& mults) {
  const size_t n = elems(log_n), hn = half(log_n);
  const size_t a = b >> (log_n - 1), q = b & (hn - 1), j = butterfly_of(q, log_n, stage), base = a << log_n;
  bool ok = a < m && j < hn && in0(j) < n && in1(j, log_n) < n && out0(j, stage) < n && out1(j, stage) < n && out0(j, stage) != out1(j, stage);
  ok = ok && base + out1(j, stage) < points(log_n, m);
  if (!unit_twiddle(j, stage)) {
    const size_t e = twiddle_exp(j, log_n, stage);
    ok = ok && e > 0 && e < hn && hn - e > 0 && hn - e < hn && stage_multiplies(stage);       // both directions read the table inside [0, n / 2)
    ++mults;
  } else {
    ok = ok && twiddle_exp(j, log_n, stage) == 0;
  }
  // the rule of the header's comment, written out
  const size_t ns = (size_t)1 << stage;
  ok = ok && out0(j, stage) == (j / ns) * 2 * ns + j % ns && out1(j, stage) == out0(j, stage) + ns && in1(j, log_n) == j + n / 2;
  ok = ok && twiddle_exp(j, log_n, stage) == (j % ns) * (n / (2 * ns)) && unit_twiddle(j, stage) == (j % ns == 0);
  EXPECT(ok, "log_n %d stage %d item %zu: j %zu", log_n, stage, b, j);
  if (seen_out) {
    EXPECT(!(*seen_out)[base + out0(j, stage)] && !(*seen_out)[base + out1(j, stage)], "log_n %d stage %d: an output written twice", log_n, stage);
    (*seen_out)[base + out0(j, stage)] = (*seen_out)[base + out1(j, stage)] = 1;
    EXPECT(!(*seen_j)[a * hn + j], "log_n %d stage %d: a butterfly taken twice", log_n, stage);
    (*seen_j)[a * hn + j] = 1;
  }
}

static void stages_and_indices() {
  for (int log_n = 1; log_n <= G1_NTT_LOG_N_MAX; ++log_n) {
    const size_t m = log_n <= 12 ? 3 : 1, total = butterflies(log_n, m);
    EXPECT(total == m * ((size_t)1 << (log_n - 1)) && stages(log_n) == log_n, "butterflies");
    for (const long long pin : PINS) {
      const size_t g = stage_grid(log_n, m, pin), lanes = g * G1_NTT_BLOCK;
      EXPECT(g >= 1 && g <= (pin < 0 ? 512 : (size_t)pin) && (g == (total + 255) / 256 || g == (pin < 0 ? 512 : (size_t)pin)), "stage grid %zu", g);
      EXPECT(lanes * G1_NTT_TABLE_BYTES_PER_LANE <= table_bytes(log_n, m, false, pin) || log_n < 2, "a lane's table lies inside the lease");
      for (int stage = 0; stage < log_n; ++stage) {
        size_t mults = 0;
        if (log_n <= 12) {            // fully: lane t of the grid walks t, t + lanes, ...
          std::vector<uint8_t> seen_out(points(log_n, m), 0), seen_j(total, 0);
          for (size_t t = 0; t < lanes; ++t)
            for (size_t b = t; b < total; b += lanes) walk_item(log_n, stage, m, b, &seen_out, &seen_j, mults);
          size_t written = 0;
          for (const uint8_t v : seen_out) written += v;
          EXPECT(written == points(log_n, m), "log_n %d stage %d: %zu of %zu outputs written", log_n, stage, written, points(log_n, m));
          EXPECT(mults == m * (stage ? half(log_n) - (half(log_n) >> stage) : 0), "log_n %d stage %d: %zu multiplications", log_n, stage, mults);
        } else if (pin < 0) {         // the ends and a spread of items
          const size_t probes[] = {0, 1, 63, 64, 255, 256, total / 3, total / 2 - 1, total / 2, total - 257, total - 2, total - 1};
          for (const size_t b : probes) walk_item(log_n, stage, m, b, nullptr, nullptr, mults);
          for (size_t b = 12345 % total, i = 0; i < 2000; ++i, b = (b * 2862933555777941757ull + 3037000493ull) % total) walk_item(log_n, stage, m, b, nullptr, nullptr, mults);
        }
      }
    }
    size_t sum = 0;
    for (int p = 1; p < log_n; ++p) sum += ((size_t)1 << (log_n - 1)) - (((size_t)1 << (log_n - 1)) >> p);
    EXPECT(multiplications(log_n) == sum, "multiplications(%d)", log_n);
  }
  EXPECT(multiplications(0) == 0 && multiplications(1) == 0 && multiplications(2) == 1 && multiplications(3) == 5 && multiplications(16) == 458753, "counts");
  // the lane-to-butterfly map: the identity at stage 0 and at the last stage's single group; the unit twiddles are the first n / (2 Ns) items
  for (size_t q = 0; q < 512; ++q) EXPECT(butterfly_of(q, 10, 0) == q && butterfly_of(q, 10, 9) == q, "identity maps");
  for (int stage = 1; stage < 10; ++stage)
    for (size_t q = 0; q < 512; ++q) EXPECT(unit_twiddle(butterfly_of(q, 10, stage), stage) == (q < ((size_t)512 >> stage)), "unit twiddles first: stage %d item %zu", stage, q);
  EXPECT(butterfly_of(5, 4, 1) == 3 && butterfly_of(1, 4, 1) == 2 && butterfly_of(4, 4, 1) == 1, "4 groups of 2: item q is butterfly (q mod 4) 2 + q div 4");
}

static void closing_and_ping_pong() {
  for (int log_n = 0; log_n <= G1_NTT_LOG_N_MAX; ++log_n) {
    EXPECT(steps(log_n) == log_n + 1 && step_writes_out(log_n, log_n), "the closing step writes out");
    for (int s = 0; s < log_n; ++s) {
      EXPECT(!step_writes_out(log_n, s), "no stage writes out");
      EXPECT(stage_dst(s) == (s & 1) && stage_dst(s) < buffers(log_n), "stage %d of %d writes a buffer that exists", s, log_n);
      EXPECT(s == 0 ? stage_src(s) == SRC_INPUT : stage_src(s) == stage_dst(s - 1), "stage %d reads what stage %d wrote", s, s - 1);
      EXPECT(stage_src(s) != stage_dst(s), "a stage never writes the buffer it reads");
    }
    EXPECT(closing_src(log_n) == (log_n ? stage_dst(log_n - 1) : SRC_INPUT), "the closing kernel reads the last stage's buffer");
    EXPECT(buffers(log_n) == (log_n == 0 ? 0 : log_n == 1 ? 1 : 2), "buffers(%d)", log_n);
    EXPECT(closing_scales(log_n, true) == (log_n > 0) && !closing_scales(log_n, false), "n^-1 only for an inverse of more than one point");
    for (const long long pin : PINS) {
      const size_t g = closing_grid(log_n, 1, pin), total = (size_t)1 << log_n;
      EXPECT(g >= 1 && g <= (pin < 0 ? 512 : (size_t)pin) && g * 256 <= table_lanes(log_n, 1, true, pin) + (log_n ? 0 : 256), "closing grid");
      for (size_t t = 0; t < g * 256; t += 97)        // the items a lane walks stay below m n
        for (size_t i = t, c = 0; i < total && c < 4; i += g * 256, ++c) EXPECT(i < points(log_n, 1) && (i >> log_n) == 0, "closing item");
    }
  }
}

static void grids_tables_and_scratch() {
  EXPECT(G1_NTT_BLOCK == 256 && G1_NTT_GRID_DEFAULT == 512 && G1_NTT_GRID_MAX == 4096 && G1_NTT_TABLE_BYTES_PER_LANE == 1024 && G1_NTT_LOG_N_MAX == 28, "constants");
  EXPECT(log_n_ok(0) && log_n_ok(28) && !log_n_ok(-1) && !log_n_ok(29) && max_blocks_ok(-1) && max_blocks_ok(-9) && max_blocks_ok(1) && !max_blocks_ok(0), "argument rules");
  EXPECT(grid_cap(-1) == 512 && grid_cap(1) == 1 && grid_cap(3) == 3 && grid_cap(4096) == 4096 && grid_cap(4097) == 4096 && grid_cap((long long)1 << 62) == 4096, "cap");
  EXPECT(grid(0, -1) == 1 && grid(1, -1) == 1 && grid(256, -1) == 1 && grid(257, -1) == 2 && grid(131072, -1) == 512 && grid(131073, -1) == 512 && grid(SAT, -1) == 512, "grid");
  // log_n = 10 has 512 butterflies: two blocks, so max_blocks = 1 strides
  EXPECT(stage_grid(10, 1, -1) == 2 && stage_grid(10, 1, 1) == 1 && stage_grid(10, 1, 3) == 2 && stage_grid(13, 1, 3) == 3 && stage_grid(13, 1, -1) == 16, "stage grids");
  // the tables: bytes = lanes of the largest multiplying launch * 1 KB; a function of the grid, the same for every n that fills the cap
  EXPECT(table_bytes(0, 5, true, -1) == 0 && table_bytes(1, 1, false, -1) == 0 && table_bytes(1, 1, true, -1) == 256 * 1024, "no multiplying stage below log_n 2");
  EXPECT(table_bytes(2, 1, false, -1) == 256 * 1024 && table_bytes(10, 1, false, -1) == 2 * 256 * 1024 && table_bytes(10, 1, true, -1) == 4 * 256 * 1024, "small n");
  for (int log_n = 18; log_n <= 28; ++log_n)
    for (const size_t m : {(size_t)1, (size_t)7, (size_t)1 << 20}) {
      EXPECT(table_bytes(log_n, m, false, -1) == (size_t)512 * 256 * 1024 && table_bytes(log_n, m, true, -1) == (size_t)512 * 256 * 1024, "128 MB whatever n is");
      EXPECT(table_bytes(log_n, m, true, 1) == 256 * 1024 && table_bytes(log_n, m, false, 2) == 2 * 256 * 1024, "the pin sets the tables");
    }
  // scratch = tables + 32 bytes per table element (n / 2 of them) + buffers of 96 n m bytes
  EXPECT(scratch_bytes(0, 3, false, -1) == 0 && scratch_bytes(0, 3, true, -1) == 0, "log_n 0: no scratch");
  EXPECT(scratch_bytes(1, 1, false, -1) == 32 + 192 && scratch_bytes(1, 2, true, -1) == 32 + 384 + 262144, "log_n 1: %zu", scratch_bytes(1, 2, true, -1));
  EXPECT(scratch_bytes(3, 1, false, -1) == 262144 + 128 + 2 * 768, "log_n 3");
  EXPECT(scratch_bytes(20, 1, true, -1) == (size_t)134217728 + 16777216 + 2 * 100663296, "log_n 20: %zu", scratch_bytes(20, 1, true, -1));
  EXPECT(buffer_words(20, 1) == 12582912 && twiddle_words(20) == 2097152 && points(3, 5) == 40, "words");
  EXPECT(xy_bytes(3, 2) == 1024 && inf_bytes(3, 2) == 16 && xy_bytes(28, 1) == (size_t)1 << 34, "the caller's arrays");
  // saturation: 2^28 * m wraps 64 bits from m = 2^36 on, the bytes of the points earlier
  EXPECT(points(28, (size_t)1 << 36) == SAT && points(28, ((size_t)1 << 36) - 1) == 0xfffffffff0000000ull, "points saturate");
  EXPECT(xy_bytes(28, (size_t)1 << 30) == SAT && xy_bytes(28, ((size_t)1 << 30) - 1) != SAT && xy_bytes(1, SAT / 2) == SAT, "bytes saturate");
  EXPECT(buffer_words(28, (size_t)1 << 33) == SAT && scratch_bytes(28, (size_t)1 << 33, false, -1) == SAT && scratch_bytes(28, (size_t)1 << 30, true, 1) == SAT, "scratch saturates");
  EXPECT(scratch_bytes(28, (size_t)1 << 29, false, -1) == SAT && scratch_bytes(28, (size_t)1 << 28, false, -1) == ((size_t)192 << 56) + ((size_t)1 << 32) + ((size_t)1 << 27), "2 * 96 * 2^57 bytes is beyond 64 bits, 2 * 96 * 2^56 is not");
  EXPECT(butterflies(28, (size_t)1 << 40) == SAT && stage_grid(28, (size_t)1 << 40, -1) == 512, "a saturated count still has a grid");
  EXPECT(disjoint(1000, 1064, 64) && disjoint(1064, 1000, 64) && !disjoint(1000, 1063, 64) && !disjoint(1063, 1000, 64) && !disjoint(1000, 1000, 64), "ranges");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // n = 8: one block of lanes multiplies, 256 KB of tables FIRST; the twiddles land on the byte behind them
    const ScratchLayout l = scratch_layout(3, 1, false, -1);
    const Region r[] = {BYTES(l, tables, 262144), WORDS(l, twiddles, 16), WORDS(l, buf[0], 96), WORDS(l, buf[1], 96)};
    EXPECT(layout_ok("n = 8", r, l.bytes) && l.tables == 0 && l.twiddles == 262144 && l.buf[0] == 262272 && l.buf[1] == 263040 && l.bytes == 263808, "n = 8: %zu", l.bytes);
  }
  {  // n = 2, inverse: the closing scale alone multiplies; one buffer
    const ScratchLayout l = scratch_layout(1, 2, true, -1);
    const Region r[] = {BYTES(l, tables, 262144), WORDS(l, twiddles, 4), WORDS(l, buf[0], 48), WORDS(l, buf[1], 0)};
    EXPECT(layout_ok("n = 2 inverse", r, l.bytes) && l.twiddles == 262144 && l.buf[0] == 262176 && l.bytes == 262560, "n = 2 inverse: %zu", l.bytes);
  }
  {  // n = 2, forward: no tables
    const ScratchLayout l = scratch_layout(1, 1, false, -1);
    const Region r[] = {BYTES(l, tables, 0), WORDS(l, twiddles, 4), WORDS(l, buf[0], 24), WORDS(l, buf[1], 0)};
    EXPECT(layout_ok("n = 2", r, l.bytes) && l.twiddles == 0 && l.buf[0] == 32 && l.bytes == 224, "n = 2: %zu", l.bytes);
  }
  EXPECT(scratch_layout(0, 3, false, -1).bytes == 0 && scratch_layout(28, (size_t)1 << 33, false, -1).bytes == SAT, "n = 1 leases nothing; saturates");
  // the tables are whole KB for every grid a pin can ask for, so the words behind them are aligned
  for (const long long pin : {-1ll, 1ll, 7ll, 4096ll, 1ll << 40}) EXPECT(table_bytes(20, 3, true, pin) % 1024 == 0, "pin %lld", pin);
}

int main() {
  stages_and_indices();
  closing_and_ping_pong();
  grids_tables_and_scratch();
  layouts();
  if (fails) {
    printf("%d of %zu checks FAILED\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
