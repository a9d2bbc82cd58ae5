// CPU-only check of the planner of the KZG proofs at every point of the domain (sylow_amd/csrc/kzg_open_all_plan.hpp).  For every log_n in
// 0 .. 27 it walks the call the way kzg_open_all.hip launches it -- the fused first stage of the inverse transform of 2n points, its
// stages from 1 on with the indices of g1_ntt_plan.hpp, the first stage of the forward transform of n points, its stages from 1 on, the
// closing kernel -- with max_blocks in {1, 3, default}, lanes of the grid and a grid stride.  Up to log_n = 10 (three arrays) it keeps, per
// column of each of the two buffers, the step that wrote it last: every index is in range, every step writes each of its columns once,
// every read meets what the step before wrote, the forward first stage reads the first n columns of each array only and takes column
// n - 1 as the identity, and the ping-pong ends in the buffer the closing kernel reads.  Above that it probes items.  Then: where F lies,
// the column of x each SRS point goes to, sums that saturate, window tables that depend on the grid and not on n.  Expected values are
// written out from the rules in the header's comments.  Built with -fsanitize=address,undefined by tests/test_kzg_open_all_plan.py: host code only.
#include "../../sylow_amd/csrc/kzg_open_all_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace kzg_open_all_plan;
namespace g1 = g1_ntt_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; if (fails < 40) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
#include "layout_check.hpp"

static const long long PINS[] = {1, 3, -1};

struct Buffers {                       // the step that wrote each column last (0: never)
  std::vector<int> col[2];
  size_t stride;
  bool read(int buf, size_t c, int step) const { return c < stride && col[buf][c] == step; }
  bool write(int buf, size_t c, int step, int before) {
    if (c >= stride || col[buf][c] == step) return false;           // out of range, or written twice by this step
    (void)before;
    col[buf][c] = step;
    return true;
  }
  size_t written(int buf, int step) const {
    size_t k = 0;
    for (const int v : col[buf]) k += v == step;
    return k;
  }
};

// a stage >= 1 of g1_ntt.hip as g1ntth::stage launches it: arrays of 2^log points at columns a 2^log of buffers of the given stride
static void walk_stage(Buffers& B, int log, int stage, size_t m, long long pin, int src, int dst, int step, size_t& mults) {
  const size_t total = g1::butterflies(log, m), lanes = g1::stage_grid(log, m, pin) * g1::G1_NTT_BLOCK, hn = g1::half(log);
  for (size_t t = 0; t < lanes; ++t)
    for (size_t b = t; b < total; b += lanes) {
      const size_t a = b >> (log - 1), j = g1::butterfly_of(b & (hn - 1), log, stage), base = a << log;
      EXPECT(B.read(src, base + g1::in0(j), step - 1) && B.read(src, base + g1::in1(j, log), step - 1), "log %d stage %d item %zu reads what step %d wrote", log, stage, b, step - 1);
      EXPECT(B.write(dst, base + g1::out0(j, stage), step, step - 1) && B.write(dst, base + g1::out1(j, stage), step, step - 1), "log %d stage %d item %zu writes once", log, stage, b);
      if (!g1::unit_twiddle(j, stage)) ++mults;
    }
  EXPECT(B.written(dst, step) == m << log, "log %d stage %d: every column of every array written", log, stage);
}

static void whole_call(int log_n, size_t m, long long pin) {
  const size_t n = elems(log_n), nn = wide(log_n), str = stride(log_n, m);
  const int L = wide_log(log_n);
  Buffers B;
  B.stride = str;
  B.col[0].assign(str, 0);
  B.col[1].assign(str, 0);
  EXPECT(str == m * 2 * n && buffer_words(log_n, m) == 12 * str, "stride");
  size_t mults = 0;
  int step = 1;
  // the fused stage: table and F indices below 2n, both outputs in range, each once
  {
    const size_t total = first_items(log_n, m), lanes = first_grid(log_n, m, pin) * g1::G1_NTT_BLOCK;
    EXPECT(total == m * n && lanes <= table_lanes(log_n, m, pin), "the fused stage's lanes have tables");
    EXPECT(inv_dst(0) != FR_BUFFER, "the fused stage does not write where F lies");
    for (size_t t = 0; t < lanes; ++t)
      for (size_t b = t; b < total; b += lanes) {
        const size_t a = b >> log_n, j = b & (n - 1);
        EXPECT(a < m && first_in0(j) == j && first_in1(j, log_n) == j + n && first_in1(j, log_n) < nn, "table and F indices of item %zu", b);
        EXPECT(a * nn + first_in1(j, log_n) < padded_words(log_n, m) / FR_WORDS, "F of array %zu", a);
        EXPECT(first_out0(a, j, log_n) == a * nn + 2 * j && first_out1(a, j, log_n) == a * nn + 2 * j + 1, "outputs of item %zu", b);
        EXPECT(B.write(inv_dst(0), first_out0(a, j, log_n), step, 0) && B.write(inv_dst(0), first_out1(a, j, log_n), step, 0), "fused item %zu writes once", b);
        mults += 2;
      }
    EXPECT(B.written(inv_dst(0), step) == str, "the fused stage writes every column");
  }
  for (int s = 1; s < inv_stages(log_n); ++s) {
    ++step;
    EXPECT(inv_src(s) == inv_dst(s - 1) && inv_src(s) != inv_dst(s), "inverse stage %d reads what stage %d wrote", s, s - 1);
    EXPECT(g1::stage_grid(L, m, pin) * g1::G1_NTT_BLOCK <= table_lanes(log_n, m, pin), "an inverse stage's lanes have tables");
    walk_stage(B, L, s, m, pin, inv_src(s), inv_dst(s), step, mults);
  }
  EXPECT(fwd_src(log_n, 0) == inv_dst(inv_stages(log_n) - 1), "h lies where the last inverse stage wrote");
  // the forward first stage: reads the first n columns of each array of 2n, column n - 1 as the identity; writes arrays of n
  {
    const int src = fwd_src(log_n, 0), dst = fwd_dst(log_n, 0), before = step;
    ++step;
    const size_t total = fwd_items(log_n, m), lanes = fwd_grid(log_n, m, pin) * g1::G1_NTT_BLOCK, hn = g1::half(log_n);
    EXPECT(src != dst && total == m * hn, "forward first stage");
    size_t identities = 0;
    for (size_t t = 0; t < lanes; ++t)
      for (size_t b = t; b < total; b += lanes) {
        const size_t a = b >> (log_n - 1), j = b & (hn - 1), i0 = fwd_in0(a, j, log_n), i1 = fwd_in1(a, j, log_n);
        EXPECT(a < m && i0 >= a * nn && i0 < a * nn + n && i1 >= a * nn && i1 < a * nn + n && i0 != i1, "item %zu reads the first n columns of array %zu", b, a);
        EXPECT(B.read(src, i0, before) && B.read(src, i1, before), "item %zu reads what the inverse transform wrote", b);
        EXPECT(fwd_in1_is_identity(j, log_n) == (i1 == a * nn + n - 1) && i0 != a * nn + n - 1, "h_(n-1) is V of the last butterfly alone");
        identities += fwd_in1_is_identity(j, log_n);
        EXPECT(fwd_out0(a, j, log_n) == a * n + 2 * j && fwd_out1(a, j, log_n) == a * n + 2 * j + 1 && fwd_out1(a, j, log_n) < m * n, "outputs of item %zu", b);
        EXPECT(B.write(dst, fwd_out0(a, j, log_n), step, before) && B.write(dst, fwd_out1(a, j, log_n), step, before), "forward item %zu writes once", b);
      }
    EXPECT(identities == m && B.written(dst, step) == m * n, "one identity per array, every column of the arrays of n written");
  }
  for (int s = 1; s < fwd_stages(log_n); ++s) {
    ++step;
    EXPECT(fwd_src(log_n, s) == fwd_dst(log_n, s - 1) && fwd_src(log_n, s) != fwd_dst(log_n, s), "forward stage %d reads what stage %d wrote", s, s - 1);
    EXPECT(g1::stage_grid(log_n, m, pin) * g1::G1_NTT_BLOCK <= table_lanes(log_n, m, pin), "a forward stage's lanes have tables");
    walk_stage(B, log_n, s, m, pin, fwd_src(log_n, s), fwd_dst(log_n, s), step, mults);
  }
  // the closing kernel reads columns i < m n of the last buffer and writes the caller's arrays: the last step of the call
  EXPECT(close_src(log_n) == fwd_dst(log_n, fwd_stages(log_n) - 1) && close_src(log_n) == 0, "the closing kernel reads the last stage's buffer");
  const size_t lanes = g1::closing_grid(log_n, m, pin) * g1::G1_NTT_BLOCK;
  for (size_t t = 0; t < lanes; ++t)
    for (size_t i = t; i < g1::points(log_n, m); i += lanes) EXPECT(B.read(close_src(log_n), i, step), "closing item %zu reads the last stage's column", i);
  EXPECT(mults == m * multiplications(log_n), "log_n %d: %zu multiplications against %zu", log_n, mults, m * multiplications(log_n));
}

static void probes(int log_n) {           // sizes too large to keep a vector for: the ends and a spread of items of both first stages
  const size_t m = 1, n = elems(log_n), nn = wide(log_n), total = first_items(log_n, m), hn = g1::half(log_n);
  for (size_t b = 7 % total, i = 0; i < 4000; ++i, b = i < 8 ? (i & 1 ? total - 1 - i : i) : (b * 2862933555777941757ull + 3037000493ull) % total) {
    const size_t j = b & (n - 1);
    EXPECT((b >> log_n) == 0 && first_in1(j, log_n) < nn && first_out1(0, j, log_n) < stride(log_n, m) && first_out0(0, j, log_n) + 1 == first_out1(0, j, log_n), "fused item %zu", b);
    const size_t q = b & (hn - 1);
    EXPECT(fwd_in0(0, q, log_n) < n && fwd_in1(0, q, log_n) < n && fwd_out1(0, q, log_n) < n && fwd_in1_is_identity(q, log_n) == (q == hn - 1), "forward item %zu", q);
  }
  const size_t cap = 512, first = n / 256 < cap ? n / 256 : cap, fwd = hn / 256 < cap ? hn / 256 : cap;          // blocks of 256 lanes, 512 by default
  EXPECT(first_grid(log_n, m, -1) == first && fwd_grid(log_n, m, -1) == fwd && g1::stage_grid(wide_log(log_n), m, -1) == first, "the grids and the cap");
  EXPECT(close_src(log_n) == 0 && fwd_src(log_n, 0) == (log_n & 1) && inv_dst(0) == 0, "ping-pong");
}

static void table_of_x() {
  for (int log_n = 0; log_n <= 10; ++log_n) {
    const size_t n = elems(log_n), nn = wide(log_n);
    std::vector<int> used(n, 0);
    size_t identities = 0;
    for (size_t k = 0; k < nn; ++k) {
      const size_t t = x_srs_index(k, log_n);
      if (t == X_IDENTITY) { ++identities; EXPECT(k <= n, "columns 0 .. n hold the identity"); continue; }
      EXPECT(t <= n - 2 && k == nn - 1 - t && !used[t], "x_(2n-1-t) = s_t, t <= n - 2");
      used[t] = 1;
    }
    EXPECT(identities == n + 1 && !used[n - 1], "n + 1 identities; s_(n-1) is not used");
    EXPECT(prepare_scratch_bytes(log_n) == 64 * nn + nn && prepare_grid(log_n) == (nn + 255) / 256, "scratch and grid of prepare");
  }
  EXPECT(x_srs_index((size_t)1 << 28, 27) == X_IDENTITY && x_srs_index(((size_t)1 << 28) - 1, 27) == 0 && x_srs_index(((size_t)1 << 27) + 1, 27) == ((size_t)1 << 27) - 2, "2^27");
}

static void sizes_tables_and_scratch() {
  EXPECT(OPEN_ALL_LOG_N_MAX == 27 && log_n_ok(0) && log_n_ok(27) && !log_n_ok(-1) && !log_n_ok(28) && max_blocks_ok(-1) && max_blocks_ok(1) && !max_blocks_ok(0), "argument rules");
  EXPECT(trivial(0) && !trivial(1) && scratch_bytes(0, 5, -1) == 0, "log_n = 0 runs nothing of the plan");
  EXPECT(multiplications(0) == 2 && multiplications(1) == 5 && multiplications(2) == 14 && multiplications(3) == 38, "counts");
  for (int log_n = 1; log_n <= 27; ++log_n) {
    const size_t n = elems(log_n);
    EXPECT(multiplications(log_n) == 2 * n + (n * (size_t)(log_n - 1) + 1) + ((n / 2) * (size_t)(log_n - 2) + 1) || log_n == 1, "the formula at %d", log_n);
  }
  EXPECT(multiplications(1) == 4 + 1 + 0, "log_n = 1: four products, one twiddle of the inverse of four points");
  // P and F: two Fr arrays of [m][4][2n] in the 12 word planes of buffer 1
  for (const size_t m : {(size_t)1, (size_t)3}) {
    EXPECT(FR_BUFFER == 1 && pad_offset() == 0 && f_offset(5, m) == 4 * 64 * m && f_offset(5, m) + padded_words(5, m) <= buffer_words(5, m), "P, then F, inside the buffer");
  }
  // tables: 1 KB per lane of the fused stage's grid; a function of the grid, the same for every n that fills the cap
  EXPECT(table_bytes(1, 1, -1) == 256 * 1024 && table_bytes(10, 1, -1) == 4 * 256 * 1024 && table_bytes(10, 1, 3) == 3 * 256 * 1024 && table_bytes(10, 1, 1) == 256 * 1024, "small n");
  for (int log_n = 17; log_n <= 27; ++log_n)
    for (const size_t m : {(size_t)1, (size_t)7, (size_t)1 << 20}) {
      EXPECT(table_bytes(log_n, m, -1) == (size_t)512 * 256 * 1024 && table_bytes(log_n, m, 1) == 256 * 1024, "the grid sets the tables");
      EXPECT(log_n < 20 || table_bytes(log_n, m, 5000) == (size_t)4096 * 256 * 1024, "a pin above 4096 is 4096");
    }
  // scratch = tables + 32 bytes per twiddle (n of 2n points, n / 2 of n) + two buffers of 192 n m bytes
  EXPECT(scratch_bytes(3, 1, -1) == 262144 + 32 * 12 + 2 * 1536, "log_n 3: %zu", scratch_bytes(3, 1, -1));
  EXPECT(scratch_bytes(1, 2, -1) == 262144 + 32 * 3 + 2 * 768, "log_n 1: %zu", scratch_bytes(1, 2, -1));
  EXPECT(scratch_bytes(20, 1, -1) == (size_t)134217728 + 48 * 1048576 + 2 * 201326592, "log_n 20: %zu", scratch_bytes(20, 1, -1));
  EXPECT(table_xy_bytes(3) == 1024 && fr_bytes(3, 2) == 512 && pi_xy_bytes(3, 2) == 1024, "the caller's arrays");
  // saturation: 2 * 2^27 * m wraps 64 bits from m = 2^36 on, the bytes earlier
  EXPECT(stride(27, (size_t)1 << 36) == SAT && stride(27, ((size_t)1 << 36) - 1) != SAT && first_items(27, (size_t)1 << 37) == SAT, "columns saturate");
  EXPECT(buffer_words(27, (size_t)1 << 33) == SAT && scratch_bytes(27, (size_t)1 << 33, -1) == SAT && scratch_bytes(27, (size_t)1 << 29, 1) == SAT, "scratch saturates");
  EXPECT(scratch_bytes(27, (size_t)1 << 28, -1) != SAT && scratch_bytes(27, (size_t)1 << 28, -1) > SAT / 2, "2 * 192 * 2^55 bytes fit 64 bits and are refused by their size");
  EXPECT(fr_bytes(27, (size_t)1 << 32) == SAT && pi_xy_bytes(27, (size_t)1 << 31) == SAT && fr_bytes(27, 1) == (size_t)1 << 32, "bytes saturate");
  EXPECT(first_grid(27, (size_t)1 << 40, -1) == 512 && fwd_grid(27, (size_t)1 << 40, 2) == 2, "a saturated count still has a grid");
  EXPECT(disjoint(1000, 64, 1064, 8) && disjoint(1064, 8, 1000, 64) && !disjoint(1000, 64, 1063, 8) && !disjoint(1007, 8, 1000, 64) && !disjoint(1000, 64, 1000, 64), "ranges");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {
    const PrepareLayout l = prepare_layout(2);
    const Region r[] = {WORDS(l, xy, 64), BYTES(l, inf, 8)};
    EXPECT(layout_ok("prepare", r, l.bytes) && l.inf == 512 && l.bytes == 520 && prepare_layout(0).inf == 128 && prepare_layout(0).bytes == 130 && prepare_layout(60).bytes == SAT,
           "prepare: %zu", l.bytes);
  }
  {  // n = 4, 3 polynomials: one block of lanes, 256 KB of tables FIRST; the twiddles of 8 and of 4 points on the bytes behind them; P and F inside buffer 1
    const ScratchLayout l = scratch_layout(2, 3, -1);
    const Region r[] = {BYTES(l, tables, 262144), WORDS(l, tw_wide, 16), WORDS(l, tw, 8), WORDS(l, buf[0], 288), WORDS(l, buf[1], 288)};
    EXPECT(layout_ok("open", r, l.bytes) && l.tw_wide == 262144 && l.tw == 262272 && l.buf[0] == 262336 && l.buf[1] == 264640 && l.bytes == 266944, "open: %zu", l.bytes);
    EXPECT(l.padded == 264640 && l.f == 265408 && l.f + 96 * 8 <= l.bytes, "P and F: %zu %zu", l.padded, l.f);
  }
  {
    const ScratchLayout l = scratch_layout(1, 1, -1);
    const Region r[] = {BYTES(l, tables, 262144), WORDS(l, tw_wide, 8), WORDS(l, tw, 4), WORDS(l, buf[0], 48), WORDS(l, buf[1], 48)};
    EXPECT(layout_ok("open n = 2", r, l.bytes) && l.tw == 262208 && l.buf[0] == 262240 && l.buf[1] == 262624 && l.bytes == 263008 && l.padded == 262624 && l.f == 262752,
           "n = 2: %zu", l.bytes);
  }
  EXPECT(scratch_layout(0, 5, -1).bytes == 0 && scratch_layout(27, (size_t)1 << 40, -1).bytes == SAT, "n = 1 leases nothing; saturates");
  for (const long long pin : {-1ll, 1ll, 7ll, 4096ll, 1ll << 40}) EXPECT(table_bytes(10, 3, pin) % 1024 == 0, "the tables are whole KB: pin %lld", pin);
}

int main() {
  for (int log_n = 1; log_n <= 10; ++log_n)
    for (const long long pin : PINS) whole_call(log_n, log_n <= 8 ? 3 : 1, pin);
  for (int log_n = 11; log_n <= OPEN_ALL_LOG_N_MAX; ++log_n) probes(log_n);
  table_of_x();
  sizes_tables_and_scratch();
  layouts();
  if (fails) {
    printf("%d of %zu checks FAILED\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
