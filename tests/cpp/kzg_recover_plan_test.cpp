// CPU-only check of the planner of the cell recovery (sylow_amd/csrc/kzg_recover_plan.hpp): the limits on (log_c, log_l), the items, grids and
// LDS bytes of the four kernels at c = 1, at BLOCK - 1, BLOCK and BLOCK + 1 items, at the largest shapes and where size_t overflows, both
// layouts of the vanishing values, every index of every kernel inside its array, and the scratch of a call with its regions laid end to
// end.  Expected values are written out by hand from the rules in the header's comments (blocks of 256 lanes, 2^20 blocks at most, a
// staging round of 256 mask bytes, 8 elements per lane of the status kernel).  Built with -fsanitize=address,undefined by
// tests/test_kzg_recover_plan.py: host code only.
#include "../../sylow_amd/csrc/kzg_recover_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace kzg_recover_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static const size_t TOP = SIZE_MAX, M20 = (size_t)1 << 20;

static void limits() {
  EXPECT(RECOVER_BLOCK == 256 && RECOVER_WAVE == 64 && RECOVER_WAVES == 4 && RECOVER_LOG_C_MAX == 12 && RECOVER_LOG_N_MAX == 27 && RECOVER_COSET_SHIFT == 5, "constants");
  EXPECT(!logs_ok(0, 0), "a domain of one point has no polynomial of degree below 1/2");
  EXPECT(logs_ok(1, 0) && logs_ok(0, 1) && logs_ok(12, 0) && logs_ok(12, 15) && logs_ok(0, 27) && logs_ok(7, 6), "the legal corners");
  EXPECT(!logs_ok(13, 0) && !logs_ok(12, 16) && !logs_ok(0, 28) && !logs_ok(-1, 5) && !logs_ok(5, -1) && !logs_ok(-1, 2) && !logs_ok(2, -1), "the illegal ones");
  EXPECT(!logs_ok(INT32_MAX, 0) && !logs_ok(0, INT32_MAX) && !logs_ok(INT32_MIN, 1), "no overflow in the sum");
  EXPECT(max_missing(0) == 0 && max_missing(1) == 1 && max_missing(2) == 2 && max_missing(7) == 64 && max_missing(12) == 2048, "c / 2 rounded down");
  EXPECT(mul_sat(TOP, 2) == SAT && mul_sat(0, TOP) == 0 && add_sat(TOP, 1) == SAT && add_sat(1, 2) == 3, "saturating arithmetic");
  EXPECT(disjoint(0, 8, 8, 8) && disjoint(8, 8, 0, 8) && !disjoint(0, 9, 8, 8) && !disjoint(8, 8, 0, 9) && !disjoint(4, 1, 0, 8), "byte ranges");
}

static void callers_arrays() {
  EXPECT(fr_bytes(2, 2, 2) == 1024 && fr_bytes(7, 6, 1) == 262144 && fr_bytes(12, 15, 1) == (size_t)1 << 32, "32 n m bytes");
  EXPECT(fr_bytes(12, 15, (size_t)1 << 32) == SAT && fr_bytes(1, 0, TOP) == SAT && fr_bytes(1, 0, 0) == 0, "32 n m bytes at the ends");
  EXPECT(present_bytes(7, 3) == 384 && present_bytes(0, 5) == 5 && present_bytes(12, TOP) == SAT, "c m bytes");
  EXPECT(z_bytes(7, 3) == 12288 && z_bytes(0, 1) == 32 && z_bytes(12, TOP / 4096) == SAT, "32 c m bytes");
  EXPECT(status_bytes(7) == 7, "m bytes");
}

static void roots() {
  EXPECT(root_words(0) == 0 && root_words(1) == 4 && root_words(2) == 8 && root_words(12) == 8192, "[4][c / 2], none at c = 1");
  EXPECT(!root_negated(0, 0) && root_slot(0, 0) == 0, "c = 1 has the root 1 and no table");
  EXPECT(!root_negated(0, 1) && root_negated(1, 1) && root_slot(1, 1) == 0, "c = 2: v = -1");
  for (int log_c = 1; log_c <= RECOVER_LOG_C_MAX; ++log_c) {
    const size_t c = elems(log_c), half = c / 2;
    bool ok = true;
    for (size_t i = 0; i < c; ++i) ok = ok && root_slot(i, log_c) < half && root_slot(i, log_c) == i % half && root_negated(i, log_c) == (i >= half);
    EXPECT(ok, "every slot inside the table of c / 2 at log_c = %d", log_c);
  }
  EXPECT(CONST_SHIFT == 0 && CONST_SL == 4 && CONST_WORDS == 8, "two values of four words");
}

static void vanish_kernel() {
  EXPECT(VANISH_CHUNK == 256 && vanish_lds_bytes() == 8208, "256 roots of 32 bytes and four counts: %zu", vanish_lds_bytes());
  // {log_c, lanes per k, values of k per block, blocks of a row, staging rounds}: 16 lanes per k from 32 cells on
  const size_t rb[][5] = {{0, 1, 256, 1, 1}, {1, 1, 256, 1, 1}, {4, 1, 256, 1, 1}, {5, 16, 16, 2, 1}, {7, 16, 16, 8, 1}, {8, 16, 16, 16, 1}, {9, 16, 16, 32, 2}, {10, 16, 16, 64, 4},
                          {12, 16, 16, 256, 16}};
  for (const auto& r : rb) {
    const int lc = (int)r[0];
    EXPECT(((size_t)1 << vanish_split_log(lc)) == r[1] && vanish_block_ks(lc) == r[2] && vanish_row_blocks(lc) == r[3] && vanish_rounds(lc) == r[4],
           "log_c = %d: %zu values per block, %zu blocks of a row, %zu rounds", lc, vanish_block_ks(lc), vanish_row_blocks(lc), vanish_rounds(lc));
  }
  EXPECT(vanish_items(0, 1) == 1 && vanish_items(4, 255) == 255 && vanish_items(8, 255) == 4080 && vanish_items(9, 3) == 96 && vanish_items(12, 5) == 1280 &&
             vanish_items(12, TOP) == SAT, "(row, block) pairs");
  EXPECT(vanish_lane_k(0, 4) == 0 && vanish_lane_k(255, 4) == 255 && vanish_lane_sub(255, 4) == 0, "a lane per k below 32 cells");
  EXPECT(vanish_lane_k(15, 7) == 0 && vanish_lane_k(16, 7) == 1 && vanish_lane_k(255, 7) == 15 && vanish_lane_sub(15, 7) == 15 && vanish_lane_sub(16, 7) == 0 &&
             vanish_lane_sub(63, 7) == 15 && vanish_lane_k(63, 7) == 3 && vanish_lane_k(64, 7) == 4, "16 adjacent lanes per k: no k straddles a wave of 64");
  EXPECT(vanish_grid(4, 1) == 1 && vanish_grid(4, M20 - 1) == M20 - 1 && vanish_grid(4, M20) == M20 && vanish_grid(4, M20 + 1) == M20 && vanish_grid(7, 3) == 24 &&
             vanish_grid(7, M20 / 8) == M20 && vanish_grid(12, TOP) == M20,
         "a block per item up to the cap");
  EXPECT(vanish_row(0, 9) == 0 && vanish_k0(0, 9) == 0 && vanish_row(1, 9) == 0 && vanish_k0(1, 9) == 16 && vanish_row(37, 9) == 1 && vanish_k0(37, 9) == 80, "item -> (row, first k)");
  EXPECT(vanish_row(5, 4) == 5 && vanish_k0(5, 4) == 0 && vanish_row(5, 7) == 0 && vanish_k0(5, 7) == 80 && vanish_row(8, 7) == 1 && vanish_k0(8, 7) == 0, "blocks of a row");
  for (int log_c : {0, 3, 5, 8, 9, 12}) {                    // every (row, k) of a batch is stored by one lane of one item
    const size_t m = 3, c = elems(log_c);
    std::vector<int> seen(m * c, 0);
    for (size_t item = 0; item < vanish_items(log_c, m); ++item)
      for (size_t t = 0; t < (size_t)RECOVER_BLOCK; ++t) {
        const size_t k = vanish_k0(item, log_c) + vanish_lane_k(t, log_c);
        if (k < c && vanish_lane_sub(t, log_c) == 0) ++seen[vanish_row(item, log_c) * c + k];
      }
    bool once = true;
    for (int s : seen) once = once && s == 1;
    EXPECT(once, "log_c = %d", log_c);
    bool covered = true;                                     // the rounds see every mask byte once
    std::vector<int> mask(c, 0);
    for (size_t round = 0; round < vanish_rounds(log_c); ++round)
      for (size_t t = 0; t < VANISH_CHUNK; ++t)
        if (round * VANISH_CHUNK + t < c) ++mask[round * VANISH_CHUNK + t];
    for (int s : mask) covered = covered && s == 1;
    EXPECT(covered, "log_c = %d", log_c);
  }
  EXPECT(vanish_products(12, 2048) == (size_t)1 << 24 && vanish_products(7, 64) == 16384 && vanish_products(3, 0) == 0, "2 c |M| products per row");
}

static void z_layouts() {
  // the caller's [m][4][c]: word w of (row, k) at ((row 4 + w) c + k); the call's own [4][m c]: at w m c + row c + k
  for (int log_c : {0, 3, 9}) {
    const size_t m = 3, c = elems(log_c);
    bool ok = true;
    std::vector<int> a(z_words(log_c, m), 0), b(z_words(log_c, m), 0);
    for (size_t row = 0; row < m; ++row)
      for (size_t k = 0; k < c; ++k)
        for (size_t w = 0; w < 4; ++w) {
          const size_t ia = z_row_off(row, log_c, false) + w * z_word_stride(log_c, m, false) + k, ib = z_row_off(row, log_c, true) + w * z_word_stride(log_c, m, true) + k;
          ok = ok && ia == (row * 4 + w) * c + k && ib == w * m * c + row * c + k && ia < a.size() && ib < b.size();
          if (ia < a.size()) ++a[ia];
          if (ib < b.size()) ++b[ib];
        }
    for (size_t i = 0; i < a.size(); ++i) ok = ok && a[i] == 1 && b[i] == 1;
    EXPECT(ok, "both layouts fill their 4 c m words once at log_c = %d", log_c);
  }
  EXPECT(z_words(7, 64) == 32768 && inv_elems(7, 64) == 8192 && z_words(12, TOP) == SAT && inv_elems(12, TOP) == SAT, "words and elements of the packed array");
}

static void element_kernels() {
  EXPECT(elem_items(2, 2, 2) == 32 && elem_items(12, 15, 2) == (size_t)1 << 28 && elem_items(1, 0, TOP) == SAT, "m n elements");
  const size_t g[][4] = {{1, 0, 1, 1}, {7, 0, 1, 1}, {7, 1, 1, 1}, {4, 4, 1, 1}, {8, 0, 1, 1}, {8, 0, 2, 2}, {4, 4, 17, 17}, {14, 14, 2, M20}, {14, 13, 2, M20}, {14, 13, 1, M20 / 2}};
  for (const auto& e : g) EXPECT(elem_grid((int)e[0], (int)e[1], e[2]) == e[3], "elem_grid(%zu, %zu, %zu) = %zu", e[0], e[1], e[2], elem_grid((int)e[0], (int)e[1], e[2]));
  EXPECT(elem_grid(1, 0, TOP) == M20 && blocks_of(0) == 0 && blocks_of(TOP) == TOP / 256 + 1, "no wrap at the top");
  EXPECT(elem_grid(3, 5, 1) == 1 && elem_grid(3, 5, 2) == 2, "255 + 1 and 256 + 256 items");
  EXPECT((elem_items(0, 8, 1) - 1 + 255) / 256 == 1 && elem_grid(0, 8, 1) == 1 && elem_grid(0, 1, 129) == 2, "BLOCK and BLOCK + 2 items");
  for (int log_c : {0, 2, 5})
    for (int log_l : {0, 1, 3}) {
      if (!logs_ok(log_c, log_l)) continue;
      const size_t m = 3, n = elems(log_c + log_l);
      bool ok = true;
      for (size_t t = 0; t < elem_items(log_c, log_l, m); ++t) {
        const size_t row = elem_row(t, log_c, log_l), col = elem_col(t, log_c, log_l);
        ok = ok && row < m && col < n && row * n + col == t && elem_cell(col, log_c) == col % elems(log_c);
      }
      EXPECT(ok, "(%d, %d)", log_c, log_l);
    }
}

static void status_kernel() {
  EXPECT(STATUS_LANE_ELEMS == 8 && STATUS_CHUNK == 2048 && status_lds_bytes() == 16, "a block reads 2048 elements");
  EXPECT(status_half(1, 0) == 1 && status_half(7, 6) == 4096 && status_half(12, 15) == (size_t)1 << 26, "n / 2");
  EXPECT(status_row_chunks(1, 0) == 1 && status_row_chunks(6, 6) == 1 && status_row_chunks(7, 6) == 2 && status_row_chunks(6, 6) * STATUS_CHUNK == status_half(6, 6), "chunks of a row");
  EXPECT(status_row_chunks(12, 15) == 32768 && status_items(12, 15, 3) == 98304 && status_items(12, 15, TOP) == SAT, "the largest rows");
  EXPECT(status_grid(1, 0, 5) == 5 && status_grid(12, 15, 32) == M20 && status_grid(12, 15, 33) == M20 && status_grid(12, 15, TOP) == M20, "a block per item up to the cap");
  EXPECT(status_close_grid(1) == 1 && status_close_grid(255) == 1 && status_close_grid(256) == 1 && status_close_grid(257) == 2 && status_close_grid(TOP) == M20, "a lane per row");
  for (int L : {1, 2, 11, 12, 13}) {                         // every element of the upper half is read once, none below it or past the row
    const size_t half = elems(L) / 2;
    std::vector<int> seen(half, 0);
    bool inside = true;
    for (size_t chunk = 0; chunk < status_row_chunks(L, 0); ++chunk)
      for (size_t t = 0; t < (size_t)RECOVER_BLOCK; ++t)
        for (int e = 0; e < STATUS_LANE_ELEMS; ++e) {
          const size_t k = chunk * STATUS_CHUNK + t + (size_t)e * RECOVER_BLOCK;
          if (k < half) ++seen[k];
        }
    for (int s : seen) inside = inside && s == 1;
    EXPECT(inside, "log_n = %d", L);
  }
  EXPECT(flag_words(0) == 1 && flag_words(1) == 1 && flag_words(2) == 2 && flag_words(3) == 2 && flag_words(5) * 8 >= 5 * 4, "u32 [m] in whole words");
  for (size_t m = 1; m < 40; ++m) EXPECT(flag_words(m) * 8 >= m * 4, "m = %zu", m);
}

static void scratch() {
  EXPECT(vanish_scratch_words(0) == 8 && vanish_scratch_words(1) == 12 && vanish_scratch_words(12) == 8200 && vanish_scratch_bytes(12) == 65600, "the constants and the roots");
  EXPECT(buffer_words(2, 2, 2) == 128 && buffer_words(12, 15, TOP) == SAT, "[m][4][n]");
  // (2, 2), m = 2: 8 + 8 roots, 3 x 32 packed words, 2 flag words, 128 buffer words
  EXPECT(recover_scratch_words(2, 2, 2) == 8 + 8 + 96 + 2 + 128 && recover_scratch_bytes(2, 2, 2) == 242 * 8, "%zu", recover_scratch_words(2, 2, 2));
  EXPECT(recover_scratch_words(0, 1, 1) == 8 + 0 + 12 + 1 + 8, "c = 1: %zu", recover_scratch_words(0, 1, 1));
  EXPECT(recover_scratch_words(7, 6, 64) == 8 + 256 + 3 * 32768 + 33 + 2097152, "a batch of real blobs: %zu", recover_scratch_words(7, 6, 64));
  EXPECT(recover_scratch_words(12, 15, 1) == 8 + 8192 + 3 * 16384 + 1 + ((size_t)1 << 29), "the largest row: %zu", recover_scratch_words(12, 15, 1));
  EXPECT(recover_scratch_bytes(12, 15, TOP) == SAT && recover_scratch_bytes(12, 15, (size_t)1 << 32) == SAT && recover_scratch_bytes(1, 0, TOP / 8) == SAT, "size_t overflow");
  EXPECT(scratch_ok(0) && scratch_ok(TOP / 2) && !scratch_ok(TOP / 2 + 1) && !scratch_ok(SAT), "refused before the lease");
  EXPECT(!scratch_ok(recover_scratch_bytes(12, 15, (size_t)1 << 31)) && scratch_ok(recover_scratch_bytes(12, 15, 4)), "a request the machine may refuse, and one no machine serves");
  EXPECT(transforms(false) == 3 && transforms(true) == 4, "the floor of a call");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // a layout of the cells alone: log_c <= 12, so nothing here can saturate
    const VanishLayout l = vanish_layout(3);
    const Region r[] = {WORDS(l, consts, 8), WORDS(l, roots, 16)};
    EXPECT(layout_ok("vanish", r, l.bytes) && l.roots == 64 && l.bytes == 192 && vanish_layout(0).roots == 64 && vanish_layout(0).bytes == 64, "vanish: %zu", l.bytes);
  }
  {  // c = 8, l = 4, 3 rows: the u32 flags of 3 rows in 2 words
    const RecoverLayout l = recover_layout(3, 2, 3);
    const Region r[] = {WORDS(l, v.consts, 8), WORDS(l, v.roots, 16), WORDS(l, zd, 96), WORDS(l, zc, 96), WORDS(l, zci, 96), WORDS(l, flags, 2), WORDS(l, buf, 384)};
    EXPECT(layout_ok("recover", r, l.bytes) && l.v.roots == 64 && l.zd == 192 && l.zc == 960 && l.zci == 1728 && l.flags == 2496 && l.buf == 2512 && l.bytes == 5584,
           "recover: %zu", l.bytes);
  }
  {  // c = 1, l = 2, one row: no roots
    const RecoverLayout l = recover_layout(0, 1, 1);
    const Region r[] = {WORDS(l, v.consts, 8), WORDS(l, v.roots, 0), WORDS(l, zd, 4), WORDS(l, zc, 4), WORDS(l, zci, 4), WORDS(l, flags, 1), WORDS(l, buf, 8)};
    EXPECT(layout_ok("recover of one", r, l.bytes) && l.zd == 64 && l.zc == 96 && l.zci == 128 && l.flags == 160 && l.buf == 168 && l.bytes == 232, "one row: %zu", l.bytes);
    EXPECT(recover_layout(3, 2, SIZE_MAX / 2).bytes == SAT, "saturates");
  }
}

int main() {
  limits();
  callers_arrays();
  roots();
  vanish_kernel();
  z_layouts();
  element_kernels();
  status_kernel();
  scratch();
  layouts();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
