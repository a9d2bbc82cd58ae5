// CPU-only check of the planner of the KZG proofs on every coset of the domain (sylow_amd/csrc/kzg_cosets_plan.hpp).  For every
// (log_c, log_l) with log_c >= 1 and log_c + log_l <= 9 it walks the call the way kzg_cosets.hip launches it -- the split, the fused first
// stage under every legal planes_log, the fold, the inverse stages from 1 on with the indices of g1_ntt_plan.hpp, the first stage of the
// forward transform of c points, its stages, the closing kernel -- with max_blocks in {1, 3, default}, lanes of the grid and a grid stride.
// It keeps, per column of the plane buffer and of each ping-pong buffer, the step that wrote it last: every index is in range, every step
// writes each of its columns once, the residue slices partition 0 .. l - 1, every read meets what the step before wrote, and the ping-pong
// ends in the buffer the closing kernel reads.  Then: the columns of x^(a) each SRS point goes to, the split's sources, the twist's items,
// the default plane rule, sums that saturate, and window tables that depend on the grid.  Expected values are written out from the rules in
// the header's comments.  Built with -fsanitize=address,undefined by tests/test_kzg_cosets_plan.py: host code only.
#include "../../sylow_amd/csrc/kzg_cosets_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace kzg_cosets_plan;
namespace g1 = g1_ntt_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; if (fails < 40) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)
#include "layout_check.hpp"

static const long long PINS[] = {1, 3, -1};

struct Columns {                       // the step that wrote each column last (0: never)
  std::vector<int> col;
  bool read(size_t c, int step) const { return c < col.size() && col[c] == step; }
  bool write(size_t c, int step) {
    if (c >= col.size() || col[c] == step) return false;             // out of range, or written twice by this step
    col[c] = step;
    return true;
  }
  size_t written(int step) const {
    size_t k = 0;
    for (const int v : col) k += v == step;
    return k;
  }
};

// a stage >= 1 of g1_ntt.hip as g1ntth::stage launches it: arrays of 2^log points at columns a 2^log of buffers of the call's stride
static void walk_stage(Columns* B, int log, int stage, size_t m, long long pin, int src, int dst, int step, size_t& mults) {
  const size_t total = g1::butterflies(log, m), lanes = g1::stage_grid(log, m, pin) * g1::G1_NTT_BLOCK, hn = g1::half(log);
  for (size_t t = 0; t < lanes; ++t)
    for (size_t b = t; b < total; b += lanes) {
      const size_t a = b >> (log - 1), j = g1::butterfly_of(b & (hn - 1), log, stage), base = a << log;
      EXPECT(B[src].read(base + g1::in0(j), step - 1) && B[src].read(base + g1::in1(j, log), step - 1), "log %d stage %d item %zu reads what step %d wrote", log, stage, b, step - 1);
      EXPECT(B[dst].write(base + g1::out0(j, stage), step) && B[dst].write(base + g1::out1(j, stage), step), "log %d stage %d item %zu writes once", log, stage, b);
      if (!g1::unit_twiddle(j, stage)) ++mults;
    }
  EXPECT(B[dst].written(step) == m << log, "log %d stage %d: every column of every array written", log, stage);
}

static void whole_call(int log_c, int log_l, size_t m, long long pin, int planes_log) {
  const size_t c = elems(log_c), l = elems(log_l), cc = wide(log_c), n = elems(log_n(log_c, log_l)), str = stride(log_c, m);
  const int L = wide_log(log_c), pl = planes_log_of(planes_log, log_c, log_l, m, pin);
  EXPECT(planes_log_ok(planes_log, log_l) && pl >= 0 && pl <= log_l && (planes_log < 0 || pl == planes_log), "planes_log %d of log_l %d", planes_log, log_l);
  EXPECT(str == m * cc && n == c * l, "stride");
  // the split: every word of [m l][4][2c] written once, consecutive items at consecutive words, sources inside the polynomial
  {
    const size_t total = split_items(log_c, log_l, m);
    std::vector<int> seen(total, 0), src(m * n, 0);
    EXPECT(total == m * l * cc && split_words(log_c, log_l, m) == 4 * total && rows(log_l, m) == m * l, "the split's items");
    for (size_t i = 0; i < total; ++i) {
      const size_t row = split_row(i, log_c), k = split_col(i, log_c), A = split_poly(row, log_l), a = split_residue(row, log_l);
      EXPECT(row * cc + k == i && row < m * l && A < m && a < l && fr_row(A, a, log_l) == row, "item %zu is word %zu of row %zu", i, k, row);
      ++seen[row * cc + k];
      if (split_is_zero(k, log_c)) { EXPECT(k >= c, "the upper half is zero"); continue; }
      const size_t s = split_src(a, k, log_l);
      EXPECT(k < c && s == a + l * k && s < n, "P^(a)_k = f_(a + l k)");
      ++src[A * n + s];
    }
    size_t once = 0, read_once = 0;
    for (const int v : seen) once += v == 1;
    for (const int v : src) read_once += v == 1;
    EXPECT(once == total && read_once == m * n, "every word written once, every coefficient read once");
  }
  Columns P, B[2];
  B[0].col.assign(str, 0);
  B[1].col.assign(str, 0);
  P.col.assign(folds(pl) ? plane_stride(log_c, m, pl) : 0, 0);
  EXPECT(plane_words(log_c, m, pl) == 12 * P.col.size() && plane_arrays(m, pl) == m << pl, "the plane buffer");
  size_t mults = 0;
  int step = 1;
  // the fused stage: table and F indices below 2c, the slices partition the residues, both outputs in range, each once
  {
    const size_t total = first_items(log_c, m, pl), lanes = first_grid(log_c, m, pl, pin) * g1::G1_NTT_BLOCK, planes = elems(pl);
    Columns& D = folds(pl) ? P : B[oa::inv_dst(0)];
    const size_t dstr = folds(pl) ? plane_stride(log_c, m, pl) : str;
    EXPECT(total == (m * c) << pl && lanes * g1::G1_NTT_TABLE_BYTES_PER_LANE == table_bytes(log_c, m, pl, pin) && dstr == D.col.size(), "the fused stage's lanes have tables");
    std::vector<int> owner(l, -1);
    for (size_t p = 0; p < planes; ++p)
      for (size_t a = slice_begin(p, log_l, pl); a < slice_begin(p, log_l, pl) + slice_len(log_l, pl); ++a) {
        EXPECT(a < l && owner[a] == -1, "residue %zu has one plane", a);
        if (a < l) owner[a] = (int)p;
      }
    for (size_t a = 0; a < l; ++a) EXPECT(owner[a] >= 0, "residue %zu has a plane", a);
    for (size_t t = 0; t < lanes; ++t)
      for (size_t b = t; b < total; b += lanes) {
        const size_t arr = first_array(b, log_c), j = first_butterfly(b, log_c), p = first_plane(arr, m), A = first_poly(arr, m);
        EXPECT(arr == p * m + A && p < planes && A < m && j < c && arr * c + j == b, "item %zu is (plane %zu, polynomial %zu, butterfly %zu)", b, p, A, j);
        EXPECT(first_in0(j) == j && first_in1(j, log_c) == j + c && first_in1(j, log_c) < cc, "table and F columns of item %zu", b);
        const size_t a1 = slice_begin(p, log_l, pl) + slice_len(log_l, pl);
        EXPECT((fr_row(A, a1 - 1, log_l) + 1) * cc * FR_WORDS <= split_words(log_c, log_l, m) && a1 <= l, "F of polynomial %zu, table of residue %zu", A, a1 - 1);
        EXPECT(first_out0(arr, j, log_c) == arr * cc + 2 * j && first_out1(arr, j, log_c) == arr * cc + 2 * j + 1, "outputs of item %zu", b);
        EXPECT(D.write(first_out0(arr, j, log_c), step) && D.write(first_out1(arr, j, log_c), step), "fused item %zu writes once", b);
        mults += 2 * slice_len(log_l, pl);
      }
    EXPECT(D.written(step) == dstr, "the fused stage writes every column");
  }
  if (folds(pl)) {
    const size_t total = fold_items(log_c, m), lanes = fold_grid(log_c, m, pin) * g1::G1_NTT_BLOCK;
    std::vector<int> reads(P.col.size(), 0);
    EXPECT(total == str, "the fold has one item per column");
    for (size_t t = 0; t < lanes; ++t)
      for (size_t q = t; q < total; q += lanes) {
        for (size_t p = 0; p < elems(pl); ++p) {
          const size_t i = fold_in(q, p, log_c, m);
          EXPECT(P.read(i, step) && i == p * str + q, "fold item %zu reads plane %zu", q, p);
          if (i < reads.size()) ++reads[i];
        }
        EXPECT(B[oa::inv_dst(0)].write(q, step), "fold item %zu writes once", q);
      }
    size_t once = 0;
    for (const int v : reads) once += v == 1;
    EXPECT(once == P.col.size() && B[oa::inv_dst(0)].written(step) == str, "every plane column read once, every column written");
  }
  for (int s = 1; s < oa::inv_stages(log_c); ++s) {
    ++step;
    EXPECT(oa::inv_src(s) == oa::inv_dst(s - 1) && oa::inv_src(s) != oa::inv_dst(s), "inverse stage %d reads what stage %d wrote", s, s - 1);
    EXPECT(g1::stage_grid(L, m, pin) <= first_grid(log_c, m, pl, pin), "an inverse stage's lanes have tables");
    walk_stage(B, L, s, m, pin, oa::inv_src(s), oa::inv_dst(s), step, mults);
  }
  EXPECT(oa::fwd_src(log_c, 0) == oa::inv_dst(oa::inv_stages(log_c) - 1), "h lies where the last inverse stage wrote");
  {
    const int src = oa::fwd_src(log_c, 0), dst = oa::fwd_dst(log_c, 0), before = step;
    ++step;
    const size_t total = oa::fwd_items(log_c, m), lanes = oa::fwd_grid(log_c, m, pin) * g1::G1_NTT_BLOCK, hn = g1::half(log_c);
    size_t identities = 0;
    for (size_t t = 0; t < lanes; ++t)
      for (size_t b = t; b < total; b += lanes) {
        const size_t a = b >> (log_c - 1), j = b & (hn - 1), i0 = oa::fwd_in0(a, j, log_c), i1 = oa::fwd_in1(a, j, log_c);
        EXPECT(a < m && i0 >= a * cc && i0 < a * cc + c && i1 >= a * cc && i1 < a * cc + c && i0 != i1, "item %zu reads the first c columns of array %zu", b, a);
        EXPECT(B[src].read(i0, before) && B[src].read(i1, before), "item %zu reads what the inverse transform wrote", b);
        EXPECT(oa::fwd_in1_is_identity(j, log_c) == (i1 == a * cc + c - 1), "h_(c-1) is V of the last butterfly alone");
        identities += oa::fwd_in1_is_identity(j, log_c);
        EXPECT(B[dst].write(oa::fwd_out0(a, j, log_c), step) && B[dst].write(oa::fwd_out1(a, j, log_c), step) && oa::fwd_out1(a, j, log_c) < m * c, "forward item %zu writes once", b);
      }
    EXPECT(src != dst && identities == m && B[dst].written(step) == m * c, "one identity per array, every column of the arrays of c written");
  }
  for (int s = 1; s < oa::fwd_stages(log_c); ++s) {
    ++step;
    EXPECT(oa::fwd_src(log_c, s) == oa::fwd_dst(log_c, s - 1) && oa::fwd_src(log_c, s) != oa::fwd_dst(log_c, s), "forward stage %d reads what stage %d wrote", s, s - 1);
    EXPECT(g1::stage_grid(log_c, m, pin) <= first_grid(log_c, m, pl, pin), "a forward stage's lanes have tables");
    walk_stage(B, log_c, s, m, pin, oa::fwd_src(log_c, s), oa::fwd_dst(log_c, s), step, mults);
  }
  EXPECT(oa::close_src(log_c) == oa::fwd_dst(log_c, oa::fwd_stages(log_c) - 1) && oa::close_src(log_c) == 0, "the closing kernel reads the last stage's buffer");
  const size_t lanes = g1::closing_grid(log_c, m, pin) * g1::G1_NTT_BLOCK;
  for (size_t t = 0; t < lanes; ++t)
    for (size_t i = t; i < g1::points(log_c, m); i += lanes) EXPECT(B[oa::close_src(log_c)].read(i, step), "closing item %zu reads the last stage's column", i);
  EXPECT(mults == m * multiplications(log_c, log_l), "(%d, %d): %zu multiplications against %zu", log_c, log_l, mults, m * multiplications(log_c, log_l));
  // the scratch holds what the launch code carves from it, in its order
  const size_t words = oa::wide_twiddle_words(log_c) + oa::twiddle_words(log_c) + 2 * 12 * str + 12 * P.col.size() + 2 * 4 * m * l * cc;
  EXPECT(scratch_bytes(log_c, log_l, m, pl, pin) == 8 * words + table_bytes(log_c, m, pl, pin), "scratch of (%d, %d)", log_c, log_l);
}

static void table_of_x() {
  for (int log_c = 0; log_c <= 6; ++log_c)
    for (int log_l = 0; log_l <= 4; ++log_l) {
      const size_t c = elems(log_c), l = elems(log_l), cc = wide(log_c), n = c * l;
      std::vector<int> used(n, 0);
      size_t identities = 0;
      for (size_t a = 0; a < l; ++a)
        for (size_t k = 0; k < cc; ++k) {
          const size_t t = x_srs_index(a, k, log_c, log_l);
          if (t == X_IDENTITY) { ++identities; EXPECT(k <= c, "columns 0 .. c hold the identity"); continue; }
          const size_t u = cc - 1 - k;
          EXPECT(u <= c - 2 && t == a + l * u && t < n - l && !used[t], "x^(a)_(2c-1-u) = s_(a + l u), u <= c - 2");
          used[t] = 1;
        }
      size_t count = 0;
      for (const int v : used) count += v;
      EXPECT(identities == l * (c + 1) && count == n - l, "s_0 .. s_(n-l-1) are used, each once");
      EXPECT(prepare_items(log_c, log_l) == l * cc && prepare_scratch_bytes(log_c, log_l) == 64 * l * cc + l * cc && table_xy_bytes(log_c, log_l) == 16 * 8 * n, "prepare");
      EXPECT(log_l != 0 || x_srs_index(0, cc - 1, log_c, 0) == oa::x_srs_index(cc - 1, log_c), "log_l = 0 is the table of every point");
    }
}

static void twist_and_rows() {
  for (int log_c = 0; log_c <= 5; ++log_c)
    for (int log_l = 0; log_l <= 9; ++log_l) {
      const size_t l = elems(log_l), n_rows = 5, q = elems(twist_lanes_log(log_l));
      EXPECT(q == (l < 64 ? l : 64) && twist_items(log_l, n_rows) == n_rows * q, "lanes of a row");
      std::vector<int> seen(n_rows * l, 0);
      for (size_t i = 0; i < twist_items(log_l, n_rows); ++i)
        for (size_t k = i & (q - 1); k < l; k += q) ++seen[(i >> twist_lanes_log(log_l)) * l + k];
      size_t once = 0;
      for (const int v : seen) once += v == 1;
      EXPECT(once == n_rows * l, "every coefficient of every row multiplied once");
      const uint64_t c = (uint64_t)1 << log_c, n = c << log_l;
      for (const uint64_t idx : {(uint64_t)0, (uint64_t)1, c - 1, c, c + 1, ~(uint64_t)0}) {
        const uint64_t i = idx % c;
        EXPECT(in_range(idx, log_c) == (idx < c) && coset_of(idx, log_c) == i, "idx %llu", (unsigned long long)idx);
        EXPECT(twist_exp(idx, log_c, log_l) == (n - i) % n && twist_exp(idx, log_c, log_l) < n && z_exp(idx, log_c, log_l) == i * l && z_exp(idx, log_c, log_l) < n, "exponents of idx %llu", (unsigned long long)idx);
      }
    }
  EXPECT(vals_bytes(4, 3) == 32 * 16 * 3 && reduce_scratch_bytes(4, 3) == 32 * 16 * 3 + 64 * 3 + 3 && verify_scratch_bytes(3) == 64 * 3 + 2 * 32 * 3 + 2 * 3, "scratch of the verifier's side");
  EXPECT(vals_bytes(27, (size_t)1 << 32) == SAT && reduce_scratch_bytes(27, (size_t)1 << 32) == SAT && verify_scratch_bytes((size_t)1 << 58) == SAT, "and it saturates");
}

static void rules_and_saturation() {
  EXPECT(COSETS_LOG_N_MAX == 27 && logs_ok(0, 0) && logs_ok(27, 0) && logs_ok(0, 27) && logs_ok(13, 14) && !logs_ok(14, 14) && !logs_ok(-1, 3) && !logs_ok(3, -1) && !logs_ok(28, 0) &&
         !logs_ok(0, 28) && !logs_ok(2147483647, 2147483647), "argument rules");
  EXPECT(planes_log_ok(-1, 0) && planes_log_ok(0, 0) && !planes_log_ok(1, 0) && planes_log_ok(4, 4) && !planes_log_ok(5, 4), "planes_log rules");
  EXPECT(trivial(0) && !trivial(1) && scratch_bytes(0, 7, 5, 0, -1) == 0, "log_c = 0 runs nothing of the plan");
  // the default planes: the smallest count that brings c m planes up to the resident lanes of the grid cap, at most l; a function of
  // (c, m, l, grid) alone
  EXPECT(resident_lanes(-1) == 512 * 256 && resident_lanes(3) == 3 * 256 && resident_lanes(100000) == 4096 * 256, "resident lanes");
  EXPECT(default_planes_log(10, 4, 1, -1) == 4 && default_planes_log(10, 6, 1, -1) == 6 && default_planes_log(10, 9, 1, -1) == 7, "2^10 butterflies want 2^7 planes, l permitting");
  EXPECT(default_planes_log(17, 4, 1, -1) == 0 && default_planes_log(16, 4, 1, -1) == 1 && default_planes_log(16, 4, 2, -1) == 0 && default_planes_log(16, 4, 3, -1) == 0, "c m fills the device");
  EXPECT(default_planes_log(8, 4, 16, -1) == 4 && default_planes_log(12, 4, 1, -1) == 4 && default_planes_log(12, 6, 1, -1) == 5 && default_planes_log(3, 0, 1, -1) == 0, "the measured shapes");
  EXPECT(default_planes_log(10, 4, 1, 1) == 0 && default_planes_log(6, 4, 1, 1) == 2 && default_planes_log(10, 4, 1, 4096) == 4, "it follows the grid cap");
  for (int log_c = 0; log_c <= 20; ++log_c)
    for (int log_l = 0; log_l <= 7; ++log_l)
      for (const size_t m : {(size_t)1, (size_t)3, (size_t)100}) {
        const int p = default_planes_log(log_c, log_l, m, -1);
        const size_t items = (m << log_c) << p;
        EXPECT(p >= 0 && p <= log_l && (p == log_l || items >= resident_lanes(-1)) && (p == 0 || items / 2 < resident_lanes(-1)), "the smallest count at (%d, %d, %zu)", log_c, log_l, m);
        EXPECT(planes_log_of(-1, log_c, log_l, m, -1) == p && planes_log_of(-7, log_c, log_l, m, -1) == p && planes_log_of(0, log_c, log_l, m, -1) == 0, "a negative pin is the default");
      }
  // tables: 1 KB per lane of the fused stage's grid
  EXPECT(table_bytes(10, 1, 0, -1) == 4 * 256 * 1024 && table_bytes(10, 1, 4, -1) == 64 * 256 * 1024 && table_bytes(10, 1, 7, -1) == (size_t)512 * 256 * 1024 && table_bytes(10, 1, 4, 3) == 3 * 256 * 1024, "tables");
  EXPECT(multiplications(0, 0) == 2 && multiplications(3, 0) == 38 && multiplications(10, 4) == 32768 + 9217 + 4097, "counts");
  EXPECT(fr_bytes(3, 2, 2) == 32 * 32 * 2 && pi_xy_bytes(3, 2) == 1024 && table_inf_bytes(3, 2) == 64, "the caller's arrays");
  // saturation
  EXPECT(stride(27, (size_t)1 << 36) == SAT && plane_stride(20, (size_t)1 << 40, 7) == SAT && first_items(20, (size_t)1 << 40, 7) == SAT, "columns saturate");
  EXPECT(split_items(20, 7, (size_t)1 << 40) == SAT && split_words(20, 7, (size_t)1 << 35) == SAT && scratch_words(20, 7, (size_t)1 << 35, 0) == SAT, "the split saturates");
  EXPECT(scratch_bytes(20, 7, (size_t)1 << 35, 0, -1) == SAT && scratch_bytes(20, 7, (size_t)1 << 32, 7, 1) == SAT, "scratch saturates");
  EXPECT(scratch_bytes(20, 7, (size_t)1 << 29, 0, -1) != SAT && scratch_bytes(20, 7, (size_t)1 << 29, 0, -1) > SAT / 2, "and what fits 64 bits is refused by its size");
  EXPECT(first_grid(20, (size_t)1 << 50, 7, -1) == 512 && fold_grid(27, (size_t)1 << 40, 2) == 2 && split_grid(20, 7, (size_t)1 << 50) == 512, "a saturated count still has a grid");
  EXPECT(fr_bytes(20, 7, (size_t)1 << 32) == SAT && table_xy_bytes(20, 7) == (size_t)1 << 34, "bytes");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // c = 4, l = 2: 2 arrays of 8 points, [2][8][8] words then 16 flags
    const PrepareLayout l = prepare_layout(2, 1);
    const Region r[] = {WORDS(l, xy, 128), BYTES(l, inf, 16)};
    EXPECT(layout_ok("prepare", r, l.bytes) && l.inf == 1024 && l.bytes == 1040, "prepare: %zu", l.bytes);
  }
  {
    const PrepareLayout l = prepare_layout(0, 0);
    const Region r[] = {WORDS(l, xy, 16), BYTES(l, inf, 2)};
    EXPECT(layout_ok("prepare of one", r, l.bytes) && l.inf == 128 && l.bytes == 130, "c = l = 1: %zu", l.bytes);
  }
  EXPECT(prepare_layout(60, 60).bytes == SAT, "saturates");
  {  // c = 2, l = 2, one polynomial, two planes: one block of lanes, 256 KB of tables FIRST; the twiddles of 4 and of 2 points behind them
    const ScratchLayout l = scratch_layout(1, 1, 1, 1, -1);
    const Region r[] = {BYTES(l, tables, 262144), WORDS(l, tw_wide, 8), WORDS(l, tw, 4), WORDS(l, buf[0], 48), WORDS(l, buf[1], 48), WORDS(l, planes, 96),
                        WORDS(l, padded, 32), WORDS(l, f, 32)};
    EXPECT(layout_ok("open, two planes", r, l.bytes) && l.tw_wide == 262144 && l.tw == 262208 && l.buf[0] == 262240 && l.buf[1] == 262624 && l.planes == 263008 &&
               l.padded == 263776 && l.f == 264032 && l.bytes == 264288, "two planes: %zu", l.bytes);
  }
  {  // one plane: the fused stage writes buffer 0 and there is no plane buffer
    const ScratchLayout l = scratch_layout(1, 1, 1, 0, -1);
    const Region r[] = {BYTES(l, tables, 262144), WORDS(l, tw_wide, 8), WORDS(l, tw, 4), WORDS(l, buf[0], 48), WORDS(l, buf[1], 48), WORDS(l, planes, 0),
                        WORDS(l, padded, 32), WORDS(l, f, 32)};
    EXPECT(layout_ok("open, one plane", r, l.bytes) && l.planes == 263008 && l.padded == 263008 && l.f == 263264 && l.bytes == 263520, "one plane: %zu", l.bytes);
  }
  EXPECT(scratch_layout(0, 3, 5, 0, -1).bytes == 0 && scratch_layout(0, 3, 5, 0, -1).f == 0, "c = 1 leases nothing");
  for (const long long pin : {-1ll, 1ll, 7ll, 4096ll, 1ll << 40}) EXPECT(table_bytes(10, 3, 2, pin) % 1024 == 0, "the tables are whole KB: pin %lld", pin);
  {
    const ReduceLayout l = reduce_layout(1, 3);
    const Region r[] = {WORDS(l, r, 24), WORDS(l, rc_xy, 24), BYTES(l, rc_inf, 3)};
    EXPECT(layout_ok("reduce", r, l.bytes) && l.rc_xy == 192 && l.rc_inf == 384 && l.bytes == 387, "reduce: %zu", l.bytes);
    const ReduceLayout one = reduce_layout(0, 1);
    const Region q[] = {WORDS(one, r, 4), WORDS(one, rc_xy, 8), BYTES(one, rc_inf, 1)};
    EXPECT(layout_ok("reduce of one", q, one.bytes) && one.rc_xy == 32 && one.rc_inf == 96 && one.bytes == 97 && reduce_layout(27, SIZE_MAX).bytes == SAT, "one row: %zu", one.bytes);
  }
  {
    const VerifyLayout l = verify_layout(3);
    const Region r[] = {WORDS(l, cred, 24), WORDS(l, z, 12), WORDS(l, y, 12), BYTES(l, cred_inf, 3), BYTES(l, in_rng, 3)};
    EXPECT(layout_ok("verify", r, l.bytes) && l.z == 192 && l.y == 288 && l.cred_inf == 384 && l.in_rng == 387 && l.bytes == 390, "verify: %zu", l.bytes);
    const VerifyLayout one = verify_layout(1);
    const Region q[] = {WORDS(one, cred, 8), WORDS(one, z, 4), WORDS(one, y, 4), BYTES(one, cred_inf, 1), BYTES(one, in_rng, 1)};
    EXPECT(layout_ok("verify of one", q, one.bytes) && one.z == 64 && one.y == 96 && one.cred_inf == 128 && one.bytes == 130 && verify_layout(SIZE_MAX).bytes == SAT, "one row: %zu",
           one.bytes);
  }
}

int main() {
  for (int log_c = 1; log_c <= 9; ++log_c)
    for (int log_l = 0; log_c + log_l <= 9; ++log_l)
      for (const long long pin : PINS) {
        const size_t m = log_c + log_l <= 6 ? 3 : 1;
        for (int pl = -1; pl <= log_l; ++pl) whole_call(log_c, log_l, m, pin, pl);
      }
  table_of_x();
  twist_and_rows();
  rules_and_saturation();
  layouts();
  if (fails) {
    printf("%d of %zu checks FAILED\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
