// kzg_cells_plan.hpp -- the geometry of the check of many cells of many KZG blobs as one boolean (kzg_cells.hip): rows of (cell index < c,
// commitment index < n_com, l values, weight), c = 2^log_c cells of l = 2^log_l points.  The route, the keys and their grouping, the keyed
// multiply-accumulate with its teams, staging and slices, the Horner fold with its chunks, the grids and the scratch with its offsets, plain C++ so that
// tests/cpp/kzg_cells_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch code asks these functions and decides
// nothing itself.
#pragma once
#include "ntt_plan.hpp"

namespace kzg_cells_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::disjoint_or_empty;      // an empty array of the caller overlaps nothing here
using plan_base::elems;
using plan_base::max_blocks_ok;
using plan_base::mul_sat;
using plan_base::words_of;
using ntt_plan::root_negated;
using ntt_plan::root_slot;
using ntt_plan::root_words;
constexpr int CELLS_BLOCK = 256;                      // == BLOCK of common.hpp (kzg_cells.hip asserts it)
constexpr int CELLS_BLOCK_LOG = 8;
constexpr int CELLS_WAVE = 64;
constexpr size_t FR_WORDS = 4, G1_WORDS = 8, G2_WORDS = 16;
constexpr int CELLS_LOG_N_MAX = 27;                   // the domains of sylow_hip_kzg_cosets.h
constexpr size_t CELLS_GRID_CAP = (size_t)1 << 16;    // blocks of one launch; more work than that is walked with a grid stride
// lanes the device keeps resident: 256 compute units x 4 SIMDs x 4 waves of 64.  Work below it is cut finer where the plan can.
constexpr size_t CELLS_RESIDENT_LANES = (size_t)256 * 4 * 4 * CELLS_WAVE;

constexpr int log_n(int log_c, int log_l) { return log_c + log_l; }
constexpr bool logs_ok(int log_c, int log_l) { return log_c >= 0 && log_l >= 0 && log_c <= CELLS_LOG_N_MAX && log_l <= CELLS_LOG_N_MAX && log_n(log_c, log_l) <= CELLS_LOG_N_MAX; }
constexpr size_t blocks_of(size_t lanes) { return lanes / CELLS_BLOCK + (lanes % CELLS_BLOCK ? 1 : 0); }          // no sum that could wrap
constexpr size_t grid(size_t blocks, long long max_blocks) {
  const size_t cap = max_blocks > 0 && (unsigned long long)max_blocks < CELLS_GRID_CAP ? (size_t)max_blocks : CELLS_GRID_CAP;
  return blocks < cap ? (blocks ? blocks : 1) : cap;
}

// ---- the route: A = sum_k r_k R_k by columns (the keyed sums S_i, one transform of c arrays, the Horner fold: N l multiply-adds, c
// transforms, c l products) or by rows (the interpolant of every row, then one linear combination: `rows` transforms and twists).  The
// column route pays for c arrays whatever `rows` is, so it is taken from rows = c on.
constexpr int ROUTE_ROWS = 0, ROUTE_COLUMNS = 1;
constexpr bool route_ok(int route) { return route <= ROUTE_COLUMNS; }
constexpr int route_of(int route, int log_c, size_t rows) { return route < 0 ? (rows >= elems(log_c) ? ROUTE_COLUMNS : ROUTE_ROWS) : route; }

// ---- the caller's arrays, bytes, saturated
constexpr size_t index_bytes(size_t rows) { return mul_sat(rows, sizeof(uint64_t)); }
constexpr size_t scalar_bytes(size_t count) { return mul_sat(count, FR_WORDS * sizeof(uint64_t)); }
constexpr size_t vals_bytes(int log_l, size_t rows) { return mul_sat(mul_sat(elems(log_l), rows), FR_WORDS * sizeof(uint64_t)); }
constexpr size_t point_bytes(size_t count) { return mul_sat(count, G1_WORDS * sizeof(uint64_t)); }

// ---- the keys.  A row that takes part (in range, weight not 0 mod r) has a commitment key and, on the column route, a cell key; the cell
// keys come first.  An entry is (row, kind): the cell entries first.  A row that takes no part carries the key n_keys, which no group has.
// The rows are grouped by key on the device: counts (atomic adds), starts (one block scans the counts in rounds of CELLS_BLOCK), and a
// permutation (an atomic cursor per key).  THE ORDER INSIDE A GROUP IS WHATEVER THE ATOMICS GIVE: the sums are exact in Fr, so the words
// do not depend on it.
constexpr size_t cell_keys(int route, int log_c) { return route == ROUTE_COLUMNS ? elems(log_c) : 0; }
constexpr size_t n_keys(int route, int log_c, size_t n_com) { return add_sat(cell_keys(route, log_c), n_com); }
constexpr size_t cell_entries(int route, size_t rows) { return route == ROUTE_COLUMNS ? rows : 0; }
constexpr size_t entries(int route, size_t rows) { return add_sat(cell_entries(route, rows), rows); }
constexpr size_t entry_row(size_t e, int route, size_t rows) { return e - (e >= cell_entries(route, rows) ? cell_entries(route, rows) : 0); }
constexpr bool in_range(uint64_t idx, int log_c) { return idx < ((uint64_t)1 << log_c); }
constexpr size_t rows_grid(size_t rows, long long max_blocks) { return grid(blocks_of(rows), max_blocks); }
constexpr size_t scatter_grid(int route, size_t rows, long long max_blocks) { return grid(blocks_of(entries(route, rows)), max_blocks); }
constexpr size_t scan_rounds(size_t keys) { return blocks_of(keys); }
// v^i, i < c, from the table of the transform of c points: root_words, root_slot and root_negated of ntt_plan.hpp

// ---- the keyed multiply-accumulate: out[key][col] = sum over the rows of the key's group of r_row val_row[col], col < 2^log_cols.  The
// work items are (key, column) FLATTENED, key-major, so that rows of 1 .. 8 columns still fill wavefronts; a block takes a tile of
// CELLS_BLOCK of them.  The lanes that share a key are a TEAM (2^mac_team_log adjacent lanes; a key of 256 columns or more spans whole
// blocks).  A group goes by in rounds of 2^mac_stage_log rows: the first lanes of a team bring the round's row numbers and weights into the
// team's LDS slots, then every lane of the team adds its products UNREDUCED; an accumulator is folded before it could hold more than
// MAC_FLUSH products (bn254_fr_acc.hpp: 16).  The LDS of a block is CELLS_BLOCK slots whatever the shape.
// Where the tiles do not fill the device and the groups are long, a group is cut into `slices` parts (item = (slice, tile)); each slice
// writes its own partial array and one more launch adds them.
constexpr int MAC_FLUSH = 16, MAC_STAGE_LOG = 4, MAC_SLICES_MAX = 64;
static_assert((1 << MAC_STAGE_LOG) <= MAC_FLUSH, "a round fits one fold");
constexpr int mac_team_log(int log_cols) { return log_cols < CELLS_BLOCK_LOG ? log_cols : CELLS_BLOCK_LOG; }
constexpr int mac_stage_log(int log_cols) { return log_cols < MAC_STAGE_LOG ? log_cols : MAC_STAGE_LOG; }
constexpr int mac_team(int lane, int log_cols) { return lane >> mac_team_log(log_cols); }
constexpr int mac_team_lane(int lane, int log_cols) { return lane & ((1 << mac_team_log(log_cols)) - 1); }
constexpr int mac_slot(int lane, int log_cols) { return mac_team(lane, log_cols) << mac_stage_log(log_cols); }        // the team's first LDS slot
constexpr int mac_slots(int log_cols) { return (CELLS_BLOCK >> mac_team_log(log_cols)) << mac_stage_log(log_cols); }   // <= CELLS_BLOCK
constexpr bool mac_folds(int pending, int log_cols) { return pending + (1 << mac_stage_log(log_cols)) > MAC_FLUSH; }  // before the next round
constexpr size_t mac_flat(size_t keys, int log_cols) { return mul_sat(keys, elems(log_cols)); }
constexpr size_t mac_tiles(size_t keys, int log_cols) { return blocks_of(mac_flat(keys, log_cols)); }
constexpr size_t mac_items(size_t keys, int log_cols, size_t slices) { return mul_sat(mac_tiles(keys, log_cols), slices); }
constexpr size_t mac_slice(size_t item, size_t tiles) { return item / tiles; }
constexpr size_t mac_tile(size_t item, size_t tiles) { return item % tiles; }
constexpr size_t mac_key(size_t flat, int log_cols) { return flat >> log_cols; }
constexpr size_t mac_col(size_t flat, int log_cols) { return flat & (elems(log_cols) - 1); }
constexpr size_t mac_grid(size_t keys, int log_cols, size_t slices, long long max_blocks) { return grid(mac_items(keys, log_cols, slices), max_blocks); }
constexpr size_t mac_lds_bytes() { return (size_t)CELLS_BLOCK * (8 * sizeof(uint32_t) + sizeof(uint64_t)) + sizeof(uint64_t); }
// slice s of a group of `len` rows: [slice_begin(len, s, slices), slice_begin(len, s + 1, slices)), the first len % slices one longer
constexpr size_t slice_begin(size_t len, size_t s, size_t slices) { return s * (len / slices) + (s < len % slices ? s : len % slices); }
// the smallest power of two that brings the items up to the resident lanes, while a slice of the AVERAGE group keeps MAC_FLUSH rows
constexpr size_t mac_slices(size_t keys, int log_cols, size_t rows) {
  if (!keys) return 1;
  const size_t lanes = mul_sat(mac_tiles(keys, log_cols), CELLS_BLOCK), avg = rows / keys;
  size_t s = 1;
  while (s < (size_t)MAC_SLICES_MAX && mul_sat(lanes, s) < CELLS_RESIDENT_LANES && avg / (2 * s) >= (size_t)MAC_FLUSH) s *= 2;
  return s;
}
constexpr bool joins(size_t slices) { return slices > 1; }
constexpr size_t join_grid(size_t keys, int log_cols, long long max_blocks) { return grid(mac_tiles(keys, log_cols), max_blocks); }
constexpr size_t slice_words(size_t keys, int log_cols) { return mul_sat(mac_flat(keys, log_cols), FR_WORDS); }       // one partial array
constexpr size_t partial_words(size_t keys, int log_cols, size_t slices) { return joins(slices) ? mul_sat(slice_words(keys, log_cols), slices) : 0; }
// where element (key, col) lies: S is [c][4][l], the layout the transform takes; W is [4][n_com], one column
constexpr size_t s_key_stride(int log_l) { return FR_WORDS << log_l; }
constexpr size_t s_word_stride(int log_l) { return elems(log_l); }
constexpr size_t w_key_stride() { return 1; }
constexpr size_t w_word_stride(size_t n_com) { return n_com; }

// ---- the Horner fold A[t] = sum_(i<c) a_i[t] g_t^i, g_t = w^(-t) = w^((n - t) mod n): l lanes alone are too few, so i is cut into
// 2^horner_lanes_log chunks over ADJACENT lanes of a wave: lane q runs Horner over the chunk's a_i from the top, multiplies by
// g_t^(chunk q), and the lanes of a t meet through shuffles.  Exponents are taken mod n and stay below 2^27.
constexpr int HORNER_LANES_LOG = 4;
constexpr int horner_lanes_log(int log_c) { return log_c < HORNER_LANES_LOG ? log_c : HORNER_LANES_LOG; }
constexpr size_t horner_chunk(int log_c) { return elems(log_c) >> horner_lanes_log(log_c); }
constexpr size_t horner_items(int log_c, int log_l) { return elems(log_l) << horner_lanes_log(log_c); }
constexpr size_t horner_t(size_t item, int log_c) { return item >> horner_lanes_log(log_c); }
constexpr size_t horner_q(size_t item, int log_c) { return item & (elems(horner_lanes_log(log_c)) - 1); }
constexpr size_t horner_first(size_t q, int log_c) { return q * horner_chunk(log_c); }                                // the chunk's lowest i
constexpr uint64_t horner_g_exp(size_t t, int log_c, int log_l) { return (elems(log_n(log_c, log_l)) - t) & (elems(log_n(log_c, log_l)) - 1); }
constexpr uint64_t horner_join_exp(size_t t, size_t q, int log_c, int log_l) {
  return (horner_g_exp(t, log_c, log_l) * (uint64_t)horner_first(q, log_c)) & (elems(log_n(log_c, log_l)) - 1);
}
constexpr size_t horner_grid(int log_c, int log_l, long long max_blocks) { return grid(blocks_of(horner_items(log_c, log_l)), max_blocks); }
static_assert((1 << HORNER_LANES_LOG) <= CELLS_WAVE, "the lanes of a t share a wave");

// ---- the scratch of the fold, saturated: the roots; the keys of the entries; counts, starts (one more) and cursors of the
// keys; the permutation; the partial sums of W; then by columns S and its transform [c][4][l] with the partials of S, by rows the
// interpolants [rows][4][l].  The calls of the library the fold makes lease their own on top.
constexpr size_t array_words(int log_c, int log_l) { return FR_WORDS << log_n(log_c, log_l); }
struct FoldLayout { size_t roots, keys, perm, cnt, start, next, wpart, body, a, spart, bytes; };      // body: S by columns, the interpolants by rows
constexpr FoldLayout fold_layout(int route, int log_c, int log_l, size_t rows, size_t n_com) {
  const bool cols = route == ROUTE_COLUMNS;
  Carve c; FoldLayout l{};
  l.roots = c.words(root_words(log_c));
  l.keys = c.words(entries(route, rows));
  l.perm = c.words(entries(route, rows));
  l.cnt = c.words(n_keys(route, log_c, n_com));
  l.start = c.words(add_sat(n_keys(route, log_c, n_com), 1));
  l.next = c.words(n_keys(route, log_c, n_com));
  l.wpart = c.words(partial_words(n_com, 0, mac_slices(n_com, 0, rows)));
  l.body = c.words(cols ? array_words(log_c, log_l) : mul_sat(mul_sat(elems(log_l), rows), FR_WORDS));
  l.a = c.words(cols ? array_words(log_c, log_l) : 0);
  l.spart = c.words(cols ? partial_words(elems(log_c), log_l, mac_slices(elems(log_c), log_l, rows)) : 0);
  l.bytes = c.at; return l;
}
constexpr size_t fold_scratch_bytes(int route, int log_c, int log_l, size_t rows, size_t n_com) { return fold_layout(route, log_c, log_l, rows, n_com).bytes; }
constexpr size_t fold_scratch_words(int route, int log_c, int log_l, size_t rows, size_t n_com) { return words_of(fold_scratch_bytes(route, log_c, log_l, rows, n_com)); }
// of the reduction: W, A, r, r z; the n_com + rows scalars and bases of the first multi-scalar multiplication; its sum and A(tau) G1gen;
// then the flags of the bases and of the two points, the latter in 8 bytes of which 2 are used.  Of the weighted check: F and P, the two
// pairs, and eight flag bytes in one word.
constexpr size_t terms(size_t rows, size_t n_com) { return add_sat(rows, n_com); }
struct ReduceLayout { size_t w, a, r, rz, sc, bases, m1, at, binf, m1inf, atinf, bytes; };
constexpr ReduceLayout reduce_layout(int log_l, size_t rows, size_t n_com) {
  Carve c; ReduceLayout l{};
  l.w = c.words(mul_sat(FR_WORDS, n_com));
  l.a = c.words(mul_sat(FR_WORDS, elems(log_l)));
  l.r = c.words(mul_sat(FR_WORDS, rows));
  l.rz = c.words(mul_sat(FR_WORDS, rows));
  l.sc = c.words(mul_sat(FR_WORDS, terms(rows, n_com)));
  l.bases = c.words(mul_sat(G1_WORDS, terms(rows, n_com)));
  l.m1 = c.words(G1_WORDS);
  l.at = c.words(G1_WORDS);
  l.binf = c.bytes(terms(rows, n_com));
  l.m1inf = c.bytes(1);
  l.atinf = c.bytes(1);
  c.bytes(6);
  l.bytes = c.at; return l;
}
constexpr size_t reduce_scratch_bytes(int log_l, size_t rows, size_t n_com) { return reduce_layout(log_l, rows, n_com).bytes; }
constexpr size_t reduce_scratch_words(int log_l, size_t rows, size_t n_com) { return words_of(reduce_layout(log_l, rows, n_com).binf); }      // before the flags
struct VerifyLayout { size_t f, p, pxy, qxy, finf, pinf_one, pinf, qinf, flag, one, bytes; };
constexpr VerifyLayout verify_layout() {
  Carve c; VerifyLayout l{};
  l.f = c.words(G1_WORDS);
  l.p = c.words(G1_WORDS);
  l.pxy = c.words(2 * G1_WORDS);
  l.qxy = c.words(2 * G2_WORDS);
  l.finf = c.bytes(1);
  l.pinf_one = c.bytes(1);
  l.pinf = c.bytes(2);
  l.qinf = c.bytes(2);
  l.flag = c.bytes(1);
  l.one = c.bytes(1);
  l.bytes = c.at; return l;
}
constexpr size_t verify_scratch_bytes() { return verify_layout().bytes; }
constexpr bool scratch_ok(size_t bytes) { return bytes <= SAT / 2; }
}  // namespace kzg_cells_plan
