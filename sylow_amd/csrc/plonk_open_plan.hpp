// plonk_open_plan.hpp -- the geometry of PLONK's closing rounds (plonk_open.hip): the rows of the per-circuit coefficient table, the slots of
// an instance's evaluations and of its weight vector, the items, chunks and tiles of the three kernels, the lengths of r and F, the chunks of
// whole instances under a scratch limit and every byte count and scratch offset, plain C++ so that tests/cpp/plonk_open_plan_test.cpp can compile it with g++ on a
// box without a GPU.  The launch code asks these functions and decides nothing itself.
#pragma once
#include "fr_scan_plan.hpp"
#include "kzg_prove_plan.hpp"
#include "ntt_plan.hpp"
#include "plan_base.hpp"

namespace plonk_open_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::disjoint;
using plan_base::elems;
using plan_base::max_blocks_ok;
using plan_base::mul_sat;
using plan_base::words_of;
constexpr int PO_BLOCK = 256;                    // == BLOCK of common.hpp (plonk_open.hip asserts it): a lane per column, a tile per block
constexpr int PO_FLUSH = 16;                     // products an accumulator adds unreduced between two Barrett reductions (bn254_fr_acc.hpp)
constexpr int PO_WEIGHT_ROUND = 16;              // weights of an instance a block stages in LDS at a time
constexpr int PO_WIRES_MIN = 2;                  // the gate multiplies w_0 by w_1
constexpr int PO_WIRES_MAX = fr_scan_plan::PLONK_WIRES_MAX;
constexpr int PO_LOG_MAX = ntt_plan::NTT_LOG_N_MAX;                    // log_n + log_e: the domains of the transform
constexpr size_t PO_GRID_CAP = (size_t)1 << 20;  // blocks of one launch; more work than that is walked with a grid stride
constexpr size_t PO_EVAL_CHUNK = kzg_plan::KZG_POLY_CHUNK;             // coefficients a block evaluates: a lane runs Horner over 8, the block folds 256 lanes
constexpr size_t FR_WORDS = 4;
constexpr int STATUS_R_NOT_ZERO = 1;             // bit 0: r(zeta) != 0
constexpr int STATUS_ZETA_IN_DOMAIN = 2;         // bit 1: zeta^n = 1

constexpr bool dims_ok(int log_n, int log_e, int wires) {
  return log_n >= 0 && log_e >= 0 && log_n <= PO_LOG_MAX && log_e <= PO_LOG_MAX && log_n + log_e <= PO_LOG_MAX && wires >= PO_WIRES_MIN && wires <= PO_WIRES_MAX;
}
constexpr int log_big(int log_n, int log_e) { return log_n + log_e; }
constexpr bool lens_ok(int log_big_n, size_t len_w, size_t len_z) { return len_w >= 1 && len_z >= 1 && len_w <= elems(log_big_n) && len_z <= elems(log_big_n); }
constexpr size_t grid(size_t items, long long max_blocks) {
  const size_t cap = max_blocks > 0 && (unsigned long long)max_blocks < PO_GRID_CAP ? (size_t)max_blocks : PO_GRID_CAP;
  return items < cap ? (items ? items : 1) : cap;
}
constexpr size_t ceil_div(size_t a, size_t b) { return a / b + (a % b ? 1 : 0); }
constexpr size_t max2(size_t a, size_t b) { return a > b ? a : b; }
constexpr size_t lane_tiles(size_t lanes) { return ceil_div(lanes, PO_BLOCK); }       // blocks of a launch that keeps a lane per element
constexpr size_t scalars_bytes(size_t count) { return mul_sat(mul_sat(count, FR_WORDS), sizeof(uint64_t)); }
constexpr size_t coeff_bytes(size_t len, size_t arrays) { return mul_sat(mul_sat(mul_sat(len, FR_WORDS), arrays), sizeof(uint64_t)); }

// ---- the coefficient table of a circuit: 2 W + 2 rows of n coefficients, [row][4][n]: q_0 .. q_(W-1), q_M, q_C, sigma_0 .. sigma_(W-1) ---------
constexpr size_t ctable_rows(int wires) { return 2 * (size_t)wires + 2; }
constexpr size_t row_selector(int j) { return (size_t)j; }
constexpr size_t row_qm(int wires) { return (size_t)wires; }
constexpr size_t row_qc(int wires) { return (size_t)wires + 1; }
constexpr size_t row_sigma(int wires, int j) { return (size_t)wires + 2 + (size_t)j; }
constexpr size_t ctable_words(int log_n, int wires) { return ctable_rows(wires) * FR_WORDS * elems(log_n); }
constexpr size_t ctable_bytes(int log_n, int wires) { return ctable_words(log_n, wires) * sizeof(uint64_t); }
constexpr size_t selectors_bytes(int log_n, int wires) { return ((size_t)wires + 2) * FR_WORDS * elems(log_n) * sizeof(uint64_t); }
constexpr size_t sigma_bytes(int log_n, int wires) { return (size_t)wires * FR_WORDS * elems(log_n) * sizeof(uint64_t); }

// ---- the evaluations of an instance: 2 W + 1 slots, instance-major in evals [4][(2 W + 1) m] ---------------------------------------------------
constexpr size_t eval_slots(int wires) { return 2 * (size_t)wires + 1; }
constexpr size_t slot_wire(int j) { return (size_t)j; }                                   // a_j = w_j(zeta), j < W
constexpr size_t slot_sigma(int wires, int j) { return (size_t)wires + (size_t)j; }        // s_j = sigma_j(zeta), j < W - 1
constexpr size_t slot_zw(int wires) { return 2 * (size_t)wires - 1; }                      // z(zeta w_n)
constexpr size_t slot_pi(int wires) { return 2 * (size_t)wires; }                          // PI(zeta), 0 without public inputs
constexpr size_t evals_count(int wires, size_t m) { return mul_sat(eval_slots(wires), m); }
constexpr size_t evals_bytes(int wires, size_t m) { return scalars_bytes(evals_count(wires, m)); }

// ---- k_po_eval: items are (instance, row, chunk of PO_EVAL_CHUNK coefficients); every row of a launch is given the chunks of the longest,
// and an item past the end of its own row stores the partial 0.  The partials [4][items], then a block per (instance, row) folds them --------
constexpr size_t eval_chunks(size_t longest) { return longest ? ceil_div(longest, PO_EVAL_CHUNK) : 1; }
constexpr size_t eval_items(size_t rows, size_t longest, size_t m) { return mul_sat(mul_sat(rows, eval_chunks(longest)), m); }
constexpr size_t eval_item_instance(size_t item, size_t rows, size_t chunks) { return item / (rows * chunks); }
constexpr size_t eval_item_row(size_t item, size_t rows, size_t chunks) { return item % (rows * chunks) / chunks; }
constexpr size_t eval_item_chunk(size_t item, size_t chunks) { return item % chunks; }
constexpr bool eval_chunk_live(size_t len, size_t chunk) { return chunk * PO_EVAL_CHUNK < len; }      // the row owns a coefficient of this chunk
// the second launch, a block per (instance, row): a lane folds `segment` consecutive chunks, the block the lanes that own one
constexpr size_t eval_fold_segment(size_t chunks) { return chunks ? ceil_div(chunks, PO_BLOCK) : 1; }
constexpr size_t eval_fold_lanes(size_t chunks) { return ceil_div(chunks, eval_fold_segment(chunks)); }
constexpr size_t eval_partial_words(size_t rows, size_t longest, size_t m) { return mul_sat(eval_items(rows, longest, m), FR_WORDS); }
// the two points of an instance, [2][4][m]: zeta and zeta w_n, canonical
constexpr size_t point_words(size_t m) { return mul_sat(2 * FR_WORDS, m); }
constexpr size_t longest_row(int log_n, size_t len_w, size_t len_z) { return max2(max2(elems(log_n), len_w), len_z); }
// the evaluate entry leases the points and the partials; c: the lease they are a part of (the full route's), or their own
struct EvaluateLayout { size_t pts, partials, bytes; };
constexpr EvaluateLayout evaluate_layout(int log_n, int wires, size_t len_w, size_t len_z, size_t m, Carve c = {}) {
  EvaluateLayout l{};
  l.pts = c.words(point_words(m));
  l.partials = c.words(eval_partial_words(eval_slots(wires), longest_row(log_n, len_w, len_z), m));
  l.bytes = c.at; return l;
}
constexpr size_t evaluate_scratch_words(int log_n, int wires, size_t len_w, size_t len_z, size_t m) {
  return words_of(evaluate_layout(log_n, wires, len_w, len_z, m).bytes);
}
constexpr bool scratch_ok(size_t words) { return words <= SAT / 2 / sizeof(uint64_t); }

// ---- the weight vector of an instance (k_po_consts), [slots][4]: the rows of the fold in the order the kernel walks them, then two scalars ---
constexpr size_t fold_rows(int log_e, int wires) { return 3 * (size_t)wires + 3 + elems(log_e); }
constexpr size_t wrow_shared(size_t row) { return row; }                                  // the 2 W + 2 rows of the table
constexpr size_t wrow_z(int wires) { return 2 * (size_t)wires + 2; }
constexpr size_t wrow_wire(int wires, int j) { return 2 * (size_t)wires + 3 + (size_t)j; }
constexpr size_t wrow_chunk(int wires, size_t e) { return 3 * (size_t)wires + 3 + e; }       // t_e, weight -ZH zeta^(e n)
constexpr size_t wslot_const(int log_e, int wires) { return fold_rows(log_e, wires); }       // the constant term of r
constexpr size_t wslot_zh(int log_e, int wires) { return fold_rows(log_e, wires) + 1; }      // ZH = zeta^n - 1, for the status
constexpr size_t weight_slots(int log_e, int wires) { return fold_rows(log_e, wires) + 2; }
constexpr size_t weight_words(int log_e, int wires, size_t m) { return mul_sat(mul_sat(weight_slots(log_e, wires), FR_WORDS), m); }
// a row that only F takes: sigma_j for j < W - 1 and the wires.  Every other row belongs to r
constexpr bool row_is_extra(int wires, size_t row) {
  return (row >= row_sigma(wires, 0) && row + 1 < row_sigma(wires, wires)) || (row >= wrow_wire(wires, 0) && row < wrow_chunk(wires, 0));
}
// products a column adds: those of r, and those of r and F together
constexpr size_t products_r(int log_e, int wires) { return (size_t)wires + 4 + elems(log_e); }
constexpr size_t products_f(int log_e, int wires) { return products_r(log_e, wires) + 2 * (size_t)wires - 1; }

// ---- k_po_fold: items are (instance, tile of PO_BLOCK coefficient columns), instance-major, a lane per column ----------------------------------
constexpr size_t len_r(int log_n, size_t len_z) { return max2(elems(log_n), len_z); }
constexpr size_t len_f(int log_n, size_t len_w, size_t len_z) { return max2(len_r(log_n, len_z), len_w); }
constexpr bool len_out_ok(int log_n, size_t len_w, size_t len_z, size_t len_out, bool with_f) {
  return len_out >= (with_f ? len_f(log_n, len_w, len_z) : len_r(log_n, len_z));
}
constexpr size_t tiles(size_t len) { return ceil_div(len, PO_BLOCK); }
constexpr size_t items(size_t len, size_t m) { return mul_sat(tiles(len), m); }
constexpr size_t item_instance(size_t item, size_t n_tiles) { return item / n_tiles; }
constexpr size_t column(size_t item, size_t n_tiles, int lane) { return item % n_tiles * PO_BLOCK + (size_t)lane; }
// the linearise entry leases: the points, the weights, r(zeta) [4][m], the partials of r's evaluation and r itself when the caller takes only F
struct LineariseLayout { size_t pts, weights, rz, partials, r_buf, bytes; };
constexpr LineariseLayout linearise_layout(int log_n, int log_e, int wires, size_t len_z, size_t len_out, size_t m, bool own_r) {
  const size_t r_row = own_r ? len_r(log_n, len_z) : len_out;
  Carve c; LineariseLayout l{};
  l.pts = c.words(point_words(m));
  l.weights = c.words(weight_words(log_e, wires, m));
  l.rz = c.words(mul_sat(FR_WORDS, m));
  l.partials = c.words(eval_partial_words(1, r_row, m));
  l.r_buf = c.words(own_r ? mul_sat(mul_sat(r_row, FR_WORDS), m) : 0);
  l.bytes = c.at; return l;
}
constexpr size_t linearise_scratch_words(int log_n, int log_e, int wires, size_t len_z, size_t len_out, size_t m, bool own_r) {
  return words_of(linearise_layout(log_n, log_e, wires, len_z, len_out, m, own_r).bytes);
}

// ---- the full route: a chunk of mc whole instances leases the points, the partials, the weights, F and the padded z [mc][4][len_srs] each,
// F(zeta) and z(zeta w_n) [4][mc] each, the two proofs [8][mc] each and their flags; sylow_hip_kzg_open_batch leases a quotient buffer
// [mc][4][len_srs] on top, which the budget counts (the commitment under it plans its own chunks against the same limit) -------------------
struct OpenLayout {
  EvaluateLayout ev;      // offsets in this lease; ev.bytes is where it ends
  size_t weights, F, Z, yf, yz, p1, p2, f1, f2, bytes;
};
constexpr OpenLayout open_layout(int log_n, int log_e, int wires, size_t len_w, size_t len_z, size_t len_srs, size_t mc) {
  Carve c; OpenLayout l{};
  l.ev = evaluate_layout(log_n, wires, len_w, len_z, mc, c);
  c.at = l.ev.bytes;
  l.weights = c.words(weight_words(log_e, wires, mc));
  l.F = c.words(mul_sat(mul_sat(FR_WORDS, len_srs), mc));
  l.Z = c.words(mul_sat(mul_sat(FR_WORDS, len_srs), mc));
  l.yf = c.words(mul_sat(FR_WORDS, mc));
  l.yz = c.words(mul_sat(FR_WORDS, mc));
  l.p1 = c.words(mul_sat(8, mc));
  l.p2 = c.words(mul_sat(8, mc));
  l.f1 = c.bytes(mc);
  l.f2 = c.bytes(mc);
  c.round();
  l.bytes = c.at; return l;
}
constexpr size_t open_chunk_bytes(int log_n, int log_e, int wires, size_t len_w, size_t len_z, size_t len_srs, size_t mc) {
  return open_layout(log_n, log_e, wires, len_w, len_z, len_srs, mc).bytes;
}
// the u64 words its two flags an instance take: the same at every shape, read off the smallest one
constexpr size_t flag_words(size_t mc) { return words_of(open_layout(0, 0, PO_WIRES_MIN, 1, 1, 1, mc).bytes - open_layout(0, 0, PO_WIRES_MIN, 1, 1, 1, mc).f1); }
constexpr size_t open_chunk_words(int log_n, int log_e, int wires, size_t len_w, size_t len_z, size_t len_srs, size_t mc) {
  return words_of(open_chunk_bytes(log_n, log_e, wires, len_w, len_z, len_srs, mc));
}
constexpr size_t open_budget_bytes(int log_n, int log_e, int wires, size_t len_w, size_t len_z, size_t len_srs, size_t mc) {
  return mul_sat(add_sat(open_chunk_words(log_n, log_e, wires, len_w, len_z, len_srs, mc), mul_sat(mul_sat(FR_WORDS, len_srs), mc)), sizeof(uint64_t));
}
// whole instances per chunk under `budget` bytes: 0 when not even one fits.  The cost grows with mc: the quotient of the budget by one
// instance's cost is a lower bound but for the rounding of the flags, stepped down while it does not fit and up while one more still does
constexpr size_t instances_per_chunk(int log_n, int log_e, int wires, size_t len_w, size_t len_z, size_t len_srs, size_t m, size_t budget) {
  if (!m || open_budget_bytes(log_n, log_e, wires, len_w, len_z, len_srs, 1) > budget) return 0;
  size_t mc = budget / open_budget_bytes(log_n, log_e, wires, len_w, len_z, len_srs, 1);
  if (mc > m) mc = m;
  while (mc > 1 && open_budget_bytes(log_n, log_e, wires, len_w, len_z, len_srs, mc) > budget) --mc;
  while (mc < m && open_budget_bytes(log_n, log_e, wires, len_w, len_z, len_srs, mc + 1) <= budget) ++mc;
  return mc;
}
constexpr size_t chunk_count(size_t m, size_t mc) { return mc ? m / mc + (m % mc ? 1 : 0) : 0; }
constexpr size_t chunk_size(size_t m, size_t mc, size_t first) { return m - first < mc ? m - first : mc; }
}  // namespace plonk_open_plan
