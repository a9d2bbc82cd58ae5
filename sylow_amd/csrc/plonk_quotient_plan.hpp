// plonk_quotient_plan.hpp -- the geometry of PLONK's quotient polynomial (plonk_quotient.hip): the rows of the per-circuit table, the items
// and tiles of the fused kernel, the degree bound and the tail the status reads, the chunks of whole instances under a scratch limit and
// every byte count and scratch offset, plain C++ so that tests/cpp/plonk_quotient_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch
// code asks these functions and decides nothing itself.
#pragma once
#include "fr_scan_plan.hpp"
#include "ntt_plan.hpp"
#include "plan_base.hpp"

namespace plonk_quotient_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::disjoint;
using plan_base::elems;
using plan_base::max_blocks_ok;
using plan_base::mul_sat;
using plan_base::words_of;
constexpr int PQ_BLOCK = 256;                    // == BLOCK of common.hpp (plonk_quotient.hip asserts it): a lane per point, a tile per block
constexpr int PQ_FLUSH = 16;                     // products the gate sum adds unreduced between two Barrett reductions (bn254_fr_acc.hpp)
constexpr uint64_t PQ_COSET_SHIFT = 5;           // K = 5 <w_N>: the shift of the Groth16 quotient; X^n - 1 never vanishes on K
constexpr int PQ_WIRES_MIN = 2;                  // the gate multiplies w_0 by w_1
constexpr int PQ_WIRES_MAX = fr_scan_plan::PLONK_WIRES_MAX;
constexpr int PQ_LOG_MAX = ntt_plan::NTT_LOG_N_MAX;                    // log_n + log_e: the domains of the transform
constexpr size_t PQ_GRID_CAP = (size_t)1 << 20;  // blocks of one launch; more work than that is walked with a grid stride
constexpr size_t FR_WORDS = 4;
constexpr int STATUS_NOT_DIVISIBLE = 1;          // bit 0: a coefficient of t past its degree bound is not 0

constexpr bool dims_ok(int log_n, int log_e, int wires) {
  return log_n >= 0 && log_e >= 0 && log_n <= PQ_LOG_MAX && log_e <= PQ_LOG_MAX && log_n + log_e <= PQ_LOG_MAX && wires >= PQ_WIRES_MIN && wires <= PQ_WIRES_MAX;
}
constexpr int log_big(int log_n, int log_e) { return log_n + log_e; }
constexpr size_t grid(size_t items, long long max_blocks) {
  const size_t cap = max_blocks > 0 && (unsigned long long)max_blocks < PQ_GRID_CAP ? (size_t)max_blocks : PQ_GRID_CAP;
  return items < cap ? (items ? items : 1) : cap;
}

// ---- the table of a circuit: 2 W + 3 rows of N points on K, [row][4][N], then zinv [4][E] ------------------------------------------------
constexpr size_t table_rows(int wires) { return 2 * (size_t)wires + 3; }
constexpr size_t row_selector(int j) { return (size_t)j; }                       // q_j, j < W
constexpr size_t row_qm(int wires) { return (size_t)wires; }
constexpr size_t row_qc(int wires) { return (size_t)wires + 1; }
constexpr size_t row_sigma(int wires, int j) { return (size_t)wires + 2 + (size_t)j; }
constexpr size_t row_l1(int wires) { return 2 * (size_t)wires + 2; }
constexpr size_t row_words(int log_n, int log_e) { return FR_WORDS * elems(log_big(log_n, log_e)); }
constexpr size_t zinv_offset_words(int log_n, int log_e, int wires) { return table_rows(wires) * row_words(log_n, log_e); }
constexpr size_t table_words(int log_n, int log_e, int wires) { return zinv_offset_words(log_n, log_e, wires) + FR_WORDS * elems(log_e); }
constexpr size_t table_bytes(int log_n, int log_e, int wires) { return table_words(log_n, log_e, wires) * sizeof(uint64_t); }
// the caller's selectors [W + 2][4][n] and sigma [W][4][n]
constexpr size_t selectors_bytes(int log_n, int wires) { return ((size_t)wires + 2) * FR_WORDS * elems(log_n) * sizeof(uint64_t); }
constexpr size_t sigma_bytes(int log_n, int wires) { return (size_t)wires * FR_WORDS * elems(log_n) * sizeof(uint64_t); }
// prepare leases: the coefficients of the 2 W + 3 rows [rows][4][n], the values of L_1 [4][n], the rows zero-padded [rows][4][N], the table
// of the N / 2 roots and the 4 words of the shift; the transforms lease their own on top
constexpr size_t PQ_SHIFT_WORDS = 4;
constexpr size_t prepare_coeff_words(int log_n, int wires) { return table_rows(wires) * FR_WORDS * elems(log_n); }
struct PrepareLayout { size_t g, roots, coeff, l1, padded, bytes; };
constexpr PrepareLayout prepare_layout(int log_n, int log_e, int wires) {
  Carve c; PrepareLayout l{};
  l.g = c.words(PQ_SHIFT_WORDS);
  l.roots = c.words(ntt_plan::root_words(log_big(log_n, log_e)));
  l.coeff = c.words(prepare_coeff_words(log_n, wires));
  l.l1 = c.words(FR_WORDS * elems(log_n));
  l.padded = c.words(zinv_offset_words(log_n, log_e, wires));
  l.bytes = c.at; return l;
}
constexpr size_t prepare_scratch_bytes(int log_n, int log_e, int wires) { return prepare_layout(log_n, log_e, wires).bytes; }
constexpr size_t prepare_scratch_words(int log_n, int log_e, int wires) { return words_of(prepare_scratch_bytes(log_n, log_e, wires)); }

// ---- the fused kernel: items are (instance, tile of PQ_BLOCK points), instance-major, a lane per point ----------------------------------
constexpr size_t tiles(int log_n, int log_e) { return elems(log_big(log_n, log_e)) / PQ_BLOCK + (elems(log_big(log_n, log_e)) % PQ_BLOCK ? 1 : 0); }
constexpr size_t items(int log_n, int log_e, size_t m) { return mul_sat(tiles(log_n, log_e), m); }
constexpr size_t item_instance(size_t item, size_t n_tiles) { return item / n_tiles; }
constexpr size_t item_tile(size_t item, size_t n_tiles) { return item % n_tiles; }
constexpr size_t point(size_t tile, int lane) { return tile * PQ_BLOCK + (size_t)lane; }
// the point whose z stands for z(w_n X) at point i: i + E, wrapped
constexpr size_t next_point(size_t i, int log_n, int log_e) { return (i + elems(log_e)) & (elems(log_big(log_n, log_e)) - 1); }
// the entry of zinv at point i
constexpr size_t zinv_slot(size_t i, int log_e) { return i & (elems(log_e) - 1); }
// the caller's arrays of the evaluation entry, bytes, saturated
constexpr size_t ext_bytes(int log_n, int log_e, size_t arrays) { return mul_sat(mul_sat(row_words(log_n, log_e), arrays), sizeof(uint64_t)); }
constexpr size_t scalars_bytes(size_t count) { return mul_sat(mul_sat(count, FR_WORDS), sizeof(uint64_t)); }
// the constants of an instance, formed once per call by a launch of their own: beta k_j 5 for j < W, then beta, gamma, alpha and alpha^2
constexpr size_t PQ_CHALLENGE_SLOTS = 4;
constexpr size_t const_slots(int wires) { return (size_t)wires + PQ_CHALLENGE_SLOTS; }
constexpr size_t consts_words(int wires, size_t m) { return mul_sat(mul_sat(const_slots(wires), FR_WORDS), m); }
// the evaluation entry leases the table of the N / 2 roots and the constants
struct EvalsLayout { size_t roots, consts, bytes; };
constexpr EvalsLayout evals_layout(int log_n, int log_e, int wires, size_t m) {
  Carve c; EvalsLayout l{};
  l.roots = c.words(ntt_plan::root_words(log_big(log_n, log_e)));
  l.consts = c.words(consts_words(wires, m));
  l.bytes = c.at; return l;
}
constexpr size_t evals_scratch_bytes(int log_n, int log_e, int wires, size_t m) { return evals_layout(log_n, log_e, wires, m).bytes; }
constexpr bool scratch_ok(size_t bytes) { return bytes <= SAT / 2; }

// ---- the degree bound of the numerator and the tail of t the status reads ----------------------------------------------------------------
constexpr bool lens_ok(int log_n, int log_e, size_t len_w, size_t len_z) {
  return len_w >= 1 && len_z >= 1 && len_w <= elems(log_big(log_n, log_e)) && len_z <= elems(log_big(log_n, log_e));
}
// D = max((len_z - 1) + W max(len_w - 1, 1), 2 (len_w - 1) + n - 1, n + len_z - 2) for lengths lens_ok accepts: below 2^34
constexpr size_t degree_bound(int log_n, int wires, size_t len_w, size_t len_z) {
  const size_t n = elems(log_n), perm = (len_z - 1) + (size_t)wires * (len_w > 2 ? len_w - 1 : 1), gate = 2 * (len_w - 1) + n - 1, bnd = n + len_z - 2;
  return perm > gate ? (perm > bnd ? perm : bnd) : (gate > bnd ? gate : bnd);
}
// the coefficients of t that must be 0: tail_first .. N - 1.  D >= n - 1, so D - n + 1 >= 0: at 0 the numerator has fewer than n coefficients
// and t must vanish
constexpr size_t tail_first(int log_n, int wires, size_t len_w, size_t len_z) { return degree_bound(log_n, wires, len_w, len_z) + 1 - elems(log_n); }
// t has N coefficients: its degree bound D - n must lie below N
constexpr bool degree_ok(int log_n, int log_e, int wires, size_t len_w, size_t len_z) {
  return tail_first(log_n, wires, len_w, len_z) <= elems(log_big(log_n, log_e));
}
constexpr size_t tail_len(int log_n, int log_e, int wires, size_t len_w, size_t len_z) { return elems(log_big(log_n, log_e)) - tail_first(log_n, wires, len_w, len_z); }
constexpr size_t tail_tiles(size_t len) { return len / PQ_BLOCK + (len % PQ_BLOCK ? 1 : 0); }
constexpr size_t tail_items(size_t len, size_t m) { return mul_sat(tail_tiles(len), m); }

// ---- the full route: W + 1 columns of an instance (the wires, then z), one more with public inputs; a chunk of mc whole instances is
// padded into one buffer [mc][cols][4][N], transformed into a second one, and t_ext [mc][4][N] takes the front of the first -------------
constexpr size_t columns(int wires, bool with_pi) { return (size_t)wires + 1 + (with_pi ? 1 : 0); }
constexpr size_t col_z(int wires) { return (size_t)wires; }
constexpr size_t col_pi(int wires) { return (size_t)wires + 1; }
constexpr size_t coeff_bytes(size_t len, size_t arrays) { return mul_sat(mul_sat(mul_sat(len, FR_WORDS), arrays), sizeof(uint64_t)); }
constexpr size_t pad_tiles(int log_n, int log_e, size_t cols, size_t mc) { return mul_sat(mul_sat(tiles(log_n, log_e), cols), mc); }
// u64 words of one of the two buffers
constexpr size_t chunk_buffer_words(int log_n, int log_e, size_t cols, size_t mc) { return mul_sat(mul_sat(row_words(log_n, log_e), cols), mc); }
// what the call leases for its chunks: the shift, the roots, the constants of the largest chunk (mc_lease instances, which fixes where the
// buffers start), the two buffers of this chunk's mc instances
struct ChunkLayout { size_t g, roots, consts, a, b, bytes; };
constexpr ChunkLayout chunk_layout(int log_n, int log_e, int wires, size_t cols, size_t mc_lease, size_t mc) {
  Carve c; ChunkLayout l{};
  l.g = c.words(PQ_SHIFT_WORDS);
  l.roots = c.words(ntt_plan::root_words(log_big(log_n, log_e)));
  l.consts = c.words(consts_words(wires, mc_lease));
  l.a = c.words(chunk_buffer_words(log_n, log_e, cols, mc));
  l.b = c.words(chunk_buffer_words(log_n, log_e, cols, mc));
  l.bytes = c.at; return l;
}
constexpr size_t chunk_bytes(int log_n, int log_e, int wires, size_t cols, size_t mc) { return chunk_layout(log_n, log_e, wires, cols, mc, mc).bytes; }
constexpr size_t chunk_words(int log_n, int log_e, int wires, size_t cols, size_t mc) { return words_of(chunk_bytes(log_n, log_e, wires, cols, mc)); }
// what a chunk holds at its peak: its own lease and the forward transform's on top (the larger of the two transforms)
constexpr size_t chunk_budget_bytes(int log_n, int log_e, int wires, size_t cols, size_t mc) {
  return mul_sat(add_sat(chunk_words(log_n, log_e, wires, cols, mc),
                         ntt_plan::scratch_words(log_big(log_n, log_e), mul_sat(cols, mc),
                                                 ntt_plan::steps(log_big(log_n, log_e), ntt_plan::NTT_STAGES_DEFAULT, false, true))),
                 sizeof(uint64_t));
}
// whole instances per chunk under `budget` bytes: 0 when not even one fits.  The cost is linear in mc but for the roots and the transform's
// table: the quotient of the budget by one instance's cost is a lower bound, stepped up while one more instance still fits (a short walk)
constexpr size_t instances_per_chunk(int log_n, int log_e, int wires, size_t cols, size_t m, size_t budget) {
  if (!m || chunk_budget_bytes(log_n, log_e, wires, cols, 1) > budget) return 0;
  size_t mc = budget / chunk_budget_bytes(log_n, log_e, wires, cols, 1);
  if (mc > m) mc = m;
  while (mc < m && chunk_budget_bytes(log_n, log_e, wires, cols, mc + 1) <= budget) ++mc;
  return mc;
}
constexpr size_t chunk_count(size_t m, size_t mc) { return mc ? m / mc + (m % mc ? 1 : 0) : 0; }
constexpr size_t chunk_size(size_t m, size_t mc, size_t first) { return m - first < mc ? m - first : mc; }
}  // namespace plonk_quotient_plan
