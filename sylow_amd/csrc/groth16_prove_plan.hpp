// groth16_prove_plan.hpp -- every size and route decision of the Groth16 prover (groth16_prove.hip): the lanes that share a row of the sparse
// product, its grid, the scratch of the three entry points with its offsets and the witnesses one chunk of a proving call holds.  Plain C++ over uint64_t,
// int32_t, int64_t, uint8_t and size_t only, so that tests/cpp/groth16_prove_plan_test.cpp can compile it with g++ on a box without a GPU.
// The launch code asks these functions and decides nothing itself.
#pragma once
#include "plan_base.hpp"

namespace g16_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::elems;
using plan_base::mul_sat;
using plan_base::words_of;
constexpr int32_t G16_BLOCK = 256;               // == BLOCK of common.hpp (groth16_prove.hip asserts it)
constexpr int32_t G16_LOG_N_MAX = 28;            // the domains of ntt_plan.hpp
constexpr size_t G16_GRID_CAP = (size_t)1 << 20; // blocks of one launch in x; more work than that is walked with a grid stride
constexpr size_t G16_GRID_Y_CAP = 65535;         // the batch index is the grid's y; more arrays than that are walked with a stride too
constexpr uint64_t G16_COSET_SHIFT = 5;          // g: the quotient is formed on g <w_n> (the generator arkworks and gnark shift by)

constexpr size_t ceil_div(size_t a, size_t b) { return a / b + (a % b ? 1 : 0); }
constexpr bool log_n_ok(int32_t log_n) { return log_n >= 0 && log_n <= G16_LOG_N_MAX; }

// ---- the sparse product out_j = M w_j: 2^k lanes share a row, k = 0 .. 6 ---------------------------------------------------------------
// A lane multiplies its entries into ONE unreduced 16-limb accumulator and reduces it (Barrett, about 2.4 products' worth of multiply-adds)
// once per SPMV_FLUSH entries and once at the end of the row; the lanes of a row then add their residues in k shuffle rounds.  A row shared
// by more lanes than it has work for pays a reduction per lane for nothing, so a lane is given at least SPMV_LANE_ENTRIES entries of an
// average row before the row is split further: k = floor(log2(density / SPMV_LANE_ENTRIES)), clamped to 0 .. SPMV_LANES_LOG_MAX.  Only
// nnz / rows is known on the host -- a skewed matrix gets the lanes of its average row.
constexpr int32_t SPMV_LANES_LOG_MAX = 6;        // one wavefront
constexpr int32_t SPMV_FLUSH = 16;               // products per reduction: 16 r^2 < 2^512 (the proof is at k_fr_spmv)
constexpr size_t SPMV_LANE_ENTRIES = 8;
constexpr bool spmv_lanes_log_ok(int32_t k) { return k < 0 || k <= SPMV_LANES_LOG_MAX; }
constexpr int32_t spmv_lanes_log(size_t rows, size_t nnz) {
  int32_t k = 0;
  if (rows)
    while (k < SPMV_LANES_LOG_MAX && (nnz / rows) >> (k + 1) >= SPMV_LANE_ENTRIES) ++k;
  return k;
}
constexpr int32_t spmv_lanes_log_or_default(int32_t k, size_t rows, size_t nnz) { return k < 0 ? spmv_lanes_log(rows, nnz) : k; }
constexpr size_t spmv_rows_per_block(int32_t k) { return (size_t)G16_BLOCK >> k; }
// blocks of rows that cover the n_out rows of one output array (the padding rows are written by the same kernel)
constexpr size_t spmv_row_blocks(size_t n_out, int32_t k) { return ceil_div(n_out, spmv_rows_per_block(k)); }
constexpr size_t grid_x(size_t items) { return items < G16_GRID_CAP ? (items ? items : 1) : G16_GRID_CAP; }
constexpr size_t grid_y(size_t m) { return m < G16_GRID_Y_CAP ? (m ? m : 1) : G16_GRID_Y_CAP; }
// u64 words of m arrays of n Fr elements, [m][4][n], saturated
constexpr size_t batch_words(size_t n, size_t m) { return mul_sat(mul_sat(4, n), m); }
// u64 words the sparse product leases: the m vectors in canonical form, SoA as they came
constexpr size_t spmv_scratch_words(size_t n_cols, size_t m) { return batch_words(n_cols, m); }
constexpr size_t spmv_scratch_bytes(size_t n_cols, size_t m) { return mul_sat(spmv_scratch_words(n_cols, m), 8); }
// element-wise kernels (canonical form, the slices, the quotient's product): one lane per element
constexpr size_t lane_blocks(size_t n) { return ceil_div(n, (size_t)G16_BLOCK); }

// ---- the quotient h = (a b - c) / (X^n - 1) on the coset g <w_n> --------------------------------------------------------------------------
// Two buffers of 3 m arrays ping-pong through the transforms (each sylow_hip_fr_ntt_batch call leases its own table and buffer on top), and
// 4 words hold g for them.
constexpr size_t QUOT_CONST_WORDS = 4;
constexpr size_t quot_buffer_words(int32_t log_n, size_t m) { return batch_words(elems(log_n), mul_sat(3, m)); }
struct QuotLayout { size_t g, x, y, bytes; };
constexpr QuotLayout quot_layout(int32_t log_n, size_t m, Carve c = {}) {      // c: the lease it is a part of (the proof's), or its own
  QuotLayout l{};
  l.g = c.words(QUOT_CONST_WORDS);
  l.x = c.words(quot_buffer_words(log_n, m));
  l.y = c.words(quot_buffer_words(log_n, m));
  l.bytes = c.at; return l;
}
constexpr size_t quot_scratch_words(int32_t log_n, size_t m) { return words_of(quot_layout(log_n, m).bytes); }

// ---- the proof: chunks of whole witnesses under the scratch budget -----------------------------------------------------------------------
// The closing sums hold, per witness: CLOSE_G1 G1 points and CLOSE_G2 G2 points as affine SoA words with a flag each, and CLOSE_FR scalars
// (groth16_prove.hip names them); the five multi-scalar multiplications leave 4 G1 points and 1 G2 point one after another before that.
constexpr size_t CLOSE_G1 = 17, CLOSE_G2 = 6, CLOSE_FR = 3, CLOSE_RAW_G1 = 4, CLOSE_RAW_G2 = 1;
// n_l = n_vars - n_inputs - 1 private variables (the caller checked n_inputs < n_vars)
constexpr size_t private_vars(size_t n_vars, size_t n_inputs) { return n_vars - n_inputs - 1; }
// the arrays a chunk of mc witnesses leases itself: the witnesses in canonical form [mc][4][n_vars], their private part [mc][4][n_l], the
// quotient's two buffers, the quotient cut to the n - 1 terms of h_query [mc][4][n - 1], the closing sums and, behind the words, their flags
// padded to a word
struct ProveLayout {
  size_t zc, zl;
  QuotLayout quot;      // offsets in this lease; quot.bytes is where it ends
  size_t hq, raw1, raw2, p, q, f, raw1_inf, raw2_inf, p_inf, q_inf, flags_end, bytes;      // flags_end: before the padding
};
constexpr ProveLayout prove_layout(int32_t log_n, size_t n_vars, size_t n_inputs, size_t mc) {
  Carve c; ProveLayout l{};
  l.zc = c.words(batch_words(n_vars, mc));
  l.zl = c.words(batch_words(private_vars(n_vars, n_inputs), mc));
  l.quot = quot_layout(log_n, mc, c);
  c.at = l.quot.bytes;
  l.hq = c.words(batch_words(elems(log_n) - 1, mc));
  l.raw1 = c.words(mul_sat(8 * CLOSE_RAW_G1, mc));
  l.raw2 = c.words(mul_sat(16 * CLOSE_RAW_G2, mc));
  l.p = c.words(mul_sat(8 * CLOSE_G1, mc));
  l.q = c.words(mul_sat(16 * CLOSE_G2, mc));
  l.f = c.words(mul_sat(4 * CLOSE_FR, mc));
  l.raw1_inf = c.bytes(mul_sat(CLOSE_RAW_G1, mc));
  l.raw2_inf = c.bytes(mul_sat(CLOSE_RAW_G2, mc));
  l.p_inf = c.bytes(mul_sat(CLOSE_G1, mc));
  l.q_inf = c.bytes(mul_sat(CLOSE_G2, mc));
  l.flags_end = c.at;
  c.round();
  l.bytes = c.at; return l;
}
constexpr size_t prove_chunk_bytes(int32_t log_n, size_t n_vars, size_t n_inputs, size_t mc) { return prove_layout(log_n, n_vars, n_inputs, mc).bytes; }
// its u64 words, before the flags
constexpr size_t prove_chunk_words(int32_t log_n, size_t n_vars, size_t n_inputs, size_t mc) { return words_of(prove_layout(log_n, n_vars, n_inputs, mc).raw1_inf); }
// the closing sums' share of it, words and flag bytes: the same under every circuit, read off the smallest one
constexpr size_t close_words(size_t mc) { return (prove_layout(0, 1, 0, mc).raw1_inf - prove_layout(0, 1, 0, mc).raw1) / 8; }
constexpr size_t close_flag_bytes(size_t mc) { return prove_layout(0, 1, 0, mc).flags_end - prove_layout(0, 1, 0, mc).raw1_inf; }
// bytes a chunk costs the budget: its own arrays and what the largest transform (3 mc arrays) leases meanwhile -- a table of n / 2 elements,
// 4 words and one more buffer.  The multi-scalar multiplications plan their own scratch under the same limit once the transforms are done.
constexpr size_t prove_budget_bytes(int32_t log_n, size_t n_vars, size_t n_inputs, size_t mc) {
  return add_sat(prove_chunk_bytes(log_n, n_vars, n_inputs, mc), mul_sat(8, add_sat(4 + 4 * (elems(log_n) / 2), quot_buffer_words(log_n, mc))));
}
// whole witnesses per chunk under `budget` bytes: 0 when not even one fits.  The cost is linear in mc but for the table, which is under 4 % of
// one witness's cost: the quotient of the budget by that cost is a lower bound, stepped up while one more witness still fits (a short walk)
constexpr size_t witnesses_per_chunk(int32_t log_n, size_t n_vars, size_t n_inputs, size_t m, size_t budget) {
  if (!m || prove_budget_bytes(log_n, n_vars, n_inputs, 1) > budget) return 0;
  size_t mc = budget / prove_budget_bytes(log_n, n_vars, n_inputs, 1);           // a lower bound: the table is counted once per witness here
  if (mc > m) mc = m;
  while (mc < m && prove_budget_bytes(log_n, n_vars, n_inputs, mc + 1) <= budget) ++mc;
  return mc;
}
}  // namespace g16_plan
