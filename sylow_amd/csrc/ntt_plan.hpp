// ntt_plan.hpp -- the geometry of the batched radix-2 transform over Fr (ntt.hip): passes, stages per pass, tiles, grids, the twiddle table,
// the ping-pong and the scratch with its offsets, plain C++ so that tests/cpp/ntt_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch
// code asks these functions and decides nothing itself.
#pragma once
#include "plan_base.hpp"

namespace ntt_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::elems;
using plan_base::mul_sat;
using plan_base::words_of;
// r - 1 = 2^28 * odd: radix-2 domains up to 2^28
constexpr int NTT_LOG_N_MAX = 28;
constexpr int NTT_BLOCK = 256;                   // == BLOCK of common.hpp (ntt.hip asserts it)
// A block takes a tile of 2^NTT_TILE_LOG elements through the stages of one pass in LDS (rows of 8 dwords: 32 KB), a lane two butterflies per
// stage.  A pass of s stages is a radix-2^s step; a tile holds 2^(NTT_TILE_LOG - s) such groups side by side (fewer when the array has fewer).
constexpr int NTT_TILE_LOG = 10;
constexpr int NTT_STAGES_MAX = NTT_TILE_LOG;     // stages of one pass: 1 .. NTT_STAGES_MAX
// 5: four passes of 5 stages (32 groups side by side: 256 consecutive bytes per word plane read, and stored from the second pass on) beat two of 10 (one group per tile:
// every access 2^(log_n - 10) elements apart) at (1, 2^20) and (64, 2^14), outside the spread of the run (profiles/ntt/bench_ntt.json)
constexpr int NTT_STAGES_DEFAULT = 5;
static_assert(NTT_STAGES_DEFAULT >= 1 && NTT_STAGES_DEFAULT <= NTT_STAGES_MAX, "the default is a legal pin");
constexpr size_t NTT_GRID_CAP = (size_t)1 << 20; // blocks of one launch; more work than that is walked with a grid stride
// exponents / elements a lane of the table kernel / the scale kernel walks, NTT_BLOCK apart: a block covers NTT_BLOCK times as many
constexpr int NTT_TABLE_LANE_ELEMS = 16;
constexpr int NTT_SCALE_LANE_ELEMS = 16;
constexpr size_t NTT_CONST_WORDS = 4;            // the shift as the element-wise kernel multiplies it in (g, or g^-1 for the inverse), formed on the device

constexpr bool stages_ok(int stages) { return stages < 0 || (stages >= 1 && stages <= NTT_STAGES_MAX); }
constexpr int stages_or_default(int stages) { return stages < 0 ? NTT_STAGES_DEFAULT : stages; }

// ---- the passes: Stockham autosort, pass p a radix-2^s step from natural order to natural order --------------------------------------
constexpr int passes(int log_n, int stages) { return (log_n + stages - 1) / stages; }
// every pass has `stages` stages but the last, which has what is left
constexpr int pass_stages(int log_n, int stages, int p) { return p + 1 < passes(log_n, stages) ? stages : log_n - p * stages; }
// log2 of the length of the sub-transforms the passes before p have finished
constexpr int pass_done_log(int stages, int p) { return p * stages; }
// log2 of the groups one tile of a pass of s stages holds side by side
constexpr int pass_group_log(int log_n, int s) { return NTT_TILE_LOG - s < log_n - s ? NTT_TILE_LOG - s : log_n - s; }
constexpr size_t pass_tiles(int log_n, int s) { return (size_t)1 << (log_n - s - pass_group_log(log_n, s)); }
// (array, tile) pairs: the work items of a pass.  m 2^log_n is the caller's array; no product here is larger than it
constexpr size_t pass_items(int log_n, int s, size_t m) { return pass_tiles(log_n, s) * m; }
constexpr size_t grid(size_t items) { return items < NTT_GRID_CAP ? (items ? items : 1) : NTT_GRID_CAP; }

// ---- the table: w_n^e, e < n / 2, [4][n / 2]; the inverse reads it too (w^-e = -w^(n/2 - e)) ------------------------------------------
constexpr size_t table_elems(int log_n) { return log_n ? (size_t)1 << (log_n - 1) : 0; }
constexpr size_t table_words(int log_n) { return 4 * table_elems(log_n); }
constexpr size_t table_blocks(int log_n) {
  return (table_elems(log_n) + (size_t)NTT_BLOCK * NTT_TABLE_LANE_ELEMS - 1) / ((size_t)NTT_BLOCK * NTT_TABLE_LANE_ELEMS);
}
// the powers past the table: w^i for i < n is w^(i - n / 2) negated from n / 2 on, and 1 at n = 1, where there is no table
constexpr size_t root_words(int log_n) { return table_words(log_n); }
constexpr bool root_negated(size_t i, int log_n) { return log_n >= 1 && i >= elems(log_n - 1); }
constexpr size_t root_slot(size_t i, int log_n) { return root_negated(i, log_n) ? i - elems(log_n - 1) : i; }
// squarings from the 2^28-th root W down to w_n
constexpr int root_squarings(int log_n) { return NTT_LOG_N_MAX - log_n; }

// ---- the element-wise kernel out_k = c s^k a_k: the forward coset shift BEFORE the passes, the inverse's closing scale AFTER them, and the
// whole of a transform that has no pass (n = 1: the value mod r) -------------------------------------------------------------------------
constexpr bool scales(int log_n, bool inverse, bool shifted) { return inverse || shifted || log_n == 0; }
constexpr size_t scale_chunks(int log_n) {
  return (elems(log_n) + (size_t)NTT_BLOCK * NTT_SCALE_LANE_ELEMS - 1) / ((size_t)NTT_BLOCK * NTT_SCALE_LANE_ELEMS);
}
constexpr size_t scale_items(int log_n, size_t m) { return scale_chunks(log_n) * m; }

// ---- the ping-pong: the steps of a call (passes and the element-wise kernel) alternate between `out` and one leased buffer so that the
// LAST step writes `out`; step 0 reads the caller's input --------------------------------------------------------------------------------
constexpr int steps(int log_n, int stages, bool inverse, bool shifted) { return passes(log_n, stages) + (scales(log_n, inverse, shifted) ? 1 : 0); }
constexpr bool step_writes_out(int n_steps, int i) { return ((n_steps - 1 - i) & 1) == 0; }
constexpr bool needs_buffer(int n_steps) { return n_steps >= 2; }
// u64 words of one buffer of the batch, [m][4][n], saturated
constexpr size_t batch_words(int log_n, size_t m) { return mul_sat(mul_sat(4, elems(log_n)), m); }
// what a call leases: the shift, the table, the ping-pong buffer
struct ScratchLayout { size_t consts, table, buf, bytes; };
constexpr ScratchLayout scratch_layout(int log_n, size_t m, int n_steps) {
  Carve c; ScratchLayout l{};
  l.consts = c.words(NTT_CONST_WORDS);
  l.table = c.words(table_words(log_n));
  l.buf = c.words(needs_buffer(n_steps) ? batch_words(log_n, m) : 0);
  l.bytes = c.at; return l;
}
constexpr size_t scratch_words(int log_n, size_t m, int n_steps) { return words_of(scratch_layout(log_n, m, n_steps).bytes); }

// ---- n^-1 = r - ((r - 1) >> log_n): n (-(r - 1) / n) = 1 - r = 1 mod r, and 2^log_n divides r - 1 for log_n <= 28 ------------------------
struct Words4 {
  uint64_t w[4];
};
constexpr Words4 FR_R = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
constexpr Words4 n_inverse(int log_n) {
  Words4 q = {{FR_R.w[0] - 1, FR_R.w[1], FR_R.w[2], FR_R.w[3]}};           // r - 1: r is odd, no borrow
  if (log_n)
    for (int i = 0; i < 4; ++i) q.w[i] = (q.w[i] >> log_n) | (i < 3 ? q.w[i + 1] << (64 - log_n) : 0);
  Words4 out = {{0, 0, 0, 0}};
  uint64_t borrow = 0;
  for (int i = 0; i < 4; ++i) {
    const uint64_t a = FR_R.w[i], b = q.w[i], d = a - b - borrow;
    borrow = (a < b) || (a == b && borrow) ? 1 : 0;
    out.w[i] = d;
  }
  return out;
}
}  // namespace ntt_plan
