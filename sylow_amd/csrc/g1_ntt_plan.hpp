// g1_ntt_plan.hpp -- the geometry of the radix-2 transform over G1 points (g1_ntt.hip): the butterflies of a stage and their indices, which
// lane takes which butterfly, the grid cap, the ping-pong between the projective buffers, the window tables and the scratch with its offsets, plain C++ so that
// tests/cpp/g1_ntt_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch code asks these functions and decides nothing itself.
#pragma once
#include "ntt_plan.hpp"

namespace g1_ntt_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::elems;
using plan_base::max_blocks_ok;
using plan_base::mul_sat;
constexpr int G1_NTT_LOG_N_MAX = ntt_plan::NTT_LOG_N_MAX;
constexpr int G1_NTT_BLOCK = 256;                        // == BLOCK of common.hpp (g1_ntt.hip asserts it)
// A lane that multiplies keeps a window table of 1 KB in global memory (bn254_pairing.hpp: G1TableGlobal).  The tables are leased per RESIDENT
// lane: the scalar-multiplication kernels run two wavefronts per SIMD (HEAVY_BOUNDS), eight per CU, two blocks of 256 lanes per CU, so 512
// blocks fill the 256 CUs of the target once and a larger grid would only queue.  Lanes walk further butterflies with a grid stride.
constexpr size_t G1_NTT_GRID_DEFAULT = 512;
constexpr size_t G1_NTT_GRID_MAX = 4096;                 // what a pin may raise it to (1 GB of tables); a larger pin is this
constexpr size_t G1_NTT_TABLE_BYTES_PER_LANE = 1024;     // == G1_TABLE_BYTES_PER_LANE (g1_ntt.hip asserts it)
constexpr size_t G1_NTT_PROJ_WORDS = 12, G1_NTT_AFFINE_WORDS = 8;

constexpr bool log_n_ok(int log_n) { return log_n >= 0 && log_n <= G1_NTT_LOG_N_MAX; }
constexpr size_t half(int log_n) { return log_n ? (size_t)1 << (log_n - 1) : 0; }
// points of the batch, m n, and the bytes of the caller's arrays (saturated): [m][8][n] words and [m][n] flags
constexpr size_t points(int log_n, size_t m) { return mul_sat(elems(log_n), m); }
constexpr size_t xy_bytes(int log_n, size_t m) { return mul_sat(points(log_n, m), G1_NTT_AFFINE_WORDS * sizeof(uint64_t)); }
constexpr size_t inf_bytes(int log_n, size_t m) { return points(log_n, m); }
// two byte ranges of `bytes` bytes each do not overlap (bytes != SAT; the sums cannot wrap for ranges that exist)
constexpr bool disjoint(uintptr_t a, uintptr_t b, size_t bytes) { return a + bytes <= b || b + bytes <= a; }

// ---- the stages: radix-2 Stockham, stage p from natural order to natural order.  With Ns = 2^p and butterfly j < n / 2:
//   U = in[j],  V = w^(+-(j mod Ns) n / (2 Ns)) in[j + n / 2],   out[(j div Ns) 2 Ns + (j mod Ns)] = U + V,   the same + Ns = U - V
// (the addressing of the Fr transform's pass at one stage per pass).  Every index below is < n for j < n / 2.
constexpr int stages(int log_n) { return log_n; }
constexpr size_t in0(size_t j) { return j; }
constexpr size_t in1(size_t j, int log_n) { return j + half(log_n); }
constexpr size_t out0(size_t j, int stage) { return ((j >> stage) << (stage + 1)) + (j & (((size_t)1 << stage) - 1)); }
constexpr size_t out1(size_t j, int stage) { return out0(j, stage) + ((size_t)1 << stage); }
// e < n / 2 with twiddle w^e (inverse: w^-e = -w^(n/2 - e) for e > 0): the table of the first half serves both directions
constexpr size_t twiddle_exp(size_t j, int log_n, int stage) { return (j & (((size_t)1 << stage) - 1)) << (log_n - 1 - stage); }
// the butterflies that multiply by 1 and so do not multiply: all of stage 0, one in Ns after it
constexpr bool unit_twiddle(size_t j, int stage) { return (j & (((size_t)1 << stage) - 1)) == 0; }
// Which butterfly work item q < n / 2 is.  With G = n / (2 Ns) groups, item q is butterfly (q mod G) Ns + (q div G): consecutive items -- the
// lanes of a wavefront -- share j mod Ns, so the unit twiddles are the items q < G, whole wavefronts of them wherever G >= 64, and a
// wavefront never waits for a multiplication that one lane in Ns skips.  A bijection of [0, n / 2); the identity at stage 0.  It costs the
// coalescing of the loads (stride Ns), which a butterfly of some 10^5 instructions per 300 bytes does not notice.
constexpr size_t butterfly_of(size_t q, int log_n, int stage) {
  return ((q & (((size_t)1 << (log_n - 1 - stage)) - 1)) << stage) | (q >> (log_n - 1 - stage));
}
// butterflies of a stage over the batch (saturated), and the scalar multiplications of ONE array's transform without the closing scale:
// sum over p >= 1 of (n / 2)(1 - 2^-p)
constexpr size_t butterflies(int log_n, size_t m) { return mul_sat(half(log_n), m); }
constexpr size_t multiplications(int log_n) {
  size_t s = 0;
  for (int p = 1; p < log_n; ++p) s += half(log_n) - (half(log_n) >> p);
  return s;
}
constexpr bool stage_multiplies(int stage) { return stage >= 1; }

// ---- grids: a launch has one lane per item up to the cap; the rest is walked with a grid stride ------------------------------------------
constexpr size_t grid_cap(long long max_blocks) {
  return max_blocks < 0 ? G1_NTT_GRID_DEFAULT : (size_t)max_blocks < G1_NTT_GRID_MAX ? (size_t)max_blocks : G1_NTT_GRID_MAX;
}
constexpr size_t blocks_for(size_t items) { return items / G1_NTT_BLOCK + (items % G1_NTT_BLOCK ? 1 : 0); }
constexpr size_t grid(size_t items, long long max_blocks) {
  return blocks_for(items) < grid_cap(max_blocks) ? (blocks_for(items) ? blocks_for(items) : 1) : grid_cap(max_blocks);
}
constexpr size_t stage_grid(int log_n, size_t m, long long max_blocks) { return grid(butterflies(log_n, m), max_blocks); }
// the closing kernel: one item per point; it multiplies (by n^-1) only for an inverse of more than one point
constexpr bool closing_scales(int log_n, bool inverse) { return inverse && log_n > 0; }
constexpr size_t closing_grid(int log_n, size_t m, long long max_blocks) { return grid(points(log_n, m), max_blocks); }

// ---- window tables: one region per lane of the LARGEST multiplying launch of the call; a function of the grid, never of n -----------------
constexpr size_t table_lanes(int log_n, size_t m, bool inverse, long long max_blocks) {
  const size_t a = log_n >= 2 ? stage_grid(log_n, m, max_blocks) : 0, b = closing_scales(log_n, inverse) ? closing_grid(log_n, m, max_blocks) : 0;
  return (a > b ? a : b) * G1_NTT_BLOCK;
}
constexpr size_t table_bytes(int log_n, size_t m, bool inverse, long long max_blocks) {
  return table_lanes(log_n, m, inverse, max_blocks) * G1_NTT_TABLE_BYTES_PER_LANE;
}

// ---- the ping-pong: stage p reads the caller's input (p = 0) or buffer (p - 1) & 1 and writes buffer p & 1; the closing kernel, the LAST
// step of every call, reads the last stage's buffer (the caller's input when there is no stage) and writes the caller's output.  Buffers
// are projective, [12][m n] words each, point k of array a at column a n + k ----------------------------------------------------------
constexpr int SRC_INPUT = -1;
constexpr int steps(int log_n) { return stages(log_n) + 1; }
constexpr int stage_src(int stage) { return stage ? (stage - 1) & 1 : SRC_INPUT; }
constexpr int stage_dst(int stage) { return stage & 1; }
constexpr int closing_src(int log_n) { return log_n ? (log_n - 1) & 1 : SRC_INPUT; }
constexpr bool step_writes_out(int log_n, int step) { return step == steps(log_n) - 1; }
constexpr int buffers(int log_n) { return log_n >= 2 ? 2 : log_n; }
constexpr size_t buffer_words(int log_n, size_t m) { return mul_sat(points(log_n, m), G1_NTT_PROJ_WORDS); }

// ---- the scratch of a call, bytes, saturated: the window tables (16-byte loads: first), the twiddle table, the buffers -----------------------------------
constexpr size_t twiddle_words(int log_n) { return ntt_plan::table_words(log_n); }
struct ScratchLayout { size_t tables, twiddles, buf[2], bytes; };
constexpr ScratchLayout scratch_layout(int log_n, size_t m, bool inverse, long long max_blocks) {
  Carve c; ScratchLayout l{};
  l.tables = c.bytes(table_bytes(log_n, m, inverse, max_blocks));      // a multiple of 1 KB: the words after it stay aligned
  l.twiddles = c.words(twiddle_words(log_n));
  l.buf[0] = c.words(buffers(log_n) > 0 ? buffer_words(log_n, m) : 0);
  l.buf[1] = c.words(buffers(log_n) > 1 ? buffer_words(log_n, m) : 0);
  l.bytes = c.at; return l;
}
constexpr size_t scratch_bytes(int log_n, size_t m, bool inverse, long long max_blocks) { return scratch_layout(log_n, m, inverse, max_blocks).bytes; }
}  // namespace g1_ntt_plan
