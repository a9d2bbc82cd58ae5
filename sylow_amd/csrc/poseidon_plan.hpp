// poseidon_plan.hpp -- the geometry of Poseidon over Fr and of its binary Merkle trees (poseidon.hip): the widths and depths accepted, the
// parameter table, the two routes and the choice between them, lane groups, tiles and grids, the levels of a tree inside nodes_out and the
// byte counts of the caller's arrays, plain C++ so that tests/cpp/poseidon_plan_test.cpp can compile it with g++ on a box without a GPU.
// The launch code asks these functions and decides nothing itself.
#pragma once
#include "plan_base.hpp"
#include "poseidon_params.hpp"

namespace poseidon_plan {
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::disjoint;
using plan_base::elems;
using plan_base::max_blocks_ok;
using plan_base::mul_sat;
constexpr int POS_BLOCK = 256;                   // == BLOCK of common.hpp (poseidon.hip asserts it)
constexpr int POS_WAVE = 64;
constexpr int T_MIN = poseidon_params::T_MIN, T_MAX = poseidon_params::T_MAX;
constexpr int DEPTH_MIN = 1, DEPTH_MAX = 28;
constexpr int FULL_HALF = poseidon_params::FULL_ROUNDS / 2;   // full rounds before, and after, the partial ones
constexpr int MERKLE_T = 3;                      // a node is hash([left, right]): the width-3 table
constexpr size_t FR_WORDS = 4;
constexpr size_t POS_GRID_CAP = (size_t)1 << 20; // blocks of one launch; more work than that is walked with a grid stride
constexpr uint8_t STATUS_OUT_OF_RANGE = 1;       // bit 0 of a query's status: tree >= m or index >= 2^depth

constexpr bool width_ok(int t) { return poseidon_params::width_ok(t); }
constexpr bool inputs_ok(int k) { return width_ok(k + 1); }
constexpr bool depth_ok(int depth) { return depth >= DEPTH_MIN && depth <= DEPTH_MAX; }
constexpr int partial_rounds(int t) { return poseidon_params::partial_rounds(t); }
constexpr int rounds(int t) { return poseidon_params::rounds(t); }

// ---- the parameter table of a width, canonical, an element as 4 consecutive words (every lane of the narrow route reads the same element:
// one scalar load of 32 bytes): the (R_F + R_P) t round constants, round-major, then M row by row ------------------------------------------
constexpr size_t matrix_elem(int t) { return (size_t)rounds(t) * (size_t)t; }            // the element index M[0][0] sits at
constexpr size_t table_elems(int t) { return matrix_elem(t) + (size_t)t * (size_t)t; }
constexpr size_t table_words(int t) { return FR_WORDS * table_elems(t); }
constexpr size_t table_bytes(int t) { return table_words(t) * sizeof(uint64_t); }

// ---- the routes.  NARROW: a lane per permutation, the state in registers, every loop over the state unrolled.  WIDE: a lane per state
// element, in a group of group_lanes(t) lanes inside a wavefront ----------------------------------------------------------------------------
enum { ROUTE_NARROW = 0, ROUTE_WIDE = 1 };
constexpr bool route_ok(int route) { return route < 0 || route == ROUTE_NARROW || route == ROUTE_WIDE; }
// The widest state the narrow route holds without scratch: the compiler's resource report of poseidon.hip (make usage UNIT=poseidon) shows
// ScratchSize 0 and no spilled register for the narrow kernels up to this width (profiles/poseidon/kernel_usage.txt).  A wider state runs
// the wide route at every n, whatever the pin.
constexpr int NARROW_T_MAX = 5;
constexpr bool narrow_ok(int t) { return t <= NARROW_T_MAX; }
// The item count up to which a launch runs wide by default, per width class (the classes are the group sizes): the largest measured n at
// which the wide route is no slower than the narrow one (profiles/poseidon/bench_poseidon.json, one MI355X, median of 7, ms):
//     n            2^12    2^13    2^14    2^15    2^16    2^17
//     t = 3 narrow 0.681   0.683   0.678   0.684   0.715   1.003        t = 5 narrow 1.311   1.305   1.298   1.308   1.318   1.909
//     t = 3 wide   0.398   0.402   0.408   0.553   0.993   1.799        t = 5 wide   0.511   0.503   0.680   1.218   2.210   4.181
// Up to 2^15 items both routes sit on the latency of one chain of rounds, and the wide chain is the shorter one; from 2^16 on the narrow
// route has the throughput (2.0 x at t = 3, 2.5 x at t = 5).  Groups of two lanes (t = 2) were not measured and take the same limit.
constexpr size_t WIDE_MAX_G2 = (size_t)1 << 15, WIDE_MAX_G4 = (size_t)1 << 15, WIDE_MAX_G8 = (size_t)1 << 15;
constexpr int group_lanes(int t) { return t <= 2 ? 2 : t <= 4 ? 4 : t <= 8 ? 8 : t <= 16 ? 16 : 32; }   // the next power of two >= t
constexpr size_t wide_max_default(int t) { return group_lanes(t) == 2 ? WIDE_MAX_G2 : group_lanes(t) == 4 ? WIDE_MAX_G4 : WIDE_MAX_G8; }
// pin: < 0 the default, else a route; wide_max: < 0 the default, else the item count up to which the default route is the wide one
constexpr int choose_route(int t, size_t items, int pin, long long wide_max) {
  if (!narrow_ok(t)) return ROUTE_WIDE;
  if (pin >= 0) return pin;
  const size_t lim = wide_max < 0 ? wide_max_default(t) : (unsigned long long)wide_max > SAT ? SAT : (size_t)wide_max;
  return items <= lim ? ROUTE_WIDE : ROUTE_NARROW;
}
constexpr int groups_per_block(int t) { return POS_BLOCK / group_lanes(t); }
constexpr size_t ceil_div(size_t a, size_t b) { return a / b + (a % b ? 1 : 0); }
// blocks that hold every item once
constexpr size_t tiles(int t, size_t items, int route) { return ceil_div(items, route == ROUTE_WIDE ? (size_t)groups_per_block(t) : (size_t)POS_BLOCK); }
constexpr size_t grid(size_t blocks, long long max_blocks) {
  const size_t cap = max_blocks > 0 && (unsigned long long)max_blocks < POS_GRID_CAP ? (size_t)max_blocks : POS_GRID_CAP;
  return blocks < cap ? (blocks ? blocks : 1) : cap;
}

// ---- a tree of n = 2^depth leaves: level k = 1 .. depth has n / 2^k nodes and starts at n - 2^(depth - k + 1) of the n - 1 nodes; level
// depth is the root, the last node --------------------------------------------------------------------------------------------------------------
constexpr size_t level_nodes(int depth, int k) { return elems(depth - k); }
constexpr size_t level_offset(int depth, int k) { return elems(depth) - elems(depth - k + 1); }
constexpr size_t node_count(int depth) { return elems(depth) - 1; }
constexpr size_t level_items(int depth, int k, size_t m) { return mul_sat(level_nodes(depth, k), m); }

// ---- the caller's arrays, bytes, saturated ----------------------------------------------------------------------------------------------------
constexpr size_t fr_bytes(size_t count) { return mul_sat(mul_sat(count, FR_WORDS), sizeof(uint64_t)); }
constexpr size_t state_bytes(int t, size_t n) { return fr_bytes(mul_sat((size_t)t, n)); }
constexpr size_t leaves_bytes(int depth, size_t m) { return fr_bytes(mul_sat(elems(depth), m)); }
constexpr size_t nodes_bytes(int depth, size_t m) { return fr_bytes(mul_sat(node_count(depth), m)); }
constexpr size_t path_bytes(int depth, size_t q) { return fr_bytes(mul_sat((size_t)depth, q)); }
constexpr size_t index_bytes(size_t q) { return mul_sat(q, sizeof(uint64_t)); }
constexpr bool n_roots_ok(size_t n_roots, size_t q) { return n_roots == 1 || n_roots == q; }
}  // namespace poseidon_plan
