// kzg_multi_plan.hpp -- the geometry of the grouped linear combination over Fr and the routes of the folded KZG openings (kzg_multi.hip):
// tiles, grids, the flush length, how group_start travels to the device, scratch sizes and offsets, and the chunks of the combined commitments.  Plain
// C++ so that tests/cpp/kzg_multi_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch code asks these functions and
// decides nothing itself.
#pragma once
#include "plan_base.hpp"

namespace kzgm_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::words_of;
// ---- groups ------------------------------------------------------------------------------------------------------------------------
// group_start is a HOST array of G + 1 offsets: non-decreasing, group_start[0] = 0, group_start[G] = m.  Empty groups are legal.
constexpr bool groups_ok(const uint64_t* group_start, size_t G, size_t m) {
  if (!group_start || group_start[0] != 0 || group_start[G] != m) return false;
  for (size_t g = 0; g < G; ++g)
    if (group_start[g] > group_start[g + 1]) return false;
  return true;
}
constexpr size_t longest_group(const uint64_t* group_start, size_t g0, size_t g1) {
  size_t c = 0;
  for (size_t g = g0; g < g1; ++g)
    if (group_start[g + 1] - group_start[g] > c) c = (size_t)(group_start[g + 1] - group_start[g]);
  return c;
}
// The offsets reach the device INSIDE KERNEL ARGUMENTS, KZGM_OFFSET_ARGS of them per launch of a one-block kernel that stores them to leased
// scratch: a launch copies its arguments before it returns, so the host array is read when the entry point returns, without a copy engine,
// a pinned buffer or a stream synchronisation.  2 KB of the 4 KB a launch may carry.
constexpr size_t KZGM_OFFSET_ARGS = 256;
constexpr size_t offset_launches(size_t G) { return (G + 1 + KZGM_OFFSET_ARGS - 1) / KZGM_OFFSET_ARGS; }
constexpr size_t offset_words(size_t G) { return G + 1; }

// ---- the linear combination: out_g[k] = sum_{j in g} w_j a_j[k] ----------------------------------------------------------------------
// A lane owns ONE coefficient column k and walks the polynomials of its group; a block of KZGM_BLOCK lanes owns a tile of KZGM_LINCOMB_TILE
// consecutive columns, so the four limb planes of a_j are read coalesced.  Work items are (group, tile) pairs: tiles along the grid's x,
// groups along its y, both walked with a stride past their caps.
constexpr int KZGM_BLOCK = 256;                        // == BLOCK of common.hpp (kzg_multi.hip asserts it)
constexpr size_t KZGM_LINCOMB_TILE = 256;              // T: columns per block, one per lane
static_assert(KZGM_LINCOMB_TILE == (size_t)KZGM_BLOCK, "one column per lane");
// products a lane adds unreduced between two reductions, and the weights a block stages in LDS per round.  THE BOUND: the accumulator enters a
// round as a residue below r and takes at most 16 products of canonical factors: r + 16 r^2 < 2^512 (r < 0.19 * 2^256, so 16 r^2 < 0.58 * 2^512).
constexpr int KZGM_LINCOMB_FLUSH = 16;                 // FL
constexpr size_t KZGM_GRID_X_CAP = (size_t)1 << 16;    // tiles of one launch
constexpr size_t KZGM_GRID_Y_CAP = 1024;               // groups of one launch (the hardware's limit is 65535)
constexpr size_t lincomb_tiles(size_t len) { return len / KZGM_LINCOMB_TILE + (len % KZGM_LINCOMB_TILE ? 1 : 0); }
constexpr size_t lincomb_grid_x(size_t len) { return lincomb_tiles(len) < KZGM_GRID_X_CAP ? lincomb_tiles(len) : KZGM_GRID_X_CAP; }
constexpr size_t lincomb_grid_y(size_t G) { return G < KZGM_GRID_Y_CAP ? G : KZGM_GRID_Y_CAP; }
// reductions a lane runs for a group of c polynomials (0 for an empty group: it stores zero)
constexpr size_t lincomb_rounds(size_t c) { return (c + KZGM_LINCOMB_FLUSH - 1) / KZGM_LINCOMB_FLUSH; }

// ---- one lane per polynomial (the powers, z spread to the polynomials) and one block per group (y_F) --------------------------------
constexpr size_t KZGM_LANE_GRID_CAP = (size_t)1 << 20;
constexpr size_t lane_grid(size_t n) { return (n + KZGM_BLOCK - 1) / KZGM_BLOCK < KZGM_LANE_GRID_CAP ? (n + KZGM_BLOCK - 1) / KZGM_BLOCK : KZGM_LANE_GRID_CAP; }
constexpr size_t group_grid(size_t G) { return G < KZGM_LANE_GRID_CAP ? G : KZGM_LANE_GRID_CAP; }

// ---- scratch, in u64 words; (size_t)-1 = does not fit size_t (the entry point refuses it before the lease) ----------------------------
constexpr size_t sat_mul(size_t a, size_t b) { return a && b > SAT / a ? SAT : a * b; }
constexpr size_t sat_add(size_t a, size_t b) { return a > SAT - b ? SAT : a + b; }
// the offsets alone
constexpr size_t offset_bytes(size_t G) { return sat_mul(offset_words(G), 8); }
// the prover: the offsets, the powers [4][m], z spread [4][m], the folded polynomials [G][4][len] (32 G len bytes) and their values [4][G]
struct OpenLayout { size_t gs, pow, zs, f, yf, bytes; };
constexpr OpenLayout open_layout(size_t len, size_t m, size_t G) {
  Carve c; OpenLayout l{};
  l.gs = c.words(offset_words(G));
  l.pow = c.words(sat_mul(4, m));
  l.zs = c.words(sat_mul(4, m));
  l.f = c.words(sat_mul(sat_mul(4, G), len));
  l.yf = c.words(sat_mul(4, G));
  l.bytes = c.at; return l;
}
constexpr size_t open_scratch_words(size_t len, size_t m, size_t G) { return words_of(open_layout(len, m, G).bytes); }
// the verifier's calls: the offsets and the powers [4][m]
struct CombineLayout { size_t gs, pow, bytes; };
constexpr CombineLayout combine_layout(size_t m, size_t G) {
  Carve c; CombineLayout l{};
  l.gs = c.words(offset_words(G));
  l.pow = c.words(sat_mul(4, m));
  l.bytes = c.at; return l;
}
constexpr size_t combine_scratch_words(size_t m, size_t G) { return words_of(combine_layout(m, G).bytes); }
// one chunk of the combined commitments, n = n_seg * terms slots: the scalars [4][n], the bases and the products [8][n] each, the segmented
// sum's w_acc words, the chunk's sums [8][n_seg]; then the flags of the bases and of the products [n] each and of the sums [n_seg]
struct ChunkLayout { size_t sc, bases, prod, acc, part, flags, prod_inf, part_inf, bytes; };
constexpr ChunkLayout chunk_layout(size_t n, size_t n_seg, size_t w_acc) {
  Carve c; ChunkLayout l{};
  l.sc = c.words(sat_mul(4, n));
  l.bases = c.words(sat_mul(8, n));
  l.prod = c.words(sat_mul(8, n));
  l.acc = c.words(w_acc);
  l.part = c.words(sat_mul(8, n_seg));
  l.flags = c.bytes(n);
  l.prod_inf = c.bytes(n);
  l.part_inf = c.bytes(n_seg);
  l.bytes = c.at; return l;
}
// sylow_hip_kzg_verify_multi_batch on top of that: C_F [8][G], y_F [4][G] and the flags [G] (rounded up to words)
struct VerifyLayout { size_t cf, yf, cf_inf, bytes; };
constexpr VerifyLayout verify_layout(size_t G) {
  Carve c; VerifyLayout l{};
  l.cf = c.words(sat_mul(8, G));
  l.yf = c.words(sat_mul(4, G));
  l.cf_inf = c.bytes(G);
  c.round();
  l.bytes = c.at; return l;
}
constexpr size_t verify_scratch_words(size_t G) { return words_of(verify_layout(G).bytes); }

// ---- the combined commitments: C_F,g = sum_j gamma_g^i C_j ---------------------------------------------------------------------------
enum class Route {
  SEGMENTS,    // a chunk of whole groups, every group padded to the longest with (identity, 0): ONE sylow_hip_g1_scalar_mul_batch, then g1h::sum_segments
  MSM,         // ONE group through sylow_hip_g1_msm: at or above its crossover, or too long for the budget on its own
};
// bytes the padded layout takes per (group, term) slot: the figure of the short commitment route (kzg_prove_plan.hpp: the window table, the
// scalar, the base, the product and its flag, the partial sums) and the flag of the base
constexpr size_t KZGM_BYTES_PER_SLOT = 1024 + 32 + 64 + 64 + 8 + 96 + 8;
struct CombineChunk {
  Route route;
  size_t g_end;      // the chunk holds the groups g0 .. g_end - 1; g_end > g0
  size_t terms;      // slots per group: the longest group of the chunk, at least 1 (SEGMENTS); the group's length (MSM)
};
// The chunk that starts at group g0 < G.  msm_min: the smallest group that takes sylow_hip_g1_msm; budget: the scratch limit in force.  A
// SEGMENTS chunk grows while the next group is below msm_min and (groups) * (longest) slots still fit the budget; a group that does not fit
// alone goes through sylow_hip_g1_msm, which cuts its own work to the budget.
constexpr CombineChunk combine_chunk(const uint64_t* group_start, size_t G, size_t g0, size_t msm_min, size_t budget) {
  const size_t first = (size_t)(group_start[g0 + 1] - group_start[g0]);
  const size_t slots = budget / KZGM_BYTES_PER_SLOT;
  if (first && (first >= msm_min || first > slots)) return CombineChunk{Route::MSM, g0 + 1, first};      // an empty group is a SEGMENTS slot
  size_t c = first ? first : 1, g = g0 + 1;
  for (; g < G; ++g) {
    const size_t n = (size_t)(group_start[g + 1] - group_start[g]), cc = n > c ? n : c;
    if (n >= msm_min || sat_mul(g + 1 - g0, cc) > slots) break;
    c = cc;
  }
  return CombineChunk{Route::SEGMENTS, g, c};
}
}  // namespace kzgm_plan
