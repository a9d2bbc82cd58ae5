// kzg_evals_plan.hpp -- the geometry of the shared-inverse batch inversion in Fr and of the KZG quotient from evaluations (kzg_evals.hip):
// every size, grid, scratch size and offset, and route decision between an entry point and its kernels, plain C++ so that tests/cpp/kzg_evals_plan_test.cpp
// can compile it with g++ on a box without a GPU.  The launch code asks these functions and decides nothing itself.
#pragma once
#include "plan_base.hpp"

namespace kzg_evals_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::elems;
using plan_base::mul_sat;
using plan_base::words_of;
// ---- the chunk: a lane owns EVALS_LANE_ELEMS consecutive elements, a block of EVALS_BLOCK lanes a chunk of EVALS_CHUNK -------------------
// The elements of a chunk share ONE inversion: prefix products inside a lane, a prefix and a suffix scan of the lane totals through LDS, the
// inverse of the chunk's product on one lane (bn254_fr_euclid.hpp), and the way back.  There is no level above the chunk: every chunk pays
// its own inversion, beside the other blocks' work, so the call has no capacity of its own and no scratch.
constexpr int EVALS_BLOCK = 256;                 // == BLOCK of common.hpp (kzg_evals.hip asserts it)
constexpr int EVALS_LANE_ELEMS = 8;              // L: the lane keeps L prefix products in registers (64 VGPRs)
constexpr size_t EVALS_CHUNK = 2048;             // CH = EVALS_BLOCK * EVALS_LANE_ELEMS
static_assert(EVALS_CHUNK == (size_t)EVALS_BLOCK * EVALS_LANE_ELEMS, "a chunk is a block of lanes");
constexpr size_t EVALS_GRID_CAP = (size_t)1 << 20;       // blocks of one launch; more work than that is walked with a grid stride
constexpr int EVALS_LOG_N_MAX = 28;              // r - 1 = 2^28 * odd, as ntt_plan.hpp

constexpr size_t chunks(size_t n) { return n / EVALS_CHUNK + (n % EVALS_CHUNK ? 1 : 0); }
constexpr size_t grid(size_t items) { return items < EVALS_GRID_CAP ? items : EVALS_GRID_CAP; }
// lanes of chunk c of an array of n elements that own an element (c < chunks(n)); the scans run over these alone
constexpr int live_lanes(size_t n, size_t c) {
  return n - c * EVALS_CHUNK >= EVALS_CHUNK ? EVALS_BLOCK : (int)((n - c * EVALS_CHUNK + EVALS_LANE_ELEMS - 1) / EVALS_LANE_ELEMS);
}
// doubling steps of a scan over `live` lanes: the smallest s with 2^s >= live
constexpr int scan_steps(int live) {
  int s = 0;
  while ((1 << s) < live) ++s;
  return s;
}
// [a, a + bytes) and [b, b + bytes) share a byte (the ends cannot wrap: both are arrays the caller holds)
constexpr bool overlaps(uintptr_t a, uintptr_t b, size_t bytes) { return bytes && !(a + bytes <= b || b + bytes <= a); }

// ---- sylow_hip_fr_batch_inv: ONE launch, a block per chunk, no scratch --------------------------------------------------------------------
constexpr size_t batch_inv_grid(size_t n) { return grid(chunks(n)); }
constexpr size_t fr_array_bytes(size_t n) { return mul_sat(mul_sat(n, 4), sizeof(uint64_t)); }

// ---- the quotient from evaluations: m polynomials of n = 2^log_n values ----------------------------------------------------------------
// Launches, in stream order:  roots (one wavefront: w^(2^s), s < log_n, and w^-1, shared by every block of the call);  dinv (a block per
// (polynomial, chunk): d_i^-1 into q_out, the chunk's part of sum f_i w^i / d_i, the index of a hit);  value (a block per polynomial: y);
// and, when the quotient is wanted,  quot (a block per (polynomial, chunk): q_i over d_i^-1 in place, and for a row with a hit the chunk's
// part of sum q_i w^i)  and  repair (a block per polynomial: q_k of a row with a hit).
constexpr size_t poly_chunks(int log_n) { return chunks(elems(log_n)); }
// (polynomial, chunk) pairs.  m 2^log_n is the caller's array; no product here is larger than it
constexpr size_t items(int log_n, size_t m) { return poly_chunks(log_n) * m; }
constexpr size_t ROOT_SLOTS = EVALS_LOG_N_MAX + 1;       // w^(2^s) at slot s < 28, w^-1 at slot 28; 4 words each
constexpr size_t roots_words() { return 4 * ROOT_SLOTS; }
// u64 words a call leases: the roots, the chunk sums [4][items] (the first sum's, then the second's), the hit index per polynomial [m],
// and y [4][m] when the caller wants none (the quotient still needs it)
struct QuotientLayout { size_t roots, totals, hit, y, bytes; };
constexpr QuotientLayout quotient_layout(int log_n, size_t m, bool has_y_out) {
  Carve c; QuotientLayout l{};
  l.roots = c.words(roots_words());
  l.totals = c.words(mul_sat(4, items(log_n, m)));
  l.hit = c.words(m);
  l.y = c.words(has_y_out ? 0 : mul_sat(4, m));
  l.bytes = c.at; return l;
}
constexpr size_t quotient_scratch_words(int log_n, size_t m, bool has_y_out) { return words_of(quotient_layout(log_n, m, has_y_out).bytes); }
constexpr size_t batch_words(int log_n, size_t m) { return mul_sat(mul_sat(4, elems(log_n)), m); }
constexpr uint64_t NO_HIT = ~(uint64_t)0;        // the hit slot of a polynomial whose z is outside the domain (k_evals_roots clears every slot to it)

// ---- the opening: the quotient's values into a leased [m][4][n], then the commitment over the Lagrange SRS -----------------------------
// The quotient's words are canonical, so the commitment is entered past its mod-r pass (kzg_prove.hip exports that entry to this unit).
constexpr size_t open_scratch_words(int log_n, size_t m) { return batch_words(log_n, m); }
constexpr size_t open_scratch_bytes(int log_n, size_t m) { return mul_sat(open_scratch_words(log_n, m), sizeof(uint64_t)); }
}  // namespace kzg_evals_plan
