// kzg_open_all_plan.hpp -- the geometry of the KZG proofs of one polynomial at ALL n = 2^log_n points of its domain (kzg_open_all.hip, the
// Feist-Khovratovich construction): the array x the table is the transform of, the fused first stage of the size-2n inverse transform, the
// first stage of the size-n forward transform that reads h out of the wider arrays, the ping-pong through both transforms, where the Fr
// arrays live, the window tables and the scratch with its offsets, plain C++ so that tests/cpp/kzg_open_all_plan_test.cpp can compile it with g++ on a box
// without a GPU.  The launch code asks these functions and decides nothing itself.  The stages between the two first stages and the closing
// kernel are g1_ntt.hip's, with the indices of g1_ntt_plan.hpp.
#pragma once
#include "g1_ntt_plan.hpp"

namespace kzg_open_all_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::disjoint;
using plan_base::elems;
using plan_base::max_blocks_ok;
using plan_base::mul_sat;
using plan_base::words_of;
using g1_ntt_plan::G1_NTT_AFFINE_WORDS;
using g1_ntt_plan::G1_NTT_PROJ_WORDS;
constexpr int OPEN_ALL_LOG_N_MAX = g1_ntt_plan::G1_NTT_LOG_N_MAX - 1;        // the transform of 2n points must fit the 2^28 roots
constexpr size_t FR_WORDS = 4;

constexpr bool log_n_ok(int log_n) { return log_n >= 0 && log_n <= OPEN_ALL_LOG_N_MAX; }
constexpr int wide_log(int log_n) { return log_n + 1; }                      // the convolution runs on 2n points
constexpr size_t wide(int log_n) { return (size_t)2 << log_n; }
// the caller's arrays, bytes, saturated: the table [8][2n] + [2n], the polynomials and y [m][4][n], the proofs [m][8][n] + [m][n]
constexpr size_t table_xy_bytes(int log_n) { return g1_ntt_plan::xy_bytes(wide_log(log_n), 1); }
constexpr size_t fr_bytes(int log_n, size_t m) { return mul_sat(mul_sat(elems(log_n), m), FR_WORDS * sizeof(uint64_t)); }
constexpr size_t pi_xy_bytes(int log_n, size_t m) { return g1_ntt_plan::xy_bytes(log_n, m); }

// ---- the table: T = the forward transform of x, 2n points with x_(2n-1-t) = s_t for t <= n - 2 and the identity everywhere else -------------
// which SRS point column k < 2n of x holds, or X_IDENTITY: s_(n-1) is not used, and columns 0 .. n hold the identity
constexpr size_t X_IDENTITY = SAT;
constexpr size_t x_srs_index(size_t k, int log_n) { return k > elems(log_n) ? wide(log_n) - 1 - k : X_IDENTITY; }
// scratch of prepare: x as affine words + flags, [8][2n] words then [2n] bytes
struct PrepareLayout { size_t xy, inf, bytes; };
constexpr PrepareLayout prepare_layout(int log_n) {
  Carve c; PrepareLayout l{};
  l.xy = c.words(words_of(table_xy_bytes(log_n)));
  l.inf = c.bytes(wide(log_n));
  l.bytes = c.at; return l;
}
constexpr size_t prepare_scratch_bytes(int log_n) { return prepare_layout(log_n).bytes; }
constexpr size_t prepare_grid(int log_n) { return g1_ntt_plan::blocks_for(wide(log_n)); }

// ---- per polynomial.  log_n = 0 has one proof, the identity (h_(n-1) is the identity): one launch writes it and nothing below runs.
// From log_n = 1 on, with L = log_n + 1:
//   pad      P = (2n)^-1 f mod r, then n zeros                           [m][4][2n]   (the inverse transform's scale, folded into the scalars)
//   Fr       F = the Fr transform of P (ntt.hip)                          [m][4][2n]
//   first    stage 0 of the size-2n INVERSE transform fused with the pointwise products: butterfly j < n of array a has
//            U = F_j T_j, V = F_(j+n) T_(j+n), out[2j] = U + V, out[2j + 1] = U - V at columns a 2n + ... of a projective buffer [12][m 2n]
//   inverse  stages 1 .. L - 1 through g1_ntt.hip's stage kernel: h_b at column a 2n + b, b < n
//   forward  stage 0 of the size-n FORWARD transform: butterfly j < n / 2 reads columns a 2n + j and a 2n + j + n / 2, takes h_(n-1) as the
//            identity whatever the buffer holds, and writes columns a n + 2j and a n + 2j + 1 of the other buffer (the stride stays m 2n)
//   forward  stages 1 .. log_n - 1 through the stage kernel, then its closing kernel without a scale into the caller's arrays
constexpr bool trivial(int log_n) { return log_n == 0; }
constexpr size_t stride(int log_n, size_t m) { return mul_sat(wide(log_n), m); }                      // of both projective buffers
constexpr size_t first_items(int log_n, size_t m) { return mul_sat(elems(log_n), m); }                  // butterflies of the fused stage
constexpr size_t first_in0(size_t j) { return j; }
constexpr size_t first_in1(size_t j, int log_n) { return j + elems(log_n); }
constexpr size_t first_out0(size_t a, size_t j, int log_n) { return a * wide(log_n) + g1_ntt_plan::out0(j, 0); }
constexpr size_t first_out1(size_t a, size_t j, int log_n) { return a * wide(log_n) + g1_ntt_plan::out1(j, 0); }
constexpr size_t fwd_items(int log_n, size_t m) { return mul_sat(g1_ntt_plan::half(log_n), m); }
constexpr size_t fwd_in0(size_t a, size_t j, int log_n) { return a * wide(log_n) + j; }
constexpr size_t fwd_in1(size_t a, size_t j, int log_n) { return a * wide(log_n) + j + g1_ntt_plan::half(log_n); }
constexpr bool fwd_in1_is_identity(size_t j, int log_n) { return j + g1_ntt_plan::half(log_n) == elems(log_n) - 1; }    // h_(n-1)
constexpr size_t fwd_out0(size_t a, size_t j, int log_n) { return a * elems(log_n) + g1_ntt_plan::out0(j, 0); }
constexpr size_t fwd_out1(size_t a, size_t j, int log_n) { return a * elems(log_n) + g1_ntt_plan::out1(j, 0); }
// scalar multiplications per polynomial on the convolution route: 2n products, the stages p >= 1 of the inverse of 2n points, n (log_n - 1) + 1,
// and of the forward of n points, (n / 2)(log_n - 2) + 1  (log_n = 0: the two products of the route; the library runs none there)
constexpr size_t multiplications(int log_n) {
  return wide(log_n) + g1_ntt_plan::multiplications(wide_log(log_n)) + g1_ntt_plan::multiplications(log_n);
}

// ---- the ping-pong between two projective buffers: inverse stage s writes buffer s & 1, so h lies in buffer log_n & 1; forward stage s
// writes buffer (log_n + 1 + s) & 1; the closing kernel reads the last of them, buffer (2 log_n) & 1 = 0, and writes the caller's arrays --------
constexpr int inv_stages(int log_n) { return wide_log(log_n); }
constexpr int inv_dst(int s) { return s & 1; }
constexpr int inv_src(int s) { return (s - 1) & 1; }                         // s >= 1; stage 0 reads the table and F
constexpr int fwd_stages(int log_n) { return log_n; }
constexpr int fwd_src(int log_n, int s) { return (log_n + s) & 1; }
constexpr int fwd_dst(int log_n, int s) { return (log_n + 1 + s) & 1; }
constexpr int close_src(int log_n) { return fwd_dst(log_n, fwd_stages(log_n) - 1); }
constexpr size_t buffer_words(int log_n, size_t m) { return mul_sat(stride(log_n, m), G1_NTT_PROJ_WORDS); }
// P and F lie in buffer 1, which no stage writes before inverse stage 1 -- by then the fused stage has read F and nobody reads P
constexpr int FR_BUFFER = 1;
constexpr size_t padded_words(int log_n, size_t m) { return mul_sat(stride(log_n, m), FR_WORDS); }
constexpr size_t pad_offset() { return 0; }
constexpr size_t f_offset(int log_n, size_t m) { return padded_words(log_n, m); }
static_assert(2 * FR_WORDS <= G1_NTT_PROJ_WORDS, "P and F fit one projective buffer");

// ---- grids and window tables: the fused stage has the most items of the call (m n, as the inverse stages; the forward stages have half), so
// its grid sizes the tables: one region per lane, a function of the grid, never of n --------------------------------------------------------
constexpr size_t first_grid(int log_n, size_t m, long long max_blocks) { return g1_ntt_plan::grid(first_items(log_n, m), max_blocks); }
constexpr size_t fwd_grid(int log_n, size_t m, long long max_blocks) { return g1_ntt_plan::grid(fwd_items(log_n, m), max_blocks); }
constexpr size_t pad_grid(int log_n, size_t m) { return g1_ntt_plan::grid(stride(log_n, m), -1); }
constexpr size_t trivial_grid(size_t m) { return g1_ntt_plan::grid(m, -1); }
constexpr size_t table_lanes(int log_n, size_t m, long long max_blocks) { return first_grid(log_n, m, max_blocks) * g1_ntt_plan::G1_NTT_BLOCK; }
constexpr size_t table_bytes(int log_n, size_t m, long long max_blocks) { return table_lanes(log_n, m, max_blocks) * g1_ntt_plan::G1_NTT_TABLE_BYTES_PER_LANE; }

// ---- the scratch of a call, bytes, saturated: the window tables (16-byte loads: first), the twiddles of 2n and of n points, two buffers --------
constexpr size_t wide_twiddle_words(int log_n) { return g1_ntt_plan::twiddle_words(wide_log(log_n)); }
constexpr size_t twiddle_words(int log_n) { return g1_ntt_plan::twiddle_words(log_n); }
// padded and f are no regions of their own: they lie in buf[FR_BUFFER], at pad_offset() and f_offset() words
struct ScratchLayout { size_t tables, tw_wide, tw, buf[2], bytes, padded, f; };
constexpr ScratchLayout scratch_layout(int log_n, size_t m, long long max_blocks) {
  Carve c; ScratchLayout l{};
  if (trivial(log_n)) return l;
  l.tables = c.bytes(table_bytes(log_n, m, max_blocks));      // a multiple of 1 KB: the words after it stay aligned
  l.tw_wide = c.words(wide_twiddle_words(log_n));
  l.tw = c.words(twiddle_words(log_n));
  l.buf[0] = c.words(buffer_words(log_n, m));
  l.buf[1] = c.words(buffer_words(log_n, m));
  l.bytes = c.at;
  l.padded = add_sat(l.buf[FR_BUFFER], mul_sat(pad_offset(), 8));
  l.f = add_sat(l.buf[FR_BUFFER], mul_sat(f_offset(log_n, m), 8));
  return l;
}
constexpr size_t scratch_bytes(int log_n, size_t m, long long max_blocks) { return scratch_layout(log_n, m, max_blocks).bytes; }
}  // namespace kzg_open_all_plan
