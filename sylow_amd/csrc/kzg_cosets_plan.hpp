// kzg_cosets_plan.hpp -- the geometry of the KZG proofs of one polynomial on EVERY COSET of its domain (kzg_cosets.hip, the multi-proof form
// of the Feist-Khovratovich construction): n = c l points cut into c = 2^log_c cosets of l = 2^log_l points, one proof per coset.  The l
// arrays x^(a) the table is the transform of, the split of a polynomial into its l residue arrays, the fused first stage with its planes, the
// fold of the planes, the ping-pong through both transforms (kzg_open_all_plan.hpp's with n -> c), the interpolation's twist, the window tables
// and the scratch with its offsets, plain C++ so that tests/cpp/kzg_cosets_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch code asks
// these functions and decides nothing itself.
#pragma once
#include "kzg_open_all_plan.hpp"

namespace kzg_cosets_plan {
namespace oa = kzg_open_all_plan;
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
using oa::FR_WORDS;
constexpr int COSETS_LOG_N_MAX = oa::OPEN_ALL_LOG_N_MAX;                   // the transform of 2c points must fit the 2^28 roots even at l = 1

constexpr bool logs_ok(int log_c, int log_l) { return log_c >= 0 && log_l >= 0 && log_c <= COSETS_LOG_N_MAX && log_l <= COSETS_LOG_N_MAX && log_c + log_l <= COSETS_LOG_N_MAX; }
constexpr int log_n(int log_c, int log_l) { return log_c + log_l; }
constexpr int wide_log(int log_c) { return oa::wide_log(log_c); }           // the convolutions run on 2c points
constexpr size_t wide(int log_c) { return oa::wide(log_c); }

// the caller's arrays, bytes, saturated: the table [l][8][2c] + [l][2c], the polynomials and y [m][4][n], the proofs [m][8][c] + [m][c]
constexpr size_t table_xy_bytes(int log_c, int log_l) { return g1_ntt_plan::xy_bytes(wide_log(log_c), elems(log_l)); }
constexpr size_t table_inf_bytes(int log_c, int log_l) { return g1_ntt_plan::inf_bytes(wide_log(log_c), elems(log_l)); }
constexpr size_t fr_bytes(int log_c, int log_l, size_t m) { return oa::fr_bytes(log_n(log_c, log_l), m); }
constexpr size_t pi_xy_bytes(int log_c, size_t m) { return oa::pi_xy_bytes(log_c, m); }

// ---- the table: T^(a) = the forward transform of x^(a), 2c points, x^(a)_(2c-1-u) = s_(a + l u) for u <= c - 2 and the identity elsewhere.
// Column k < 2c of array a < l holds the SRS point x_srs_index names, or X_IDENTITY; the points used are s_0 .. s_(n-l-1).
constexpr size_t X_IDENTITY = oa::X_IDENTITY;
constexpr size_t x_srs_index(size_t a, size_t k, int log_c, int log_l) {
  return oa::x_srs_index(k, log_c) == X_IDENTITY ? X_IDENTITY : a + (oa::x_srs_index(k, log_c) << log_l);
}
constexpr size_t prepare_items(int log_c, int log_l) { return mul_sat(wide(log_c), elems(log_l)); }
struct PrepareLayout { size_t xy, inf, bytes; };
constexpr PrepareLayout prepare_layout(int log_c, int log_l) {
  Carve c; PrepareLayout l{};
  l.xy = c.words(words_of(table_xy_bytes(log_c, log_l)));
  l.inf = c.bytes(table_inf_bytes(log_c, log_l));
  l.bytes = c.at; return l;
}
constexpr size_t prepare_scratch_bytes(int log_c, int log_l) { return prepare_layout(log_c, log_l).bytes; }
constexpr size_t prepare_grid(int log_c, int log_l) { return g1_ntt_plan::grid(prepare_items(log_c, log_l), -1); }

// ---- per polynomial.  log_c = 0 has one proof, the identity: one launch writes it.  From log_c = 1 on, with L = log_c + 1:
//   split    P^(a)_j = (2c)^-1 f_(a + l j) mod r for j < c, then c zeros: row A l + a of [m l][4][2c]; item i is (row i div 2c, column i mod 2c),
//            so consecutive lanes WRITE consecutive words and read f at a stride of l
//   Fr       F = the Fr transform of the m l rows (ntt.hip)
//   first    item (array A, plane p, butterfly j < c): over the residues a of the plane's slice, U = sum F^(a)_j T^(a)_j, then
//            V = sum F^(a)_(j+c) T^(a)_(j+c); out[2j] = U + V, out[2j + 1] = U - V at columns (p m + A) 2c + ... of a projective buffer of
//            planes m 2c columns -- the butterfly is linear, so the planes add
//   fold     column q < m 2c: the sum over the planes of column p m 2c + q, into buffer 0 (not launched at planes = 1, where `first` writes buffer 0)
//   then kzg_open_all_plan's steps with n -> c: the inverse stages 1 .. L - 1, the forward first stage that takes h_(c-1) as the identity,
//   the forward stages, the closing kernel.
constexpr bool trivial(int log_c) { return oa::trivial(log_c); }
constexpr size_t rows(int log_l, size_t m) { return mul_sat(elems(log_l), m); }                                    // Fr arrays of 2c points
constexpr size_t split_items(int log_c, int log_l, size_t m) { return mul_sat(rows(log_l, m), wide(log_c)); }
constexpr size_t split_row(size_t i, int log_c) { return i >> wide_log(log_c); }
constexpr size_t split_col(size_t i, int log_c) { return i & (wide(log_c) - 1); }
constexpr size_t split_poly(size_t row, int log_l) { return row >> log_l; }
constexpr size_t split_residue(size_t row, int log_l) { return row & (elems(log_l) - 1); }
constexpr bool split_is_zero(size_t col, int log_c) { return col >= elems(log_c); }
constexpr size_t split_src(size_t residue, size_t col, int log_l) { return residue + (col << log_l); }              // < n for col < c
constexpr size_t split_words(int log_c, int log_l, size_t m) { return mul_sat(split_items(log_c, log_l, m), FR_WORDS); }
constexpr size_t fr_row(size_t poly, size_t residue, int log_l) { return (poly << log_l) + residue; }

// the planes: 2^planes_log of them, plane p owns the residues [p l / planes, (p + 1) l / planes).  The default is the smallest count that
// brings the items c m planes up to the resident lanes of the grid cap (g1_ntt_plan.hpp), at most l, and 1 when c m alone fills them
constexpr bool planes_log_ok(int planes_log, int log_l) { return planes_log < 0 || planes_log <= log_l; }
constexpr size_t resident_lanes(long long max_blocks) { return g1_ntt_plan::grid_cap(max_blocks) * g1_ntt_plan::G1_NTT_BLOCK; }
constexpr int default_planes_log(int log_c, int log_l, size_t m, long long max_blocks) {
  int p = 0;
  while (p < log_l && mul_sat(mul_sat(elems(log_c), m), elems(p)) < resident_lanes(max_blocks)) ++p;
  return p;
}
constexpr int planes_log_of(int planes_log, int log_c, int log_l, size_t m, long long max_blocks) {
  return planes_log < 0 ? default_planes_log(log_c, log_l, m, max_blocks) : planes_log;
}
constexpr size_t slice_len(int log_l, int pl) { return elems(log_l - pl); }
constexpr size_t slice_begin(size_t p, int log_l, int pl) { return p << (log_l - pl); }
constexpr size_t plane_arrays(size_t m, int pl) { return mul_sat(m, elems(pl)); }                                  // (plane, polynomial) pairs
constexpr size_t first_items(int log_c, size_t m, int pl) { return mul_sat(plane_arrays(m, pl), elems(log_c)); }
constexpr size_t first_array(size_t b, int log_c) { return b >> log_c; }                                            // p m + A
constexpr size_t first_butterfly(size_t b, int log_c) { return b & (elems(log_c) - 1); }
constexpr size_t first_plane(size_t arr, size_t m) { return arr / m; }
constexpr size_t first_poly(size_t arr, size_t m) { return arr % m; }
constexpr size_t first_in0(size_t j) { return oa::first_in0(j); }
constexpr size_t first_in1(size_t j, int log_c) { return oa::first_in1(j, log_c); }
constexpr size_t first_out0(size_t arr, size_t j, int log_c) { return oa::first_out0(arr, j, log_c); }
constexpr size_t first_out1(size_t arr, size_t j, int log_c) { return oa::first_out1(arr, j, log_c); }
constexpr size_t stride(int log_c, size_t m) { return oa::stride(log_c, m); }                                      // of the two ping-pong buffers
constexpr size_t plane_stride(int log_c, size_t m, int pl) { return mul_sat(stride(log_c, m), elems(pl)); }
constexpr bool folds(int pl) { return pl > 0; }
constexpr size_t fold_items(int log_c, size_t m) { return stride(log_c, m); }
constexpr size_t fold_in(size_t q, size_t p, int log_c, size_t m) { return p * stride(log_c, m) + q; }
constexpr size_t plane_words(int log_c, size_t m, int pl) { return folds(pl) ? mul_sat(plane_stride(log_c, m, pl), G1_NTT_PROJ_WORDS) : 0; }
// scalar multiplications per polynomial: 2n products, then the stages of the inverse of 2c points and of the forward of c points
constexpr size_t multiplications(int log_c, int log_l) {
  return mul_sat(wide(log_c), elems(log_l)) + g1_ntt_plan::multiplications(wide_log(log_c)) + g1_ntt_plan::multiplications(log_c);
}

// ---- grids and window tables: the fused stage has the most multiplying items of the call, so its grid sizes the tables ----------------------
constexpr size_t first_grid(int log_c, size_t m, int pl, long long max_blocks) { return g1_ntt_plan::grid(first_items(log_c, m, pl), max_blocks); }
constexpr size_t fold_grid(int log_c, size_t m, long long max_blocks) { return g1_ntt_plan::grid(fold_items(log_c, m), max_blocks); }
constexpr size_t split_grid(int log_c, int log_l, size_t m) { return g1_ntt_plan::grid(split_items(log_c, log_l, m), -1); }
constexpr size_t table_bytes(int log_c, size_t m, int pl, long long max_blocks) {
  return first_grid(log_c, m, pl, max_blocks) * g1_ntt_plan::G1_NTT_BLOCK * g1_ntt_plan::G1_NTT_TABLE_BYTES_PER_LANE;
}

// ---- the scratch of a call, bytes, saturated: the window tables (16-byte loads: first), the twiddles of 2c and of c points, the two
// ping-pong buffers, the plane buffer, P and F -------------------------------------------------------------------------------------------------
struct ScratchLayout { size_t tables, tw_wide, tw, buf[2], planes, padded, f, bytes; };
constexpr ScratchLayout scratch_layout(int log_c, int log_l, size_t m, int pl, long long max_blocks) {
  Carve c; ScratchLayout l{};
  if (trivial(log_c)) return l;
  l.tables = c.bytes(table_bytes(log_c, m, pl, max_blocks));      // a multiple of 1 KB: the words after it stay aligned
  l.tw_wide = c.words(oa::wide_twiddle_words(log_c));
  l.tw = c.words(oa::twiddle_words(log_c));
  l.buf[0] = c.words(oa::buffer_words(log_c, m));
  l.buf[1] = c.words(oa::buffer_words(log_c, m));
  l.planes = c.words(plane_words(log_c, m, pl));
  l.padded = c.words(split_words(log_c, log_l, m));
  l.f = c.words(split_words(log_c, log_l, m));
  l.bytes = c.at; return l;
}
constexpr size_t scratch_bytes(int log_c, int log_l, size_t m, int pl, long long max_blocks) { return scratch_layout(log_c, log_l, m, pl, max_blocks).bytes; }
// its u64 words, behind the tables (none at c = 1, where nothing is leased)
constexpr size_t scratch_words(int log_c, int log_l, size_t m, int pl) {
  return scratch_layout(log_c, log_l, m, pl, -1).bytes == SAT ? SAT : (scratch_layout(log_c, log_l, m, pl, -1).bytes - scratch_layout(log_c, log_l, m, pl, -1).tw_wide) / 8;
}

// ---- the verifier's side: R_i = f mod (X^l - v^i) from the l values of coset i: the inverse Fr transform of l points, then
// r_k <- r_k g^k with g = w^(-i) = w^((n - i) mod n).  A row's l coefficients are walked by TWIST_LANES lanes (fewer for a shorter row): lane
// q takes k = q, q + lanes, ... with a running product from g^q in steps of g^lanes, so a row costs three short exponentiations per lane
// and no power per element.  idx >= c: the words are those of idx mod c, and in_range is 0.
constexpr int TWIST_LANES_LOG = 6;
constexpr int twist_lanes_log(int log_l) { return log_l < TWIST_LANES_LOG ? log_l : TWIST_LANES_LOG; }
constexpr size_t twist_items(int log_l, size_t n_rows) { return mul_sat(n_rows, elems(twist_lanes_log(log_l))); }
constexpr size_t twist_grid(int log_l, size_t n_rows) { return g1_ntt_plan::grid(twist_items(log_l, n_rows), -1); }
constexpr uint64_t coset_of(uint64_t idx, int log_c) { return idx & (((uint64_t)1 << log_c) - 1); }
constexpr bool in_range(uint64_t idx, int log_c) { return idx < ((uint64_t)1 << log_c); }
constexpr uint64_t twist_exp(uint64_t idx, int log_c, int log_l) {                                                // g = w^this
  return (((uint64_t)1 << log_n(log_c, log_l)) - coset_of(idx, log_c)) & (((uint64_t)1 << log_n(log_c, log_l)) - 1);
}
constexpr uint64_t z_exp(uint64_t idx, int log_c, int log_l) { return coset_of(idx, log_c) << log_l; }              // v^i = w^this
constexpr size_t vals_bytes(int log_l, size_t n_rows) { return mul_sat(mul_sat(elems(log_l), n_rows), FR_WORDS * sizeof(uint64_t)); }
// scratch of the reduction: R [rows][4][l], R(tau) G1gen as [8][rows] + [rows]; of the verifier: C - R(tau) G1gen likewise, z and y = 0
// [4][rows] each, in_range [rows]
constexpr size_t point_bytes(size_t n_rows) { return mul_sat(n_rows, G1_NTT_AFFINE_WORDS * sizeof(uint64_t)); }
constexpr size_t scalar_bytes(size_t n_rows) { return mul_sat(n_rows, FR_WORDS * sizeof(uint64_t)); }
struct ReduceLayout { size_t r, rc_xy, rc_inf, bytes; };
constexpr ReduceLayout reduce_layout(int log_l, size_t n_rows) {
  Carve c; ReduceLayout l{};
  l.r = c.words(words_of(vals_bytes(log_l, n_rows)));
  l.rc_xy = c.words(words_of(point_bytes(n_rows)));
  l.rc_inf = c.bytes(n_rows);
  l.bytes = c.at; return l;
}
constexpr size_t reduce_scratch_bytes(int log_l, size_t n_rows) { return reduce_layout(log_l, n_rows).bytes; }
struct VerifyLayout { size_t cred, z, y, cred_inf, in_rng, bytes; };
constexpr VerifyLayout verify_layout(size_t n_rows) {
  Carve c; VerifyLayout l{};
  l.cred = c.words(words_of(point_bytes(n_rows)));
  l.z = c.words(words_of(scalar_bytes(n_rows)));
  l.y = c.words(words_of(scalar_bytes(n_rows)));
  l.cred_inf = c.bytes(n_rows);
  l.in_rng = c.bytes(n_rows);
  l.bytes = c.at; return l;
}
constexpr size_t verify_scratch_bytes(size_t n_rows) { return verify_layout(n_rows).bytes; }
}  // namespace kzg_cosets_plan
