// kzg_recover_plan.hpp -- the geometry of the recovery of a KZG polynomial from any half of its cosets (kzg_recover.hip): n = c l points cut
// into c = 2^log_c cells of l = 2^log_l points, a polynomial of degree below n / 2, and per row a set M of at most c / 2 missing cells.
// The vanishing values, the staging of the missing roots, the element-wise kernels, the status reduction and the scratch with its offsets, plain C++ so
// that tests/cpp/kzg_recover_plan_test.cpp can compile it with g++ on a box without a GPU.  The launch code asks these functions and
// decides nothing itself.
#pragma once
#include "ntt_plan.hpp"

namespace kzg_recover_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::disjoint;
using plan_base::elems;
using plan_base::mul_sat;
using plan_base::words_of;
using ntt_plan::root_negated;
using ntt_plan::root_slot;
using ntt_plan::root_words;
constexpr int RECOVER_BLOCK = 256;                    // == BLOCK of common.hpp (kzg_recover.hip asserts it)
constexpr int RECOVER_WAVE = 64;
constexpr int RECOVER_WAVES = RECOVER_BLOCK / RECOVER_WAVE;
constexpr size_t FR_WORDS = 4;
// Z = prod_(i in M) (X^l - v^i) is a polynomial in X^l: c values on the domain, c on the coset, and each costs |M| <= c / 2 products --
// c^2 / 2 per row and array, quadratic in c.  2^12 cells keep that below the transforms of a row for every l >= 2^5 or so, and far below a
// second at the cap; a longer list of cells wants a product tree, which this unit does not have.
constexpr int RECOVER_LOG_C_MAX = 12;
constexpr int RECOVER_LOG_N_MAX = 27;
constexpr uint64_t RECOVER_COSET_SHIFT = 5;           // s: the generator the Groth16 quotient shifts by; s^(2^k) != 1 for k <= 28

constexpr int log_n(int log_c, int log_l) { return log_c + log_l; }
constexpr bool logs_ok(int log_c, int log_l) {
  return log_c >= 0 && log_l >= 0 && log_c <= RECOVER_LOG_C_MAX && log_l <= RECOVER_LOG_N_MAX && log_n(log_c, log_l) >= 1 &&
         log_n(log_c, log_l) <= RECOVER_LOG_N_MAX;
}
constexpr size_t max_missing(int log_c) { return elems(log_c) / 2; }                      // c / 2 rounded down: 0 at c = 1
constexpr size_t grid(size_t items) { return ntt_plan::grid(items); }
constexpr size_t blocks_of(size_t lanes) { return lanes / RECOVER_BLOCK + (lanes % RECOVER_BLOCK ? 1 : 0); }   // no sum that could wrap

// the caller's arrays, bytes, saturated: y, coeffs_out, y_out [m][4][n]; present [m][c]; zd_out, zc_out [m][4][c]; status_out [m]
constexpr size_t fr_bytes(int log_c, int log_l, size_t m) { return mul_sat(mul_sat(elems(log_n(log_c, log_l)), m), FR_WORDS * sizeof(uint64_t)); }
constexpr size_t present_bytes(int log_c, size_t m) { return mul_sat(elems(log_c), m); }
constexpr size_t z_bytes(int log_c, size_t m) { return mul_sat(mul_sat(elems(log_c), m), FR_WORDS * sizeof(uint64_t)); }
constexpr size_t status_bytes(size_t m) { return m; }

// ---- the constants of a call, [CONST_WORDS] u64: s as the transforms take their shift, then s^l = s^(2^log_l) (log_l squarings, one lane)
constexpr size_t CONST_SHIFT = 0, CONST_SL = 4, CONST_WORDS = 8;
// the roots v^e, e < c / 2, [4][c / 2]: the table of the transform of c points, root_words(log_c) of ntt_plan.hpp; none at c = 1

// ---- vanish: item (row, block of the row).  The row's mask is walked in rounds of VANISH_CHUNK indices: a round compacts the missing ones
// among them into an LDS list of at most VANISH_CHUNK roots (a ballot per wave, the waves' counts through LDS), then the lanes multiply their
// two chains by (a - x) over the list.  LDS does not grow with c.  A pass over the mask that only counts comes first: its count decides
// status 1 before a product is spent.  A value k is shared by 2^vanish_split_log adjacent lanes of a wave: lane `sub` takes the roots sub,
// sub + lanes, ... of every list and the partial products meet through log2(lanes) shuffles -- the chain of dependent products of a value
// is |M| / lanes + log2(lanes) long instead of |M|, and a row has `lanes` times as many blocks to spread over the device.  Below 2^5 cells
// the lists are too short to cut.  A row spans c / vanish_block_ks blocks, each staging the same lists.
constexpr size_t VANISH_CHUNK = RECOVER_BLOCK;
constexpr int VANISH_SPLIT_LOG = 4, VANISH_SPLIT_MIN_LOG_C = 5;
constexpr int vanish_split_log(int log_c) { return log_c >= VANISH_SPLIT_MIN_LOG_C ? VANISH_SPLIT_LOG : 0; }
constexpr size_t vanish_block_ks(int log_c) { return (size_t)RECOVER_BLOCK >> vanish_split_log(log_c); }       // values of k a block owns
constexpr size_t vanish_row_blocks(int log_c) { return (elems(log_c) + vanish_block_ks(log_c) - 1) / vanish_block_ks(log_c); }
constexpr size_t vanish_items(int log_c, size_t m) { return mul_sat(vanish_row_blocks(log_c), m); }
constexpr size_t vanish_row(size_t item, int log_c) { return item / vanish_row_blocks(log_c); }
constexpr size_t vanish_k0(size_t item, int log_c) { return (item % vanish_row_blocks(log_c)) * vanish_block_ks(log_c); }
constexpr size_t vanish_lane_k(size_t lane, int log_c) { return lane >> vanish_split_log(log_c); }             // + vanish_k0: the lane's k
constexpr size_t vanish_lane_sub(size_t lane, int log_c) { return lane & (((size_t)1 << vanish_split_log(log_c)) - 1); }
constexpr size_t vanish_rounds(int log_c) { return (elems(log_c) + VANISH_CHUNK - 1) / VANISH_CHUNK; }
constexpr size_t vanish_grid(int log_c, size_t m) { return grid(vanish_items(log_c, m)); }
constexpr size_t vanish_lds_bytes() { return VANISH_CHUNK * 8 * sizeof(uint32_t) + RECOVER_WAVES * sizeof(uint32_t); }
constexpr size_t vanish_products(int log_c, size_t missing) { return mul_sat(mul_sat(elems(log_c), missing), 2); }   // per row
// Where element (row, k) of zd / zc lies, in u64 words from the base, and the distance between its four words.  The caller's arrays are
// [m][4][c]; the call's own are ONE array [4][m c], the layout sylow_hip_fr_batch_inv takes, so that one call inverts every row's values.
constexpr size_t z_row_off(size_t row, int log_c, bool packed) { return packed ? row << log_c : (row * FR_WORDS) << log_c; }
constexpr size_t z_word_stride(int log_c, size_t m, bool packed) { return packed ? mul_sat(elems(log_c), m) : elems(log_c); }
constexpr size_t z_words(int log_c, size_t m) { return mul_sat(mul_sat(elems(log_c), m), FR_WORDS); }
constexpr size_t inv_elems(int log_c, size_t m) { return mul_sat(elems(log_c), m); }

// ---- mask-mul and div: an item per element of [m][4][n], consecutive lanes on consecutive words; the factor is read at k mod c
constexpr size_t elem_items(int log_c, int log_l, size_t m) { return mul_sat(elems(log_n(log_c, log_l)), m); }
constexpr size_t elem_row(size_t t, int log_c, int log_l) { return t >> log_n(log_c, log_l); }
constexpr size_t elem_col(size_t t, int log_c, int log_l) { return t & (elems(log_n(log_c, log_l)) - 1); }
constexpr size_t elem_cell(size_t col, int log_c) { return col & (elems(log_c) - 1); }
constexpr size_t elem_grid(int log_c, int log_l, size_t m) { return grid(blocks_of(elem_items(log_c, log_l, m))); }

// ---- status: item (row, chunk) over the upper half of a row, n / 2 elements from n / 2 on; a lane ORs the words of STATUS_LANE_ELEMS
// elements BLOCK apart, a wave reduces with a ballot, the block's first lane ORs into the row's flag word (u32, scratch); a small launch
// turns the flags into status 2 and leaves 0 and 1 alone
constexpr int STATUS_LANE_ELEMS = 8;
constexpr size_t STATUS_CHUNK = (size_t)RECOVER_BLOCK * STATUS_LANE_ELEMS;
constexpr size_t status_half(int log_c, int log_l) { return elems(log_n(log_c, log_l)) / 2; }
constexpr size_t status_row_chunks(int log_c, int log_l) { return (status_half(log_c, log_l) + STATUS_CHUNK - 1) / STATUS_CHUNK; }
constexpr size_t status_items(int log_c, int log_l, size_t m) { return mul_sat(status_row_chunks(log_c, log_l), m); }
constexpr size_t status_grid(int log_c, int log_l, size_t m) { return grid(status_items(log_c, log_l, m)); }
constexpr size_t status_close_grid(size_t m) { return grid(blocks_of(m)); }
constexpr size_t status_lds_bytes() { return RECOVER_WAVES * sizeof(uint32_t); }
constexpr size_t flag_words(size_t m) { return m / 2 + 1; }                               // u32 [m] in whole u64 words

// ---- the scratch of a call, u64 words then bytes, saturated.  vanish alone: the constants and the roots.  recover: those, zd, zc and
// zc^-1 packed, the flags, and ONE buffer [m][4][n] that the transforms ping-pong against coeffs_out (each transform leases its own table
// and buffer on top)
struct VanishLayout { size_t consts, roots, bytes; };
constexpr VanishLayout vanish_layout(int log_c, Carve c = {}) {      // c: the lease it is a part of (recover's), or its own
  VanishLayout l{};
  l.consts = c.words(CONST_WORDS);
  l.roots = c.words(root_words(log_c));
  l.bytes = c.at; return l;
}
constexpr size_t vanish_scratch_bytes(int log_c) { return vanish_layout(log_c).bytes; }
constexpr size_t vanish_scratch_words(int log_c) { return words_of(vanish_scratch_bytes(log_c)); }
constexpr size_t buffer_words(int log_c, int log_l, size_t m) { return mul_sat(elem_items(log_c, log_l, m), FR_WORDS); }
struct RecoverLayout {
  VanishLayout v;      // offsets in this lease; v.bytes is where it ends
  size_t zd, zc, zci, flags, buf, bytes;
};
constexpr RecoverLayout recover_layout(int log_c, int log_l, size_t m) {
  Carve c; RecoverLayout l{};
  l.v = vanish_layout(log_c, c);
  c.at = l.v.bytes;
  l.zd = c.words(z_words(log_c, m));
  l.zc = c.words(z_words(log_c, m));
  l.zci = c.words(z_words(log_c, m));
  l.flags = c.words(flag_words(m));
  l.buf = c.words(buffer_words(log_c, log_l, m));
  l.bytes = c.at; return l;
}
constexpr size_t recover_scratch_bytes(int log_c, int log_l, size_t m) { return recover_layout(log_c, log_l, m).bytes; }
constexpr size_t recover_scratch_words(int log_c, int log_l, size_t m) { return words_of(recover_scratch_bytes(log_c, log_l, m)); }
constexpr bool scratch_ok(size_t bytes) { return bytes <= SAT / 2; }
constexpr int transforms(bool with_y) { return with_y ? 4 : 3; }                       // sylow_hip_fr_ntt_batch calls: the floor of a call
}  // namespace kzg_recover_plan
