// fr_scan_plan.hpp -- the geometry of the scans over Fr under + and * and of PLONK's permutation grand product (fr_scan.hip): every size,
// grid, item, tile, scratch size and offset, and route decision between an entry point and its kernels, plain C++ so that tests/cpp/fr_scan_plan_test.cpp can
// compile it with g++ on a box without a GPU.  The launch code asks these functions and decides nothing itself.
#pragma once
#include "kzg_evals_plan.hpp"
#include "ntt_plan.hpp"
#include "plan_base.hpp"

namespace fr_scan_plan {
using plan_base::Carve;
using plan_base::SAT;
using plan_base::add_sat;
using plan_base::disjoint;
using plan_base::elems;
using plan_base::max_blocks_ok;
using plan_base::mul_sat;
// ---- the chunk is kzg_evals_plan.hpp's: a lane owns SCAN_LANE_ELEMS consecutive elements, a block of SCAN_BLOCK lanes a chunk of
// SCAN_CHUNK; the ratio scan shares the chunk's ONE inversion with sylow_hip_fr_batch_inv, so the two cannot differ ------------------------
constexpr int SCAN_BLOCK = 256;                  // == BLOCK of common.hpp (fr_scan.hip asserts it)
constexpr int SCAN_LANE_ELEMS = 8;               // L
constexpr size_t SCAN_CHUNK = 2048;              // CH = SCAN_BLOCK * SCAN_LANE_ELEMS
static_assert(SCAN_BLOCK == kzg_evals_plan::EVALS_BLOCK && SCAN_LANE_ELEMS == kzg_evals_plan::EVALS_LANE_ELEMS && SCAN_CHUNK == kzg_evals_plan::EVALS_CHUNK,
              "the chunk of the shared inversion");
constexpr size_t SCAN_GRID_CAP = (size_t)1 << 20;                       // blocks of one launch; more work than that is walked with a grid stride
constexpr int SCAN_TOTALS_TILE_MAX = 256;        // chunk totals the second level scans per step: a lane each, so at most a block of them
constexpr int SCAN_TOTALS_TILE_DEFAULT = 256;    // the whole block: a row of 2^28 elements is 2^17 totals, 512 steps of one block
constexpr int PLONK_WIRES_MAX = 32;              // columns of the permutation argument (SYLOW_HIP_PLONK_WIRES_MAX; fr_scan.hip asserts it)
constexpr int PLONK_LOG_N_MAX = 28;              // the domains of the transform
constexpr size_t FR_WORDS = 4;
static_assert(SCAN_TOTALS_TILE_MAX <= SCAN_BLOCK && SCAN_TOTALS_TILE_DEFAULT >= 1 && SCAN_TOTALS_TILE_DEFAULT <= SCAN_TOTALS_TILE_MAX, "a lane per total; the default is a legal pin");
static_assert(PLONK_WIRES_MAX <= SCAN_BLOCK && PLONK_LOG_N_MAX == ntt_plan::NTT_LOG_N_MAX, "a lane forms beta k_j per column; w is the transform's");
constexpr int OP_SUM = 0, OP_PRODUCT = 1;

constexpr bool op_ok(int op) { return op == OP_SUM || op == OP_PRODUCT; }
constexpr bool flag_ok(int flag) { return flag == 0 || flag == 1; }
// a pin: < 0 the default, 1 .. SCAN_TOTALS_TILE_MAX a tile
constexpr bool tile_ok(long long tile) { return tile < 0 || (tile >= 1 && tile <= SCAN_TOTALS_TILE_MAX); }
constexpr int tile_of(long long tile) { return tile < 0 ? SCAN_TOTALS_TILE_DEFAULT : (int)tile; }
constexpr bool plonk_ok(int log_n, int wires) { return log_n >= 0 && log_n <= PLONK_LOG_N_MAX && wires >= 1 && wires <= PLONK_WIRES_MAX; }
constexpr size_t grid(size_t items, long long max_blocks) {
  const size_t cap = max_blocks > 0 && (unsigned long long)max_blocks < SCAN_GRID_CAP ? (size_t)max_blocks : SCAN_GRID_CAP;
  return items < cap ? (items ? items : 1) : cap;
}

// ---- phase 1: the work items are (row, chunk), row-major; a block scans its chunk and leaves the chunk's total ---------------------------
constexpr size_t chunks(size_t len) { return kzg_evals_plan::chunks(len); }
constexpr size_t items(size_t len, size_t m) { return mul_sat(chunks(len), m); }
constexpr size_t item_row(size_t item, size_t n_chunks) { return item / n_chunks; }
constexpr size_t item_chunk(size_t item, size_t n_chunks) { return item % n_chunks; }
// the first element of lane t of chunk c
constexpr size_t lane_base(size_t c, int t) { return c * SCAN_CHUNK + (size_t)t * SCAN_LANE_ELEMS; }
// lanes of chunk c of a row of len elements that own an element: the block's scans run over these alone
constexpr int live_lanes(size_t len, size_t c) { return kzg_evals_plan::live_lanes(len, c); }
constexpr int scan_steps(int live) { return kzg_evals_plan::scan_steps(live); }
// A ROW OF ONE CHUNK NEEDS ONLY PHASE 1: its block writes the row's total (and the row's status) itself, and the call leases nothing
constexpr bool upper_phases(size_t len) { return chunks(len) > 1; }

// ---- phase 2: ONE block per row walks the row's chunk totals `tile` at a time, a lane per total, and carries the running value across the
// tiles in a register: no recursion, and no level that could run out below len = 2^28.  It leaves, in place, the prefix of every chunk ----
constexpr size_t tile_steps(size_t n_chunks, int tile) { return n_chunks / (size_t)tile + (n_chunks % (size_t)tile ? 1 : 0); }
constexpr size_t tile_first(size_t step, int tile) { return step * (size_t)tile; }
// totals of the step that starts at `first` < n_chunks: 1 .. tile
constexpr int tile_count(size_t n_chunks, size_t first, int tile) { return n_chunks - first < (size_t)tile ? (int)(n_chunks - first) : tile; }
constexpr size_t totals_grid(size_t m, long long max_blocks) { return grid(m, max_blocks); }

// ---- phase 3: the items are (row, chunk c >= 1): every element of the chunk is combined with the chunk's prefix, a lane SCAN_BLOCK apart
// from its neighbours' (the loads and stores of a wave are consecutive) ------------------------------------------------------------------
constexpr size_t apply_items(size_t len, size_t m) { return upper_phases(len) ? mul_sat(chunks(len) - 1, m) : 0; }
constexpr size_t apply_row(size_t item, size_t n_chunks) { return item / (n_chunks - 1); }
constexpr size_t apply_chunk(size_t item, size_t n_chunks) { return 1 + item % (n_chunks - 1); }
constexpr size_t apply_elem(size_t c, int i, int t) { return c * SCAN_CHUNK + (size_t)i * SCAN_BLOCK + (size_t)t; }

// ---- bytes of the caller's arrays, saturated ---------------------------------------------------------------------------------------------
constexpr size_t rows_bytes(size_t len, size_t m) { return mul_sat(mul_sat(mul_sat(len, FR_WORDS), m), sizeof(uint64_t)); }
constexpr size_t scalars_bytes(size_t count) { return mul_sat(mul_sat(count, FR_WORDS), sizeof(uint64_t)); }
constexpr bool scratch_ok(size_t bytes) { return bytes <= SAT / 2; }

// ---- the scratch of a scan, bytes, saturated: the chunk totals [4][items], which phase 2 turns into the chunk prefixes in place, and for
// the ratio scan a byte per item (a denominator of the chunk was 0), behind them.  Nothing for rows of one chunk -------------------------
constexpr size_t totals_words(size_t len, size_t m) { return upper_phases(len) ? mul_sat(FR_WORDS, items(len, m)) : 0; }
struct ScanLayout { size_t totals, zflag, bytes; };
constexpr ScanLayout scan_layout(size_t len, size_t m, bool ratio) {
  Carve c; ScanLayout l{};
  l.totals = c.words(totals_words(len, m));
  l.zflag = c.bytes(upper_phases(len) && ratio ? items(len, m) : 0);
  l.bytes = c.at; return l;
}
constexpr size_t scan_scratch_bytes(size_t len, size_t m, bool ratio) { return scan_layout(len, m, ratio).bytes; }

// ---- PLONK: the identity columns k_j w^i and the terms of the grand product.  w^i comes out of the transform's table of n / 2 roots
// (ntt_plan.hpp: root_words, root_slot, root_negated) by ONE load: no power is formed per element.  A lane owns ONE element of a row, so a
// wave's loads of every column are consecutive; the items of the terms kernel are (instance, tile of SCAN_BLOCK elements), those of the
// identity kernel tiles of the W n flattened (column, element) pairs ---------------------------------------------------------------------
constexpr size_t tiles_of(size_t lanes) { return lanes / SCAN_BLOCK + (lanes % SCAN_BLOCK ? 1 : 0); }
constexpr size_t root_words(int log_n) { return ntt_plan::root_words(log_n); }
constexpr size_t identity_items(int log_n, int wires) { return tiles_of(mul_sat(elems(log_n), (size_t)wires)); }
constexpr size_t identity_bytes(int log_n, int wires) { return rows_bytes(elems(log_n), (size_t)wires); }
constexpr size_t identity_scratch_bytes(int log_n) { return mul_sat(root_words(log_n), sizeof(uint64_t)); }
constexpr size_t terms_tiles(int log_n) { return tiles_of(elems(log_n)); }
constexpr size_t terms_items(int log_n, size_t m) { return mul_sat(terms_tiles(log_n), m); }
constexpr size_t wires_bytes(int log_n, int wires, size_t m) { return rows_bytes(elems(log_n), mul_sat((size_t)wires, m)); }
// u64 words of num or of den, [m][4][n]
constexpr size_t terms_words(int log_n, size_t m) { return mul_sat(mul_sat(FR_WORDS, elems(log_n)), m); }
// the permutation entry leases the roots, num and den; the ratio scan it ends in leases its own on top
struct PermutationLayout { size_t roots, num, den, bytes; };
constexpr PermutationLayout permutation_layout(int log_n, size_t m) {
  Carve c; PermutationLayout l{};
  l.roots = c.words(root_words(log_n));
  l.num = c.words(terms_words(log_n, m));
  l.den = c.words(terms_words(log_n, m));
  l.bytes = c.at; return l;
}
constexpr size_t permutation_scratch_bytes(int log_n, size_t m) { return permutation_layout(log_n, m).bytes; }
// STATUS of a row: bit 0 a denominator was 0 mod r; bit 1 (the permutation entry alone) the product did not close to 1
constexpr int STATUS_ZERO_DEN = 1, STATUS_NOT_CLOSED = 2;
}  // namespace fr_scan_plan
