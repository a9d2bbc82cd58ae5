// plonk_open.hip -- PLONK's closing rounds (include/sylow_popen.h):
//   sylow_popen_prepare           the coefficient table of a circuit: its selectors and sigma as coefficients, [2 W + 2][4][n];
//   sylow_popen_evaluate_batch    the 2 W + 1 evaluations of m instances at zeta (z at zeta w_n), the sigma rows read in place;
//   sylow_popen_linearise_batch   r and F of m instances: the scalars and weights on the device, then ONE fused linear combination;
//   sylow_popen_open_batch        the route to (evaluations, W_zeta, W_omega) per chunk of whole instances under the scratch limit.
// The fused kernel keeps a lane per coefficient column and streams over the rows -- the shared rows of the table, z, the chunks of t, the
// wires -- with two unreduced accumulators, r's and what F adds.  Nothing of size W lives in registers.  Slots, rows, items, chunks and
// scratch: plonk_open_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_block.hpp"
#include "bn254_fr_acc.hpp"
#include "bn254_fr_roots.hpp"
#include "kzg_scan_dev.hpp"
#include "plonk_open_plan.hpp"
#include "../../include/sylow_popen.h"

namespace po {
using namespace plonk_open_plan;
static_assert(PO_BLOCK == BLOCK && PO_EVAL_CHUNK == (size_t)kzg_scan::CH, "a tile per block of BLOCK lanes; the chunks of the Horner scan");
static_assert(SYLOW_HIP_PLONK_WIRES_MAX == PO_WIRES_MAX && PO_WEIGHT_ROUND <= BLOCK, "the header's bound is the plan's; a lane per staged weight");

// element k of an Fr SoA array of stride n, mod r, the reduction out of line as in plonk_quotient.hip
BN_NOINLINE Fp canon(Fp a) { return fr_reduce_plain(a); }
BN_DEV Fp at(const u64* a, size_t n, size_t k) { return canon(load_plain(a, n, k, 0)); }
// entry i of an array [.][4] of canonical values (the weights of an instance)
BN_DEV Fp slot(const u64* a, size_t i) { return load_plain(a + i * FR_WORDS, 1, 0, 0); }
BN_DEV void slot_put(u64* a, size_t i, const Fp& v) { store_plain(a + i * FR_WORDS, 1, 0, 0, v); }
struct Wide {
  u32 v[16];
};
// the one Barrett reduction of the fused kernel, out of line: its constants stay out of the kernel's scalar registers
BN_NOINLINE Fp fold(Wide a) { return fr_reduce_wide(a.v); }
// acc += a b, unreduced; the PO_FLUSH products before it are folded first.  THE BOUND (bn254_fr_acc.hpp): both factors are canonical and a
// fold leaves a residue below r, so the accumulator stays below r + 16 r^2 < 2^512.
BN_DEV void acc_add(Wide& acc, int& pending, const Fp& a, const Fp& b) {
  if (pending == PO_FLUSH) {
    const Fp f = fold(acc);
#pragma unroll
    for (int k = 0; k < 16; ++k) acc.v[k] = k < 8 ? f.v[k] : 0;
    pending = 0;
  }
  mul_acc(acc.v, a, b);
  ++pending;
}

// The two points of instance s0 + s, s < mc, a lane each, canonical: pts [2][4][mc], zeta and zeta w_n; w_n is the 2^28-th root squared down,
// as the transform's table forms it
__global__ void __launch_bounds__(BLOCK) k_po_points(const u64* zeta, size_t m, size_t s0, size_t mc, int log_n, u64* pts) {
#pragma unroll 1
  for (size_t s = TID; s < mc; s += (size_t)gridDim.x * BLOCK) {
    const Fp x = elem(zeta, m, s0 + s);
    Fp w = fp_from_limbs(BN_FR_ROOT28);
#pragma unroll 1
    for (int i = 0; i < ntt_plan::root_squarings(log_n); ++i) w = fr_mul(w, w);
    store_plain(pts, mc, s, 0, x);
    store_plain(pts + FR_WORDS * mc, mc, s, 0, fr_mul(x, w));
  }
}

// The rows of ONE instance in one launch of k_po_eval, in this order: nw rows of len_w coefficients at wires [.][nw][4][len_w]; ns rows of
// n coefficients at sigma [ns][4][n], SHARED by every instance; has_z: one row at z [.][4][len_z], evaluated at the second point; pi_slot:
// one row at pi [.][4][n], or the value 0 when pi is NULL.  wires, z and pi point at the launch's first instance.
struct Rows {
  const u64 *wires, *sigma, *z, *pi;
  size_t len_w, len_z, n;
  int nw, ns, has_z, pi_slot;
};
static size_t row_count(const Rows& r) { return (size_t)(r.nw + r.ns + r.has_z + r.pi_slot); }

// Item (instance s, row c, chunk q): the chunk's value at its own base, sum_{i < CH} f_{q CH + i} x^i, into partials [4][n_items] at the item.
// A lane runs Horner over its L consecutive coefficients and the block folds the lane values with x^(L 2^s) (kzg_scan_dev.hpp).  The chunks
// are those of the launch's longest row: an item past the end of its own row stores 0.  The grid is walked with a stride of whole blocks:
// every lane of a block sees the same item, so the barriers are reached by whole blocks.  No read leaves a row: lane_value guards every
// coefficient by len, and s < mc, c < rows by the item count.
__global__ void __launch_bounds__(BLOCK) k_po_eval(Rows r, const u64* pts, size_t mc, size_t rows, size_t chunks, size_t n_items, u64* partials) {
  __shared__ u32 pw[kzg_scan::LOG_BLOCK][8], part[BLOCK][8];
#pragma unroll 1
  for (size_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const size_t s = eval_item_instance(it, rows, chunks), c = eval_item_row(it, rows, chunks), q = eval_item_chunk(it, chunks);
    const u64* f;
    size_t len, pt = 0;
    if (c < (size_t)r.nw) { f = r.wires + (s * (size_t)r.nw + c) * FR_WORDS * r.len_w; len = r.len_w; }
    else if (c < (size_t)(r.nw + r.ns)) { f = r.sigma + (c - (size_t)r.nw) * FR_WORDS * r.n; len = r.n; }
    else if (r.has_z && c == (size_t)(r.nw + r.ns)) { f = r.z + s * FR_WORDS * r.len_z; len = r.len_z; pt = 1; }
    else { f = r.pi ? r.pi + s * FR_WORDS * r.n : nullptr; len = r.pi ? r.n : 0; }
    if (!eval_chunk_live(len, q)) {                           // block-uniform, and before any barrier of this item
      if (threadIdx.x == 0) store_plain(partials, n_items, it, 0, fr_zero());
      continue;
    }
    const Fp x = load_plain(pts + pt * FR_WORDS * mc, mc, s, 0);
    kzg_scan::block_powers<kzg_scan::LOG_L>(x, pw);
    const Fp v = kzg_scan::lane_value(f, len, q * PO_EVAL_CHUNK + (size_t)threadIdx.x * kzg_scan::L, x);
    const Fp sum = kzg_scan::block_suffix<false>(v, pw, part, kzg_scan::live_lanes(len, q));     // its first barrier publishes pw, its last one frees part and pw
    if (threadIdx.x == 0) store_plain(partials, n_items, it, 0, sum);
  }
}
// A block per (instance s, row c): sum_q partial_q (x^CH)^q into out [4][out_stride] at out_first + s rows + c.  Lane t folds the partials of
// its `seg` consecutive chunks by Horner with x^CH, and the block folds the lane values with powers of x^(CH seg), as k_po_eval folds its
// lanes: a row of 2^20 coefficients is 512 chunks, two a lane, not 512 dependent products on one.  One chunk: the partial is the value.
// z_row: the row evaluated at the second point, or -1.
__global__ void __launch_bounds__(BLOCK) k_po_eval_fold(const u64* partials, const u64* pts, size_t mc, size_t rows, int z_row, size_t chunks, size_t seg,
                                                        size_t n_items, u64* out, size_t out_stride, size_t out_first) {
  __shared__ u32 pw[kzg_scan::LOG_BLOCK][8], part[BLOCK][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t f = blockIdx.x; f < mc * rows; f += gridDim.x) {
    if (chunks == 1) {                                        // block-uniform, and before any barrier of this row
      if (t == 0) store_plain(out, out_stride, out_first + f, 0, load_plain(partials, n_items, f, 0));
      continue;
    }
    const size_t s = f / rows, c = f - s * rows, q0 = (size_t)t * seg;
    Fp xc = load_plain(pts + (z_row >= 0 && c == (size_t)z_row ? FR_WORDS * mc : 0), mc, s, 0);
#pragma unroll 1
    for (int i = 0; i < kzg_scan::LOG_L + kzg_scan::LOG_BLOCK; ++i) xc = fr_mul(xc, xc);
    kzg_scan::block_powers<0>(fr_pow(xc, (u64)seg), pw);
    Fp v = fr_zero();
#pragma unroll 1
    for (size_t i = seg; i-- > 0;)
      if (q0 + i < chunks) v = fr_add(fr_mul(v, xc), load_plain(partials, n_items, f * chunks + q0 + i, 0));
    const Fp sum = kzg_scan::block_suffix<false>(v, pw, part, (int)eval_fold_lanes(chunks));     // its first barrier publishes pw, its last one frees part and pw
    if (t == 0) store_plain(out, out_stride, out_first + f, 0, sum);
  }
}

// The weight vector of instance s0 + s, s < mc, a block each: weights [mc][slots][4] (plonk_open_plan.hpp: one weight per row of the fold, then
// the constant term of r and ZH), canonical.  Lane 0 brings the challenges and the evaluations to canonical form and forms zeta^n by log_n
// squarings, ZH, L1 (WITHOUT an inversion, see below), A, B and the five scalars the weights are made of; then a lane per slot: a
// power of v, or -ZH zeta^(e n), by square-and-multiply, so that the lanes stay independent.  v may be NULL: the rows only F takes weigh 0.
enum { SC_ZN, SC_NEG_ZH, SC_ZH, SC_V, SC_WZ, SC_WSIGMA, SC_CONST, SC_A01, SC_COUNT };
__global__ void __launch_bounds__(BLOCK) k_po_consts(const u64* evals, const u64* shifts, const u64* beta, const u64* gamma, const u64* alpha, const u64* zeta,
                                                     const u64* v, size_t m, size_t s0, size_t mc, int log_n, int log_e, int W, u64* weights) {
  __shared__ u32 sc[SC_COUNT][8];
  const int t = threadIdx.x;
  const size_t ev_n = evals_count(W, m), NW = weight_slots(log_e, W);
#pragma unroll 1
  for (size_t s = blockIdx.x; s < mc; s += gridDim.x) {
    const size_t g = s0 + s, e0 = g * eval_slots(W);
    __syncthreads();                                         // the instance before has read sc
    if (t == 0) {
      const Fp x = elem(zeta, m, g), b = elem(beta, m, g), gm = elem(gamma, m, g), al = elem(alpha, m, g);
      // no inversion: (zeta^n - 1) / (zeta - 1) = 1 + zeta + .. + zeta^(n-1) is the product of 1 + zeta^(2^i) over the squarings that form zeta^n,
      // and inv(n) is log_n halvings of 1 mod r; zeta = 1 is the one point where the header's inv(0) = 0 shows: L1 = 0 there
      Fp zn = x, geo = fr_one(), ninv = fr_one();
#pragma unroll 1
      for (int i = 0; i < log_n; ++i) {
        geo = fr_mul(geo, fr_add(fr_one(), zn));
        zn = fr_mul(zn, zn);
        fr_euclid::half_mod(ninv.v);
      }
      const Fp zh = fr_sub(zn, fr_one());
      const Fp l1 = fp_eq(x, fr_one()) ? fr_zero() : fr_mul(geo, ninv);
      const Fp bx = fr_mul(b, x);
      Fp A = fr_one(), B = fr_one(), a01 = fr_one(), last = fr_zero();
#pragma unroll 1
      for (int j = 0; j < W; ++j) {
        const Fp aj = elem(evals, ev_n, e0 + slot_wire(j)), ag = fr_add(aj, gm);
        A = fr_mul(A, fr_add(ag, fr_mul(bx, elem(shifts, (size_t)W, (size_t)j))));
        if (j + 1 < W) B = fr_mul(B, fr_add(ag, fr_mul(b, elem(evals, ev_n, e0 + slot_sigma(W, j)))));
        else last = ag;
        if (j < 2) a01 = j ? fr_mul(a01, aj) : aj;
      }
      const Fp al2l1 = fr_mul(fr_mul(al, al), l1), abz = fr_mul(fr_mul(al, B), elem(evals, ev_n, e0 + slot_zw(W)));
      lds_put(sc, SC_ZN, zn);
      lds_put(sc, SC_NEG_ZH, fr_neg(zh));
      lds_put(sc, SC_ZH, zh);
      lds_put(sc, SC_V, v ? elem(v, m, g) : fr_zero());
      lds_put(sc, SC_WZ, fr_add(fr_mul(al, A), al2l1));
      lds_put(sc, SC_WSIGMA, fr_neg(fr_mul(abz, b)));
      lds_put(sc, SC_CONST, fr_sub(fr_sub(elem(evals, ev_n, e0 + slot_pi(W)), fr_mul(abz, last)), al2l1));
      lds_put(sc, SC_A01, a01);
    }
    __syncthreads();
#pragma unroll 1
    for (size_t i = (size_t)t; i < NW; i += BLOCK) {
      Fp w;
      if (i < (size_t)W) w = elem(evals, ev_n, e0 + slot_wire((int)i));
      else if (i == row_qm(W)) w = lds_get(sc, SC_A01);
      else if (i == row_qc(W)) w = fr_one();
      else if (i < row_sigma(W, W - 1)) w = v ? fr_pow(lds_get(sc, SC_V), (u64)W + 1 + (i - row_sigma(W, 0))) : fr_zero();
      else if (i == row_sigma(W, W - 1)) w = lds_get(sc, SC_WSIGMA);
      else if (i == wrow_z(W)) w = lds_get(sc, SC_WZ);
      else if (i < wrow_chunk(W, 0)) w = v ? fr_pow(lds_get(sc, SC_V), 1 + (i - wrow_wire(W, 0))) : fr_zero();
      else if (i < wslot_const(log_e, W)) w = fr_mul(lds_get(sc, SC_NEG_ZH), fr_pow(lds_get(sc, SC_ZN), i - wrow_chunk(W, 0)));
      else w = lds_get(sc, i == wslot_const(log_e, W) ? SC_CONST : SC_ZH);
      slot_put(weights, s * NW + i, w);
    }
  }
}

// what one launch of the fused kernel reads and writes; wires, z, t and the outputs point at the launch's first instance
struct Fold {
  const u64 *ctable, *wires, *z, *t, *weights;        // [2 W + 2][4][n], [.][W][4][len_w], [.][4][len_z], [.][4][N], [.][slots][4]
  size_t len_w, len_z, r_len, f_len;
  u64 *r_dst, *f_dst, *z_dst;                         // [.][4][r_len], [.][4][f_len], [.][4][f_len]; each may be NULL
  int log_n, log_e, W;
};
// Item (instance s, tile of BLOCK columns), a lane per column k:
//   r_k = sum over the rows of r of weight_row row[k],  plus the constant term at k = 0;   F_k = r_k + sum over the rows only F takes
// The rows go by in rounds of PO_WEIGHT_ROUND: that many lanes stage the round's weights in LDS (ONE fetch per block and row; every lane
// then reads the same LDS word), and each lane adds weight x row[k] into the accumulator of the row's kind, unreduced, for the rows that
// reach its column: a row of the table has n coefficients, z len_z, a wire len_w, and chunk e of t is t[e n + k] for k < n.  Without f_dst
// the rows only F takes are stepped over.  z_dst takes z mod r, zero from len_z on.  Every lane of a block sees the same instance and the
// same rows, so the barriers are reached by whole blocks.  Every index is size_t; a load is guarded by k < the row's length and a store by
// k < the output's row length, and s < the instances of the launch by the item count.
__global__ void __launch_bounds__(BLOCK) k_po_fold(Fold a, size_t n_tiles, size_t n_items) {
  __shared__ u32 wl[PO_WEIGHT_ROUND][8];
  const int t = threadIdx.x;
#pragma unroll 1
  for (size_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    // the sizes are derived per item from scalars the compiler must take as new here: hoisted out of this loop, the values derived from
    // them (row offsets, counts) would each hold scalar registers across the row loop, more than there are (plonk_quotient.hip does the same)
    int log_n = a.log_n, log_e = a.log_e, W = a.W;
    asm volatile("" : "+s"(log_n), "+s"(log_e), "+s"(W));
    const size_t n = elems(log_n), N = elems(log_big(log_n, log_e)), NR = fold_rows(log_e, W), NW = weight_slots(log_e, W);
    const size_t s = item_instance(it, n_tiles), k = column(it, n_tiles, t);
    const bool want_f = a.f_dst != nullptr;
    Wide ar, af;
#pragma unroll
    for (int i = 0; i < 16; ++i) ar.v[i] = af.v[i] = 0;
    int pr = 0, pf = 0;
#pragma unroll 1
    for (size_t base = 0; base < NR; base += PO_WEIGHT_ROUND) {
      const int cnt = NR - base < (size_t)PO_WEIGHT_ROUND ? (int)(NR - base) : PO_WEIGHT_ROUND;
      __syncthreads();                                       // the round before has read its weights
      if (t < cnt) lds_put(wl, t, slot(a.weights, s * NW + base + (size_t)t));
      __syncthreads();
#pragma unroll 1
      for (int i = 0; i < cnt; ++i) {
        const size_t row = base + (size_t)i;
        const bool extra = row_is_extra(W, row);
        if (extra && !want_f) continue;
        const u64* p;
        size_t len, stride, idx = k;
        if (row < ctable_rows(W)) { p = a.ctable + row * FR_WORDS * n; len = stride = n; }
        else if (row == wrow_z(W)) { p = a.z + s * FR_WORDS * a.len_z; len = stride = a.len_z; }
        else if (row < wrow_chunk(W, 0)) { p = a.wires + (s * (size_t)W + (row - wrow_wire(W, 0))) * FR_WORDS * a.len_w; len = stride = a.len_w; }
        else { p = a.t + s * FR_WORDS * N; len = n; stride = N; idx = (row - wrow_chunk(W, 0)) * n + k; }
        if (k >= len) continue;
        const Fp x = at(p, stride, idx);
        if (extra) acc_add(af, pf, x, lds_get(wl, i));
        else acc_add(ar, pr, x, lds_get(wl, i));
      }
    }
    Fp r = fold(ar);
    if (k == 0) r = fr_add(r, slot(a.weights, s * NW + wslot_const(log_e, W)));
    if (a.r_dst && k < a.r_len) store_plain(a.r_dst + s * FR_WORDS * a.r_len, a.r_len, k, 0, r);
    if (want_f && k < a.f_len) store_plain(a.f_dst + s * FR_WORDS * a.f_len, a.f_len, k, 0, fr_add(r, fold(af)));
    if (a.z_dst && k < a.f_len) store_plain(a.z_dst + s * FR_WORDS * a.f_len, a.f_len, k, 0, k < a.len_z ? at(a.z + s * FR_WORDS * a.len_z, a.len_z, k) : fr_zero());
  }
}

// status[s0 + s] for s < mc, a lane each.  Bit 0 from r(zeta): rz [4][mc] holds it, or, when yf [4][mc] = F(zeta) is given, it is
// F(zeta) - sum_j v^(1+j) a_j - sum_j v^(W+1+j) s_j with the powers of v as the weights hold them.  Bit 1 from ZH = 0.
__global__ void __launch_bounds__(BLOCK) k_po_status(const u64* rz, const u64* yf, const u64* evals, const u64* weights, size_t m, size_t s0, size_t mc, int log_e,
                                                     int W, uint8_t* status) {
  const size_t ev_n = evals_count(W, m), NW = weight_slots(log_e, W);
#pragma unroll 1
  for (size_t s = TID; s < mc; s += (size_t)gridDim.x * BLOCK) {
    Fp r = load_plain(yf ? yf : rz, mc, s, 0);
    if (yf) {
      const size_t e0 = (s0 + s) * eval_slots(W);
#pragma unroll 1
      for (int j = 0; j < W; ++j) {
        r = fr_sub(r, fr_mul(slot(weights, s * NW + wrow_wire(W, j)), elem(evals, ev_n, e0 + slot_wire(j))));
        if (j + 1 < W) r = fr_sub(r, fr_mul(slot(weights, s * NW + row_sigma(W, j)), elem(evals, ev_n, e0 + slot_sigma(W, j))));
      }
    }
    status[s0 + s] = (uint8_t)((fp_is_zero(r) ? 0 : STATUS_R_NOT_ZERO) | (fp_is_zero(slot(weights, s * NW + wslot_zh(log_e, W))) ? STATUS_ZETA_IN_DOMAIN : 0));
  }
}
// the proofs of a chunk, [8][mc] + flags each, to columns s0 .. s0 + mc - 1 of the caller's [8][m] + flags
__global__ void __launch_bounds__(BLOCK) k_po_scatter(const u64* p1, const uint8_t* f1, const u64* p2, const uint8_t* f2, size_t m, size_t s0, size_t mc, u64* o1,
                                                      uint8_t* of1, u64* o2, uint8_t* of2) {
#pragma unroll 1
  for (size_t s = TID; s < mc; s += (size_t)gridDim.x * BLOCK) {
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      o1[(size_t)w * m + s0 + s] = p1[(size_t)w * mc + s];
      o2[(size_t)w * m + s0 + s] = p2[(size_t)w * mc + s];
    }
    of1[s0 + s] = f1[s];
    of2[s0 + s] = f2[s];
  }
}

static unsigned lane_grid(size_t lanes, long long max_blocks) { return (unsigned)grid(lane_tiles(lanes), max_blocks); }
// the rows of mc instances at their points pts, through `partials`, into out [4][out_stride] from out_first on, instance-major
static void eval_launch(const Rows& r, const u64* pts, size_t mc, size_t longest, long long max_blocks, u64* partials, u64* out, size_t out_stride, size_t out_first,
                        hipStream_t st) {
  const size_t rows = row_count(r), chunks = eval_chunks(longest), its = eval_items(rows, longest, mc);
  k_po_eval<<<dim3((unsigned)grid(its, max_blocks)), dim3(BLOCK), 0, st>>>(r, pts, mc, rows, chunks, its, partials);
  k_po_eval_fold<<<dim3((unsigned)grid(mc * rows, max_blocks)), dim3(BLOCK), 0, st>>>(partials, pts, mc, rows, r.has_z ? r.nw + r.ns : -1, chunks,
                                                                                       eval_fold_segment(chunks), its, out, out_stride, out_first);
}
static void fold_launch(const Fold& f, size_t mc, long long max_blocks, hipStream_t st) {
  const size_t longest = max2(f.r_dst ? f.r_len : 0, f.f_dst || f.z_dst ? f.f_len : 0), n_tiles = tiles(longest), its = items(longest, mc);
  k_po_fold<<<dim3((unsigned)grid(its, max_blocks)), dim3(BLOCK), 0, st>>>(f, n_tiles, its);
}

struct Job {
  const u64 *srs, *ctable, *wires, *z, *pi, *t, *shifts, *beta, *gamma, *alpha, *zeta, *v;
  size_t len_w, len_z, len_f, m, mc;                  // mc: the instances of a full chunk, which fixes the layout of the lease
  int log_n, log_e, W;
  u64 *evals_out, *w_zeta_xy, *w_omega_xy;
  uint8_t *w_zeta_inf, *w_omega_inf, *status;
};
// instances s0 .. s0 + c - 1 through the lease ws (open_layout): every part sized for a full chunk
static int32_t chunk(const Job& j, size_t s0, size_t c, const host::Lease& ws, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = elems(j.log_n), N = elems(log_big(j.log_n, j.log_e)), longest = longest_row(j.log_n, j.len_w, j.len_z);
  const OpenLayout l = open_layout(j.log_n, j.log_e, j.W, j.len_w, j.len_z, j.len_f, j.mc);
  u64 *pts = ws.at<u64>(l.ev.pts), *partials = ws.at<u64>(l.ev.partials), *weights = ws.at<u64>(l.weights), *F = ws.at<u64>(l.F), *Z = ws.at<u64>(l.Z),
      *yf = ws.at<u64>(l.yf), *yz = ws.at<u64>(l.yz), *p1 = ws.at<u64>(l.p1), *p2 = ws.at<u64>(l.p2);
  uint8_t *f1 = ws.at<uint8_t>(l.f1), *f2 = ws.at<uint8_t>(l.f2);
  const u64 *wires = j.wires + s0 * (size_t)j.W * FR_WORDS * j.len_w, *z = j.z + s0 * FR_WORDS * j.len_z;
  k_po_points<<<dim3(lane_grid(c, -1)), dim3(BLOCK), 0, st>>>(j.zeta, j.m, s0, c, j.log_n, pts);
  const Rows rows = {wires, j.ctable + row_sigma(j.W, 0) * FR_WORDS * n, z, j.pi ? j.pi + s0 * FR_WORDS * n : nullptr, j.len_w, j.len_z, n, j.W, j.W - 1, 1, 1};
  eval_launch(rows, pts, c, longest, -1, partials, j.evals_out, evals_count(j.W, j.m), s0 * eval_slots(j.W), st);
  k_po_consts<<<dim3((unsigned)grid(c, -1)), dim3(BLOCK), 0, st>>>(j.evals_out, j.shifts, j.beta, j.gamma, j.alpha, j.zeta, j.v, j.m, s0, c, j.log_n, j.log_e, j.W, weights);
  const Fold f = {j.ctable, wires, z, j.t + s0 * FR_WORDS * N, weights, j.len_w, j.len_z, 0, j.len_f, nullptr, F, Z, j.log_n, j.log_e, j.W};
  fold_launch(f, c, -1, st);
  int32_t rc = sylow_hip_kzg_open_batch(j.srs, F, j.len_f, c, pts, yf, p1, f1, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_kzg_open_batch(j.srs, Z, j.len_f, c, pts + FR_WORDS * c, yz, p2, f2, stream);
  if (rc != SYLOW_HIP_OK) return rc;
  k_po_status<<<dim3(lane_grid(c, -1)), dim3(BLOCK), 0, st>>>(nullptr, yf, j.evals_out, weights, j.m, s0, c, j.log_e, j.W, j.status);
  k_po_scatter<<<dim3(lane_grid(c, -1)), dim3(BLOCK), 0, st>>>(p1, f1, p2, f2, j.m, s0, c, j.w_zeta_xy, j.w_zeta_inf, j.w_omega_xy, j.w_omega_inf);
  return SYLOW_HIP_OK;
}
}  // namespace po

extern "C" {
int32_t sylow_popen_prepare(const uint64_t* selectors, const uint64_t* sigma, int32_t log_n, int32_t W, uint64_t* ctable, void* stream) {
  using namespace plonk_open_plan;
  ARGCHK(dims_ok(log_n, 0, W));
  ARGCHK(selectors && sigma && ctable);
  const host::Range in[2] = {{(uintptr_t)selectors, selectors_bytes(log_n, W)}, {(uintptr_t)sigma, sigma_bytes(log_n, W)}};
  const host::Range outs[1] = {{(uintptr_t)ctable, ctable_bytes(log_n, W)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  int32_t rc = sylow_hip_fr_ntt_batch(selectors, log_n, (size_t)W + 2, /*inverse=*/1, nullptr, ctable, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_fr_ntt_batch(sigma, log_n, (size_t)W, /*inverse=*/1, nullptr, ctable + row_sigma(W, 0) * FR_WORDS * elems(log_n), stream);
  return rc;
}

int32_t sylow_popen_evaluate_batch_tuned(const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* pi,
                                         const uint64_t* zeta, int32_t log_n, int32_t W, size_t m, int64_t max_blocks, uint64_t* evals_out, void* stream) {
  using namespace plonk_open_plan;
  ARGCHK(dims_ok(log_n, 0, W) && max_blocks_ok(max_blocks) && lens_ok(PO_LOG_MAX, len_w, len_z));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(ctable && wires && z && zeta && evals_out);
  const size_t n = elems(log_n), scratch = evaluate_scratch_words(log_n, W, len_w, len_z, m);
  ARGCHK(coeff_bytes(len_w, mul_sat((size_t)W, m)) != SAT && coeff_bytes(len_z, m) != SAT && coeff_bytes(n, m) != SAT && evals_bytes(W, m) != SAT && scratch_ok(scratch));
  const host::Range in[5] = {{(uintptr_t)ctable, ctable_bytes(log_n, W)}, {(uintptr_t)wires, coeff_bytes(len_w, (size_t)W * m)}, {(uintptr_t)z, coeff_bytes(len_z, m)},
                             {(uintptr_t)pi, coeff_bytes(n, m)}, {(uintptr_t)zeta, scalars_bytes(m)}};
  const host::Range outs[1] = {{(uintptr_t)evals_out, evals_bytes(W, m)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  const EvaluateLayout l = evaluate_layout(log_n, W, len_w, len_z, m);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *pts = ws.at<u64>(l.pts), *partials = ws.at<u64>(l.partials);
  po::k_po_points<<<dim3(po::lane_grid(m, max_blocks)), dim3(BLOCK), 0, st>>>(zeta, m, 0, m, log_n, pts);
  const po::Rows rows = {wires, ctable + row_sigma(W, 0) * FR_WORDS * n, z, pi, len_w, len_z, n, W, W - 1, 1, 1};
  po::eval_launch(rows, pts, m, longest_row(log_n, len_w, len_z), max_blocks, partials, evals_out, evals_count(W, m), 0, st);
  return host::finish(rc, ws);
}
int32_t sylow_popen_evaluate_batch(const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* pi,
                                   const uint64_t* zeta, int32_t log_n, int32_t W, size_t m, uint64_t* evals_out, void* stream) {
  return sylow_popen_evaluate_batch_tuned(ctable, wires, len_w, z, len_z, pi, zeta, log_n, W, m, -1, evals_out, stream);
}

int32_t sylow_popen_linearise_batch_tuned(const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* t,
                                          const uint64_t* evals, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha,
                                          const uint64_t* zeta, const uint64_t* v, int32_t log_n, int32_t log_e, int32_t W, size_t m, size_t len_out,
                                          int64_t max_blocks, uint64_t* r_out, uint64_t* f_out, uint8_t* status, void* stream) {
  using namespace plonk_open_plan;
  ARGCHK(dims_ok(log_n, log_e, W) && max_blocks_ok(max_blocks) && lens_ok(log_big(log_n, log_e), len_w, len_z));
  ARGCHK(len_out_ok(log_n, len_w, len_z, len_out, false));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(ctable && z && t && evals && shifts && beta && gamma && alpha && zeta && status && (r_out || f_out) && (!f_out || (wires && v)));
  ARGCHK(len_out_ok(log_n, len_w, len_z, len_out, f_out != nullptr));
  const bool own_r = r_out == nullptr;
  const size_t N = elems(log_big(log_n, log_e)), scratch = linearise_scratch_words(log_n, log_e, W, len_z, len_out, m, own_r);
  ARGCHK(coeff_bytes(len_w, mul_sat((size_t)W, m)) != SAT && coeff_bytes(N, m) != SAT && coeff_bytes(len_out, m) != SAT && evals_bytes(W, m) != SAT && scratch_ok(scratch));
  const host::Range in[11] = {{(uintptr_t)ctable, ctable_bytes(log_n, W)}, {(uintptr_t)wires, coeff_bytes(len_w, (size_t)W * m)}, {(uintptr_t)z, coeff_bytes(len_z, m)},
                              {(uintptr_t)t, coeff_bytes(N, m)}, {(uintptr_t)evals, evals_bytes(W, m)}, {(uintptr_t)shifts, scalars_bytes((size_t)W)},
                              {(uintptr_t)beta, scalars_bytes(m)}, {(uintptr_t)gamma, scalars_bytes(m)}, {(uintptr_t)alpha, scalars_bytes(m)},
                              {(uintptr_t)zeta, scalars_bytes(m)}, {(uintptr_t)v, scalars_bytes(m)}};
  const host::Range outs[3] = {{(uintptr_t)r_out, coeff_bytes(len_out, m)}, {(uintptr_t)f_out, coeff_bytes(len_out, m)}, {(uintptr_t)status, m}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  const LineariseLayout l = linearise_layout(log_n, log_e, W, len_z, len_out, m, own_r);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  const size_t r_len = own_r ? len_r(log_n, len_z) : len_out;
  u64 *pts = ws.at<u64>(l.pts), *weights = ws.at<u64>(l.weights), *rz = ws.at<u64>(l.rz), *partials = ws.at<u64>(l.partials),
      *r_buf = own_r ? ws.at<u64>(l.r_buf) : r_out;
  po::k_po_points<<<dim3(po::lane_grid(m, max_blocks)), dim3(BLOCK), 0, st>>>(zeta, m, 0, m, log_n, pts);
  po::k_po_consts<<<dim3((unsigned)grid(m, max_blocks)), dim3(BLOCK), 0, st>>>(evals, shifts, beta, gamma, alpha, zeta, f_out ? v : nullptr, m, 0, m, log_n, log_e, W, weights);
  const po::Fold f = {ctable, wires, z, t, weights, len_w, len_z, r_len, len_out, r_buf, f_out, nullptr, log_n, log_e, W};
  po::fold_launch(f, m, max_blocks, st);
  const po::Rows rows = {r_buf, nullptr, nullptr, nullptr, r_len, 0, 0, 1, 0, 0, 0};                  // r(zeta) from r's coefficients
  po::eval_launch(rows, pts, m, r_len, max_blocks, partials, rz, m, 0, st);
  po::k_po_status<<<dim3(po::lane_grid(m, max_blocks)), dim3(BLOCK), 0, st>>>(rz, nullptr, nullptr, weights, m, 0, m, log_e, W, status);
  return host::finish(rc, ws);
}
int32_t sylow_popen_linearise_batch(const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* t,
                                    const uint64_t* evals, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha,
                                    const uint64_t* zeta, const uint64_t* v, int32_t log_n, int32_t log_e, int32_t W, size_t m, size_t len_out,
                                    uint64_t* r_out, uint64_t* f_out, uint8_t* status, void* stream) {
  return sylow_popen_linearise_batch_tuned(ctable, wires, len_w, z, len_z, t, evals, shifts, beta, gamma, alpha, zeta, v, log_n, log_e, W, m, len_out, -1, r_out,
                                           f_out, status, stream);
}

int32_t sylow_popen_open_batch(const uint64_t* srs_g1_xy, const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z,
                               const uint64_t* pi, const uint64_t* t, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma,
                               const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, int32_t log_n, int32_t log_e, int32_t W, size_t m,
                               size_t len_f, uint64_t* evals_out, uint64_t* w_zeta_xy, uint8_t* w_zeta_inf, uint64_t* w_omega_xy, uint8_t* w_omega_inf,
                               uint8_t* status, void* stream) {
  using namespace plonk_open_plan;
  ARGCHK(dims_ok(log_n, log_e, W) && lens_ok(log_big(log_n, log_e), len_w, len_z));
  ARGCHK(len_out_ok(log_n, len_w, len_z, len_f, true));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(srs_g1_xy && ctable && wires && z && t && shifts && beta && gamma && alpha && zeta && v);
  ARGCHK(evals_out && w_zeta_xy && w_zeta_inf && w_omega_xy && w_omega_inf && status);
  const size_t n = elems(log_n), N = elems(log_big(log_n, log_e));
  ARGCHK(coeff_bytes(len_w, mul_sat((size_t)W, m)) != SAT && coeff_bytes(N, m) != SAT && mul_sat(len_f, 8 * sizeof(uint64_t)) != SAT && evals_bytes(W, m) != SAT &&
         mul_sat(m, 8 * sizeof(uint64_t)) != SAT && open_budget_bytes(log_n, log_e, W, len_w, len_z, len_f, 1) != SAT);
  const host::Range in[12] = {{(uintptr_t)srs_g1_xy, len_f * 8 * sizeof(uint64_t)}, {(uintptr_t)ctable, ctable_bytes(log_n, W)},
                              {(uintptr_t)wires, coeff_bytes(len_w, (size_t)W * m)}, {(uintptr_t)z, coeff_bytes(len_z, m)}, {(uintptr_t)pi, coeff_bytes(n, m)},
                              {(uintptr_t)t, coeff_bytes(N, m)}, {(uintptr_t)shifts, scalars_bytes((size_t)W)}, {(uintptr_t)beta, scalars_bytes(m)},
                              {(uintptr_t)gamma, scalars_bytes(m)}, {(uintptr_t)alpha, scalars_bytes(m)}, {(uintptr_t)zeta, scalars_bytes(m)},
                              {(uintptr_t)v, scalars_bytes(m)}};
  const host::Range outs[6] = {{(uintptr_t)evals_out, evals_bytes(W, m)}, {(uintptr_t)w_zeta_xy, m * 8 * sizeof(uint64_t)}, {(uintptr_t)w_zeta_inf, m},
                               {(uintptr_t)w_omega_xy, m * 8 * sizeof(uint64_t)}, {(uintptr_t)w_omega_inf, m}, {(uintptr_t)status, m}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const size_t lim = host::scratch_limit(), mc = instances_per_chunk(log_n, log_e, W, len_w, len_z, len_f, m, lim ? lim : msmh::default_budget());
  if (!mc) {
    snprintf(sylow_g_err, sizeof(sylow_g_err), "plonk_open: the scratch limit does not hold one instance (%zu bytes)",
             open_budget_bytes(log_n, log_e, W, len_w, len_z, len_f, 1));
    return SYLOW_HIP_E_HIP;
  }
  const hipStream_t st = (hipStream_t)stream;
  host::Lease ws;
  int32_t rc = ws.acquire(open_chunk_bytes(log_n, log_e, W, len_w, len_z, len_f, mc), st);
  if (rc != SYLOW_HIP_OK) return rc;
  const po::Job job = {srs_g1_xy, ctable, wires, z, pi, t, shifts, beta, gamma, alpha, zeta, v, len_w, len_z, len_f, m, mc, log_n, log_e, W,
                       evals_out, w_zeta_xy, w_omega_xy, w_zeta_inf, w_omega_inf, status};
  for (size_t s0 = 0; s0 < m && rc == SYLOW_HIP_OK; s0 += mc) rc = po::chunk(job, s0, chunk_size(m, mc, s0), ws, stream);
  return host::finish(rc, ws);
}
}  // extern "C"
