// plk_common.hpp -- helpers shared by the LANE-PAIR kernel units (bn254_pair.hpp, bn254_pair29.hpp).
// Thread t handles coordinate pair_role(t) of element pair_index(t) (bn254_pair.hpp), so a launch covers 2 n threads and a wavefront carries 32 elements.
// Both lanes of a pair always take the same branches.
#pragma once
#include "host.hpp"
#include "bn254_pair29.hpp"

#include <atomic>

namespace plk {
using namespace bn254;
using namespace bn254::pl;

// element geometry of the unit: one lane pair per element (32 per wavefront), or -- BN_QUAD 1, plk_quad.hip -- one lane quad (16 per wavefront),
// whose two lane pairs compute the same values: sub-pair 0 stores
#if BN_QUAD
BN_DEV size_t elem_index(size_t t) { return quad_index(t); }
BN_DEV bool elem_writer(size_t t) { return quad_sub(t) == 0; }
constexpr int ELEMS_PER_BLOCK = BLOCK / 4;
#else
BN_DEV size_t elem_index(size_t t) { return pair_index(t); }
BN_DEV bool elem_writer(size_t) { return true; }
constexpr int ELEMS_PER_BLOCK = BLOCK / 2;
#endif
BN_DEV S2 load_s2(const u64* base, size_t n, size_t i, int w0, int odd) { return S2{load_fp(base, n, i, w0 + 4 * odd)}; }
BN_DEV void store_s2(u64* base, size_t n, size_t i, int w0, int odd, const S2& a) { store_fp(base, n, i, w0 + 4 * odd, a.c); }
BN_DEV void load_s12(S12& r, const u64* base, size_t n, size_t i, int odd) {
  r.c0.c0 = load_s2(base, n, i, 0, odd); r.c0.c1 = load_s2(base, n, i, 8, odd); r.c0.c2 = load_s2(base, n, i, 16, odd);
  r.c1.c0 = load_s2(base, n, i, 24, odd); r.c1.c1 = load_s2(base, n, i, 32, odd); r.c1.c2 = load_s2(base, n, i, 40, odd);
}
BN_DEV void store_s12(u64* base, size_t n, size_t i, int odd, const S12& a) {
  store_s2(base, n, i, 0, odd, a.c0.c0); store_s2(base, n, i, 8, odd, a.c0.c1); store_s2(base, n, i, 16, odd, a.c0.c2);
  store_s2(base, n, i, 24, odd, a.c1.c0); store_s2(base, n, i, 32, odd, a.c1.c1); store_s2(base, n, i, 40, odd, a.c1.c2);
}
// ---- test hook (sylow_hip_fp12_hook_batch) shared by the lane-pair and the lane-quad unit: one routine of the carry-free tower on element i,
// off = op - the block's base (host.hpp OPW_* - OPW_MUL).  `b` holds the second operand, the three line coefficients (ell_0, ell_vw, ell_vv:
// 24 words) for the sparse products, or P for the Miller steps.  Compiled with BN_QUAD 1 the routines reach the leaf-pair forms: the
// product, square, sparse products and Frobenius maps W2_MUL2; the cyclotomic square and exp_by_neg_z W2_MUL2 through w_fp4_square_fold
// and the product; the doubling step W2_MUL_SQR, W2_SQR2, W2_SQR_MUL and W2_MUL2; the addition step W2_MUL2 and W2_SQR2; the line
// scaling after either step W2_SCALE2.
BN_DEV void w12_hook_op(int off, S12& sr, const S12& sx, const u64* b, size_t n, size_t i, int odd) {
  using namespace plkh;
  constexpr int MUL = OPW_MUL;
  W12 x, y, r;
  w12_from_s12(x, sx);
  if (off == OPW_DBL - MUL || off == OPW_ADD - MUL) {            // Miller steps (ISO = false): R in x.c0, Q in x.c1.c0 / c1.c1, P in b
    const F29 px = f29_reduce(f29_from_fp(load_fp(b, n, i, 0))), py = f29_reduce(f29_from_fp(load_fp(b, n, i, 4)));
    G2W q{x.c0.c0, x.c0.c1, x.c0.c2};
    W2 l0, l1, l2, s1, s2;
    if (off == OPW_ADD - MUL) g2_addition_step29(q, x.c1.c0, x.c1.c1, l0, l1, l2);
    else g2_doubling_step29<false>(q, l0, l1, l2);
    W2_SCALE2(s1, s2, l1, py, l2, px);                             // the Miller loop's line_mul: l1 y_P, l2 x_P
    r.c0 = W6{q.x, q.y, q.z};
    r.c1 = W6{l0, s1, s2};
  } else {
    if (b) {
      S12 sy;
      if (off == OPW_SPARSE - MUL || off == OPW_SPARSE_UNIT - MUL) {   // three line coefficients: 24 words, whatever the width of the array behind them
        sy.c0.c0 = load_s2(b, n, i, 0, odd); sy.c0.c1 = load_s2(b, n, i, 8, odd); sy.c0.c2 = load_s2(b, n, i, 16, odd);
        sy.c1 = sy.c0;
      } else {
        load_s12(sy, b, n, i, odd);
      }
      w12_from_s12(y, sy);
    }
    switch (off) {
      case OPW_MUL - MUL: w12_mul_nl(r, x, y); break;
      case OPW_SQR - MUL: r = w12_sqr(x); break;
      case OPW_SPARSE - MUL: r = w12_sparse_mul(x, y.c0.c0, y.c0.c1, y.c0.c2); break;
      case OPW_CYCSQR - MUL: w12_cyclotomic_sqr_nl(r, x); break;
      case OPW_FROB1 - MUL: w12_frobenius_nl<1>(r, x); break;
      case OPW_FROB2 - MUL: w12_frobenius_nl<2>(r, x); break;
      case OPW_FROB3 - MUL: w12_frobenius_nl<3>(r, x); break;
      case OPW_CONJ - MUL: r = w12_conj(x); break;
      case OPW_SPARSE_UNIT - MUL: r = w12_sparse_mul_unit(x, (i32)(i & 1), y.c0.c1, y.c0.c2); break;
      default: exp_by_neg_z29(r, x); break;
    }
  }
  w12_to_s12(sr, r);
}
// ---- staggered launches (plk_pairing.hip: k_pairing; plk_verify.hip: k_bls_verify_fused) -------------------------------------------------
// Blocks [first, first + count) run only the first half of their element's work (the Miller loop) and park the value; blocks >= nblk finish
// the parked chunks (b - nblk + first).  See k_pairing for why.
struct Stagger {
  unsigned first, count, nblk;
  unsigned mute;                    // test mode (SYLOW_HIP_OPT_STAGGER = 2): parking blocks never publish, so every finishing block takes the recompute fallback
  u64* park;                        // [48][count * BLOCK / 2] raw Miller values
  unsigned* done;                   // [count] set by a parking block when its values are visible
  u64* clk;                         // sylow_hip_clock_probe: [64][4] accumulators, or NULL (the default)
};
// Live clock probe (include/sylow_hip.h: sylow_hip_clock_probe).  Every wavefront reads the shader-clock counter and the constant-rate counter
// when it starts and when it ends; lane 0 adds the two deltas, a wavefront count and the longest residency into slot blockIdx % 64.  Four scalar
// registers across the kernel and four fire-and-forget atomics per wavefront (32 768 wavefronts per 2^20 pairings): not measurable in the kernel's
// time (same-box A/B: profiles/r06_ab/r05_vs_r06.log).
struct ClockProbe { u64 c0, w0; };
BN_DEV void probe_begin(ClockProbe& pb, const u64* clk) {
  if (clk) { pb.c0 = __builtin_amdgcn_s_memtime(); pb.w0 = __builtin_amdgcn_s_memrealtime(); }
}
BN_DEV void probe_end(const ClockProbe& pb, u64* clk) {
  if (!clk) return;
  const u64 dc = __builtin_amdgcn_s_memtime() - pb.c0, dw = __builtin_amdgcn_s_memrealtime() - pb.w0;
  if ((threadIdx.x & 63) == 0) {
    u64* a = clk + 4 * (blockIdx.x & 63);
    __hip_atomic_fetch_add(a + 0, dc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(a + 1, dw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(a + 2, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(a + 3, dw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// role of this block -- 0: whole element, 1: Miller loop only (park), 2: final exponentiation only -- and the chunk of elements it works on
BN_DEV int stagger_role(const Stagger& st, unsigned& chunk) {
  chunk = blockIdx.x;
  if (st.count) {
    if (chunk >= st.first && chunk < st.first + st.count) return 1;
    if (chunk >= st.nblk) { chunk = chunk - st.nblk + st.first; return 2; }
  }
  return 0;
}
BN_DEV void stagger_publish(const Stagger& st, unsigned chunk) {       // role 1, after the block's stores to st.park
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0 && !st.mute) __hip_atomic_store(&st.done[chunk - st.first], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// role 2, before the block's loads from st.park: true when the parked values are visible.  The parking block was dispatched long before this
// one (in-order dispatch; it has normally finished whole rounds ago), so the flag is set on the first look; the wait is BOUNDED (~2 ms) all the
// same, and on false the caller recomputes the chunk from its inputs (role 0 on the same elements) -- no schedule of the dispatcher, no other
// grid sharing the GPU can turn the skew into a deadlock.
BN_DEV bool stagger_wait(const Stagger& st, unsigned chunk) {
  __shared__ int ready;
  if (threadIdx.x == 0) {
    int r = 0;
#pragma unroll 1
    for (int it = 0; it < 4096 && !r; ++it) {
      r = __hip_atomic_load(&st.done[chunk - st.first], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0u;
      if (!r) __builtin_amdgcn_s_sleep(16);
    }
    ready = r;
  }
  __syncthreads();
  // every wavefront reads st.park next: the acquire above was thread 0's; the barrier orders the workgroup but is no agent-scope acquire for
  // the other wavefronts' vector loads in the memory model (one L1 per CU makes it hold in practice) -- one fence per wavefront makes it formal
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return ready != 0;
}

BN_DEV S2 s2_g2gen_x() { return S2{sel(lane_odd(), fp_const(C_G2_GEN[0]), fp_const(C_G2_GEN[1]))}; }
BN_DEV S2 s2_g2gen_y() { return S2{sel(lane_odd(), fp_const(C_G2_GEN[2]), fp_const(C_G2_GEN[3]))}; }
BN_DEV W2 w2_select(const W2& a, const W2& b, bool c) { return W2{sel9(c, a.c, b.c)}; }     // c ? b : a


// Line table of one G2 point (G2Affine::precompute, pairing.rs:676-708) for the verification kernels, which only need the pairing
// up to factors the final exponentiation removes: every line (l0, l1, l2) is stored divided by l0 -- any Fp2 factor dies in the
// easy part -- as (l1 / l0, l2 / l0) plus a unit word (1; 0 for a line whose l0 is zero, stored undivided), so the accumulator
// update is a 10-product multiplication by (unit + x2 v^2 + x4 v w) instead of the 13-product mul_by_024.
// Layout: [87][2 coefficients][2 coordinates][9 limbs] int32 R-class digits, then [87] unit words.
constexpr int LINE_TABLE_LINES = 87;
constexpr int LINE_TABLE_WORDS = LINE_TABLE_LINES * 36 + LINE_TABLE_LINES;
}  // namespace plk

namespace plkh {
// plk_pairing.hip: fills `sg` for a staggered launch of `nblk` blocks, `full` of them whole chunks (count = 0: plain launch)
// `resident` = blocks of the kernel one CU holds (blocks_per_cu of the caller's kernel)
hipError_t stagger_setup(plk::Stagger& sg, host::Lease& ws, size_t nblk, size_t full, hipStream_t st, int resident);
// Blocks of kernel K one CU holds, cached per kernel and per device; 2 (what the kernels are built for) if the query fails
template <auto K> int blocks_per_cu() {
  auto query = [] {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, K, BLOCK, 0) != hipSuccess || b < 1) { (void)hipGetLastError(); b = 2; }
    return b;
  };
  static std::atomic<int> cache[64];          // 0: not asked yet
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) { (void)hipGetLastError(); return query(); }
  int v = cache[d].load(std::memory_order_relaxed);
  if (!v) cache[d].store(v = query(), std::memory_order_relaxed);
  return v;
}
// Whole rounds staggered on lane pairs + the remainder (tail_split) on quads beside them, for a batch of n elements on stream `st`.
//   launch_main(m, blocks, sg): the lane-pair kernel (`resident` = its blocks_per_cu) on the first m elements, `blocks` blocks, on st
//   launch_tail(m, tail, side): the quad route on elements [m, m + tail) on stream `side`; returns its status
// The side stream forks behind everything st holds on entry; the park block is released right behind the main kernel (the tail does not read it).
template <class Main, class Tail>
int32_t launch_rounds_and_tail(size_t n, hipStream_t st, int resident, Main&& launch_main, Tail&& launch_tail) {
  const size_t tail = tail_split(n), m = n - tail;
  host::Fork fk;
  hipStream_t side = tail ? fk.open(st) : st;
  // staggered launch (see k_pairing): needs one full resident set of blocks made of whole chunks
  const size_t nblk = (2 * m + BLOCK - 1) / BLOCK, full = (2 * m) / BLOCK;
  plk::Stagger sg;
  host::Lease park;
  const hipError_t es = stagger_setup(sg, park, nblk, full, st, resident);
  if (es != hipSuccess) return host::fail(es, "stagger flags");
  launch_main(m, (unsigned)(nblk + sg.count), sg);
  int32_t rc = host::finish(SYLOW_HIP_OK, park);
  if (tail && rc == SYLOW_HIP_OK) {
    rc = launch_tail(m, tail, side);
    const int32_t joined = fk.join(st);
    if (rc == SYLOW_HIP_OK) rc = joined;
  }
  return rc;
}
}  // namespace plkh
