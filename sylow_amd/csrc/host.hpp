// host.hpp -- host-side plumbing shared by the translation units of libsylow_hip.so: error reporting, launch macros,
// the per-(device, stream) scratch workspace, the per-device G2-generator line tables, and the launchers each unit exports
// to the others.  Every unit compiles its own kernels (no relocatable device code): a kernel and the host function that
// launches it always live in the same .hip file.
#pragma once
#include "common.hpp"
#include "plan_base.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

extern thread_local char sylow_g_err[256];
namespace host {
int32_t fail(hipError_t e, const char* what);
// The aliasing check of an entry point: its inputs and outputs as two tables of Range, and outputs_disjoint(in, out, test) with the range test
// it wants -- plan_base::disjoint, or plan_base::disjoint_or_empty where an empty array may point anywhere.  The text is plan_base.hpp's, so
// that a host-only test can compile it.
using plan_base::Range;
using plan_base::outputs_disjoint;

// Scratch workspace (runtime.hip).  A Lease hands out one device block for the duration of ONE entry-point call: blocks are
// keyed per device, a block whose previous user ran on the same stream is reused in stream order, a block last used on another
// stream is reused only after that stream's completion event (the new stream waits on the event; no stored stream handle is
// ever dereferenced), and two host threads never hold the same block.  release() records the completion event.
struct Lease {
  void* p = nullptr;
  int dev = -1, slot = -1;
  hipStream_t st = nullptr;
  int32_t acquire(size_t bytes, hipStream_t stream);
  int32_t release();                 // records the block's completion event on the stream; idempotent
  template <class T> T* at(size_t off) const { return (T*)((char*)p + off); }     // the region at a byte offset of the unit's layout (plan_base::Carve)
  ~Lease() { release(); }
};
// The one way to end an entry point that holds leases and has launched kernels.  Reads the sticky launch error and releases every lease, in
// argument order, whatever the outcome; returns the first failure: an earlier `rc`, else the launch error, else the first failing release.
template <class... L> int32_t finish(int32_t rc, L&... leases) {
  const hipError_t e = hipGetLastError();
  if (rc == SYLOW_HIP_OK && e != hipSuccess) rc = fail(e, "kernel launch");
  for (const int32_t r : {leases.release()...}) if (rc == SYLOW_HIP_OK) rc = r;
  return rc;
}
// per-device line tables of the G2 generator (G2Affine::precompute of the constant, pairing.rs:676-708), built on first use
int32_t gen_lines29(const bn254::i32** out, hipStream_t st);    // carry-free lane-pair line table (plk_common.hpp: LINE_TABLE_WORDS)
int32_t g1_gen_comb(const bn254::i32** out, hipStream_t st);     // fixed-base table of the G1 generator (g1.hip), built on first use
int32_t g2_gen_comb(const bn254::i32** out, hipStream_t st);     // fixed-base table of the G2 generator (plk_group.hip), built on first use
void dst_arg(DstPrime& dp, const uint8_t* dst, size_t len);     // NULL -> sylow's DST (lib.rs:90)
size_t scratch_limit();                                         // sylow_hip_set_scratch_limit: 0 = default
unsigned compute_units();                                       // CUs of the calling thread's current device (0 if unknown)
long long option(int opt);                                      // sylow_hip_set_option: the value in force, -1 = the default (SYLOW_HIP_OPT_*)
inline long long option_or(int opt, long long dflt) { const long long v = option(opt); return v < 0 ? dflt : v; }
uint64_t* clock_probe();                                        // sylow_hip_clock_probe: the accumulator the metric's kernels add to, or NULL
// A short-lived side stream for work that may run BESIDE what the caller's stream holds next (the aggregate verifiers' signature half beside the
// hashing; the lane-quad tail of a batch beside its full rounds).  open(): the side stream waits for everything the caller's stream holds at this
// point; join(): the caller's stream waits for the side work.  Any failure to create the stream or its events degrades to the caller's stream
// (same results, no overlap), and so does enable = false.
struct Fork {
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t open(hipStream_t main, bool enable = true) {
    if (!enable) return main;
    if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) { side = nullptr; (void)hipGetLastError(); return main; }
    if (hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventRecord(ev_fork, main) != hipSuccess || hipStreamWaitEvent(side, ev_fork, 0) != hipSuccess) {
      (void)hipGetLastError();
      close();
      return main;
    }
    return side;
  }
  int32_t join(hipStream_t main) {
    if (!side) return SYLOW_HIP_OK;
    hipError_t e = hipEventRecord(ev_join, side);
    if (e == hipSuccess) e = hipStreamWaitEvent(main, ev_join, 0);
    if (e != hipSuccess) { (void)hipStreamSynchronize(side); return fail(e, "join of the side stream"); }
    return SYLOW_HIP_OK;
  }
  void close() {     // destroying a stream / an event with work in flight is deferred by the runtime until that work completes
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (side) (void)hipStreamDestroy(side);
    ev_fork = ev_join = nullptr; side = nullptr;
  }
  ~Fork() { close(); }
};
}  // namespace host

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return host::fail(e_, #x); } while (0)
#define ARGCHK(c) do { if (!(c)) { snprintf(sylow_g_err, sizeof(sylow_g_err), "bad argument: %s", #c); return SYLOW_HIP_E_ARG; } } while (0)
#define GRID(n) dim3((unsigned)(((n) + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream
#define LAUNCHED() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return host::fail(e_, "kernel launch"); return SYLOW_HIP_OK; } while (0)

// ---- launchers exported between units (argument lists as the C entry points of include/sylow_hip.h) ----------------------
namespace towerh {      // tower.hip: the one-element-per-lane Fp12 selector behind sylow_hip_fp12_hook_batch (ops 0..11)
int32_t fp12_hook(int32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
}  // namespace towerh
namespace g1h {         // g1.hip
size_t g1_comb_bytes();
int32_t build_g1_comb(bn254::i32* table, void* stream);
// hash.hip: H(m_i) (or -H(m_i)) affine, SoA stride n, with the library DST / a caller's DST
int32_t hash_to_g1(const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t* out_xy, uint8_t* out_inf, size_t n, int negate, void* stream);
int32_t hash_to_g1_proj(const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t* acc, size_t n, void* stream);   // projective, into sum_tree's array
// sign_wide.hip: sk_i * H(m_i) on eight lanes per signature (single calls and small batches)
int32_t sign_wide(const uint64_t* sk, const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t* sig_xy, uint8_t* sig_inf, size_t n, void* stream);
int32_t g1_scalar_mul_wide(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
size_t sign_wide_max();
int32_t evm_ecmul_wide(const uint8_t* in, uint8_t* out, uint8_t* status, size_t n, void* stream);
// sign_wide.hip: the same on eight lanes per message (small batches)
int32_t hash_to_g1_wide(const uint8_t* msgs, const uint64_t* msg_offsets, const DstPrime& dp, uint64_t* out_xy, uint8_t* out_inf, size_t n, int negate, void* stream);
int32_t hash_to_g1_dst(const uint8_t* msgs, const uint64_t* msg_offsets, const DstPrime& dp, uint64_t* out_xy, uint8_t* out_inf, size_t n, int negate, void* stream);
// expand.hip: the whole-call conditions of a caller-chosen expander (SYLOW_HIP_EXPANDER_*; E_ARG and the reason in sylow_hip_last_error), and
// H(m_i) (or -H(m_i)) affine under it with the caller's tag (dst NULL = the library tag); expander 0 is hash_to_g1_dst
int32_t expander_check(int32_t expander, int32_t security_bits, size_t len_in_bytes);
int32_t hash_to_g1_expander(int32_t expander, const uint8_t* dst, size_t dst_len, int32_t security_bits, const uint8_t* msgs, const uint64_t* msg_offsets,
                            uint64_t* out_xy, uint8_t* out_inf, size_t n, int negate, void* stream);
// sum_i P_i (or its negative) -> column `col` of an affine SoA array of stride `stride`; acc: scratch of 12 n words
int32_t sum(const uint64_t* p_xy, const uint8_t* p_inf, size_t n, uint64_t* acc, uint64_t* out_xy, uint8_t* out_inf, size_t stride, size_t col, int negate, void* stream);
// the same from an acc [12][n] that already holds the n projective points
int32_t sum_tree(uint64_t* acc, size_t n, uint64_t* out_xy, uint8_t* out_inf, size_t stride, size_t col, int negate, void* stream);
// the same for the first m elements of an acc whose SoA stride is acc_stride
int32_t sum_tree_strided(uint64_t* acc, size_t acc_stride, size_t m, uint64_t* out_xy, uint8_t* out_inf, size_t stride, size_t col, int negate, void* stream);
// n_seg independent sums of c points each, term-major (term k of segment s at index k * n_seg + s) -> affine SoA [8][n_seg] + flags;
// acc: scratch of sum_segments_scratch_words(n_seg, c) words (0 when one stage does it)
size_t sum_segments_scratch_words(size_t n_seg, size_t c);
int32_t sum_segments(const uint64_t* p_xy, const uint8_t* p_inf, size_t n_seg, size_t c, uint64_t* acc, uint64_t* out_xy, uint8_t* out_inf, void* stream);
}  // namespace g1h
namespace msmh {        // msm.hip: what sylow_hip_g1_msm(_tuned) does by default, for the units that plan around it
size_t g1_default_min();           // the smallest n that takes the bucket route (G1Lane::DEFAULT_MIN)
size_t default_budget();           // bytes of scratch a call may take when sylow_hip_set_scratch_limit is 0
bool window_ok(int32_t window);    // what the _tuned entry points accept: < 0 (the default) or a width they support
}  // namespace msmh
namespace kzgph {       // kzg_prove.hip: sylow_hip_kzg_commit_batch for coefficients known to be canonical (below r), past the mod-r pass; len > 0, m > 0
int32_t commit_canonical(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, uint64_t* out_xy, uint8_t* out_inf, void* stream);
}  // namespace kzgph
namespace ntth {        // ntt.hip: the twiddle table of the Fr transform, w_n^e for e < n / 2 as [4][n / 2] canonical words; log_n >= 1
int32_t build_table(int log_n, uint64_t* table, void* stream);
}  // namespace ntth
namespace g1ntth {      // g1_ntt.hip: ONE launch of its transform on a caller's projective buffers [12][stride], m arrays of 2^log_n points, array a at
// columns a 2^log_n: stage `stage` >= 1 (log_n >= 2; twiddles: ntth::build_table(log_n); tables: G1_TABLE_BYTES_PER_LANE bytes per lane of
// g1_ntt_plan::stage_grid(log_n, m, max_blocks) blocks), and the closing kernel without a scale: affine + flags into [m][8][n] + [m][n]
int32_t stage(const uint64_t* src, uint64_t* dst, int log_n, size_t m, size_t stride, int stage, bool inverse, const uint64_t* twiddles, uint8_t* tables,
              long long max_blocks, void* stream);
int32_t close(const uint64_t* src, int log_n, size_t m, size_t stride, uint64_t* out_xy, uint8_t* out_inf, long long max_blocks, void* stream);
}  // namespace g1ntth
namespace kzoah {       // kzg_open_all.hip: stage 0 of the forward transform of 2^log_n points (log_n >= 1) that reads h_b of array a at column a 2^(log_n+1) + b
// of src, takes h_(n-1) as the identity, and writes array a at columns a 2^log_n of dst; both buffers [12][stride] (kzg_open_all_plan.hpp: fwd_*)
int32_t fwd_first(const uint64_t* src, uint64_t* dst, int log_n, size_t m, size_t stride, long long max_blocks, void* stream);
}  // namespace kzoah
namespace kzgh {        // kzg.hip: F_i = C_i - y_i G1gen + z_i pi_i (affine SoA + flags, stride n) and, when neg_xy is given, -pi_i beside it: one launch
int32_t fold(const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z, const uint64_t* y, const uint64_t* pi_xy, const uint8_t* pi_inf,
             uint64_t* out_xy, uint8_t* out_inf, uint64_t* neg_xy, uint8_t* neg_inf, size_t n, void* stream);
}  // namespace kzgh
namespace plkh {        // lane-pair units
// selectors of plk_pairing.hip's Fp12 kernel (sylow_hip_fp12_hook_batch, and the Fp12 entry points of tower.hip)
enum { OPW_MUL = 16, OPW_SQR = 17, OPW_SPARSE = 18, OPW_CYCSQR = 19, OPW_FROB1 = 20, OPW_FROB2 = 21, OPW_FROB3 = 22, OPW_EXPZ = 23,
       OPW_S_MUL = 24, OPW_S_SQR = 25, OPW_S_INV = 26, OPW_S_CYCSQR = 27, OPW_CONJ = 28,
       OPW_SPARSE_UNIT = 29, OPW_DBL = 30, OPW_ADD = 31, OPW_LAST = 31 };   // 29: first line coefficient = (element index & 1), the other two from `b` as for 18
// 30 / 31: g2_doubling_step29 / g2_addition_step29 (ISO = false).  a: R = (X, Y, Z) in words 0..23, Q = (bx, by) in words 24..39 (31 only);
// b: P = (x, y) in words 0..7.  out: the stepped R in words 0..23, then the line as the Miller loop multiplies it in: l0, l1 y_P, l2 x_P.
// The same routines on the other layouts, at the same offset from their block's base: op = OPB_* + (OPW_* - OPW_MUL).  The one-wavefront
// blocks have no saturated routines; their offsets 8 and 10 are final_exponentiation29_wide and w12_inv_wide.
enum { OPB_QUAD = 32, OPB_WIDE1 = 48, OPB_WIDE2 = 64, OPB_END = 80, OPX_FINAL_EXP = 8, OPX_INV = 10 };
// the offsets each block serves: lane-pair 0..15, quad 0..7 and 13..15, wide 0..8, 10, 14, 15; and those that read `b`
constexpr unsigned OPX_QUAD_SET = 0xE0FFu, OPX_WIDE_SET = 0xC5FFu, OPX_NEEDS_B = 0xE005u;
// plk_pairing.hip: one Fp12 operation on the lane-pair layer (op = an OPW_* selector; OPW_SPARSE: b = 24 words)
int32_t fp12_op(int32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
int32_t build_lines29(const uint64_t* q_xy, size_t n, size_t idx, bn254::i32* table, void* stream);   // plk_verify.hip; q_xy NULL = generator
size_t line_table_bytes();                                                                             // plk_verify.hip
size_t g2_comb_bytes();                                                                                // plk_group.hip
int32_t build_g2_comb(bn254::i32* table, void* stream);                                                // plk_group.hip
// plk_group.hip: the G2 twin of g1h::sum_segments -- n_seg sums of c points each, term-major -> affine SoA [16][n_seg] + flags (the public keys
// of n_seg committees); acc: scratch of g2_sum_scratch_words(n_seg, c) words
size_t g2_sum_scratch_words(size_t n_seg, size_t c);
int32_t g2_sum(const uint64_t* q_xy, const uint8_t* q_inf, size_t n_seg, size_t c, uint64_t* acc, uint64_t* out_xy, uint8_t* out_inf, void* stream);
// plk_multi.hip: small batches on one wavefront per element, and the eight-lane routes of sign_wide.hip (small_routes_on: SYLOW_HIP_OPT_WIDE_TAIL != 0)
bool small_routes_on();
size_t wide_batch_max();           // 0 when the small-batch routes are off
size_t wide_verify_max();
int32_t miller_raw_wide_batch(const uint64_t* p_xy, const uint64_t* q_xy, uint64_t* f_out, size_t n, void* stream);
int32_t final_exp_wide_batch(const uint64_t* f, uint64_t* gt_out, size_t n, void* stream);
int32_t fp12_op_wide(int epw, int32_t off, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);   // test hook, ops OPB_WIDE1 / 2 + off
int32_t verify_two_pairings_wide_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* h, const uint8_t* h_inf, const uint64_t* sig_xy, const uint8_t* sig_inf,
                                       uint64_t* scratch, uint8_t* ok, size_t n, void* stream);
int32_t pairing_wide_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf, uint64_t* scratch, uint64_t* gt_out, size_t n, void* stream);
int32_t verify_wide_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* hneg, const uint8_t* hneg_inf, const uint64_t* sig_xy, const uint8_t* sig_inf,
                          uint64_t* scratch, uint8_t* ok, size_t n, void* stream, int one_key = 0);
// plk_quad.hip: mid-size batches on one lane QUAD per element (the lane-pair tower compiled with BN_QUAD 1); 0 from quad_batch_max = route off
size_t quad_batch_max();
size_t tail_split(size_t n);       // the remainder of a batch of whole rounds + a short tail that runs on quads beside the rounds, or 0
int32_t pairing_quad_range(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf, uint64_t* gt_out, size_t n, size_t m, void* stream);
int32_t miller_loop_quad_batch(const uint64_t* p_xy, const uint64_t* q_xy, uint64_t* f_out, size_t n, void* stream);
int32_t final_exp_quad_batch(const uint64_t* f, uint64_t* gt_out, size_t n, void* stream);
int32_t fp12_op_quad(int32_t off, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);   // test hook, ops OPB_QUAD + off
int32_t verify_fused_quad(int pk_is_table, const uint64_t* pk_xy, const uint8_t* pk_inf, const bn254::i32* pk_table, const uint64_t* hneg, const uint8_t* hneg_inf,
                          const uint64_t* sig_xy, const uint8_t* sig_inf, const bn254::i32* gen, uint8_t* ok, size_t n, size_t m, void* stream);
// plk_group.hip: EIP-197 pair decoding + validation into SoA arrays (one lane pair per 192-byte pair)
int32_t evm_decode_pairs(const uint8_t* in, size_t n_pairs, uint64_t* pxy, uint8_t* pinf, uint64_t* qxy, uint8_t* qinf, uint8_t* pst, void* stream);
}  // namespace plkh
