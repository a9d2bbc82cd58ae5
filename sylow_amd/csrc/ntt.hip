// ntt.hip -- the batched radix-2 transform over Fr (include/sylow_hip.h, "Fr: transforms on radix-2 domains"): m arrays of n = 2^log_n
//   elements, natural order in and out, forward  out_i = sum_k a_k (g w^i)^k  and inverse  out_k = n^-1 g^-k sum_i a_i w^(-ik).
// Three kernels: the twiddle table w^e, e < n/2, built per call; the passes (Stockham autosort: pass p is a radix-2^s step that reads its
// 2^s inputs n/2^s apart, multiplies in the twiddles that join it to the passes before, runs s radix-2 stages on chip and writes its digit
// transposed, so no pass needs a bit reversal of the array); and ONE element-wise kernel c s^k a_k for the coset shift and the inverse's scale.
// Geometry, ping-pong and scratch: ntt_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_dev.hpp"
#include "bn254_fr_roots.hpp"
#include "ntt_plan.hpp"

namespace ntt {
using namespace ntt_plan;
static_assert(NTT_BLOCK == BLOCK, "the kernels run blocks of BLOCK lanes");
static_assert(NTT_BLOCK >= 128, "the table kernel's second wavefront forms the shift");
constexpr int TILE = 1 << NTT_TILE_LOG, LOG_BLOCK = __builtin_ctz((unsigned)BLOCK);
static_assert(TILE >= 2 * BLOCK, "a lane owns whole butterflies");

struct Scalar : FrArg {};      // a kernel names its parameter types in its symbol: this one stays a type of this namespace so that the symbol does not move

// The table [4][half], half = n/2 = 2^(log_n - 1): block b holds the exponents from b * BLOCK * NTT_TABLE_LANE_ELEMS on, lane t those BLOCK
// apart from its first.  ONE wavefront squares the 2^28-th root down to w_n and on to pw[s] = w_n^(2^s), s <= log_n - 2 (a chain; the
// branch is wave-uniform); each lane multiplies its first power together from the set bits of its exponent and walks on with pw[LOG_BLOCK].
// shift != NULL: the second wavefront of block 0 leaves the multiplier of the element-wise kernel in consts: g mod r, or its inverse (inv(0) = 0).
__global__ void __launch_bounds__(BLOCK) k_ntt_table(int log_n, u64* table, const u64* shift, int inverse, u64* consts) {
  __shared__ __attribute__((aligned(16))) u32 pw[NTT_LOG_N_MAX][8];
  const int t = threadIdx.x;
  if (shift && blockIdx.x == 0 && t == 64) {
    const Fp g = fr_reduce_plain(load_plain(shift, 1, 0, 0));
    store_plain(consts, 1, 0, 0, inverse ? fr_inv(g) : g);
  }
  if (log_n < 1) return;
  const size_t half = (size_t)1 << (log_n - 1);
  if (t < 64) {
    Fp p = fp_from_limbs(BN_FR_ROOT28);
#pragma unroll 1
    for (int i = 0; i < root_squarings(log_n) + log_n - 1; ++i) {
      if (i >= root_squarings(log_n) && t == 0) lds_put(pw, i - root_squarings(log_n), p);
      p = fr_mul(p, p);
    }
  }
  __syncthreads();
  size_t e = (size_t)blockIdx.x * BLOCK * NTT_TABLE_LANE_ELEMS + t;
  if (e >= half) return;
  Fp p = fr_one();
#pragma unroll 1
  for (int s = 0; s + 1 < log_n; ++s)
    if ((e >> s) & 1) p = fr_mul(p, lds_get(pw, s));
#pragma unroll 1
  for (int i = 0; i < NTT_TABLE_LANE_ELEMS && e < half; ++i, e += BLOCK) {
    store_plain(table, half, e, 0, p);
    if (e + BLOCK < half) p = fr_mul(p, lds_get(pw, LOG_BLOCK));     // half > BLOCK: pw[LOG_BLOCK] was formed
  }
}

// w^e (inverse: w^-e) for e < n from the table of the first half: w^(n/2) = -1
BN_DEV Fp twiddle(const u64* table, size_t n, int inverse, size_t e) {
  const size_t half = n >> 1;
  if (inverse) e = (n - e) & (n - 1);
  return e < half ? load_plain(table, half, e, 0) : fr_neg(load_plain(table, half, e - half, 0));
}

// One pass of s stages over items (array, tile).  With R = 2^s, Ns = 2^done (the length the passes before have finished) and j < n/R:
//   v_r = in[j + r n/R] w^(r (j mod Ns) n/(Ns R)),   V = DFT_R(v),   out[(j div Ns) Ns R + (j mod Ns) + r' Ns] = V_r'.
// A tile holds the groups j = jb .. jb + G - 1, G = 2^glog, element (r, g) at row r G + g of LDS: consecutive lanes take consecutive g, which
// are consecutive words of the array on both sides.  The stages run decimation-in-frequency in place, half = R/2 .. 1, ONE product per
// butterfly (none in the last stage, whose twiddle is 1); that leaves V bit-reversed in r, which the store undoes by reading row
// bitrev(r') G + g.  raw: the input is the caller's (any words): taken mod r.  Every index is size_t; rows stay below 2^(s + glog) <= TILE.
__global__ void __launch_bounds__(BLOCK) k_ntt_pass(const u64* in, u64* out, int log_n, int s, int done, int glog, size_t tiles, size_t items,
                                                     const u64* table, int inverse, int raw) {
  __shared__ __attribute__((aligned(16))) u32 x[TILE][8];
  const int t = threadIdx.x, rows = 1 << (s + glog), gmask = (1 << glog) - 1;
  const size_t n = (size_t)1 << log_n, ns_mask = ((size_t)1 << done) - 1;
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t a = it / tiles, jb = (it - a * tiles) << glog;
    const u64* src = in + a * 4 * n;
    u64* dst = out + a * 4 * n;
#pragma unroll 1
    for (int i = t; i < rows; i += BLOCK) {
      const size_t r = (size_t)(i >> glog), j = jb + (size_t)(i & gmask), k = j & ns_mask;
      Fp v = load_plain(src, n, j + (r << (log_n - s)), 0);
      if (raw) v = fr_reduce_plain(v);
      if (r * k) v = fr_mul(v, twiddle(table, n, inverse, (r * k) << (log_n - done - s)));
      lds_put(x, i, v);
    }
    __syncthreads();
#pragma unroll 1
    for (int hl = s - 1; hl >= 0; --hl) {
#pragma unroll 1
      for (int b = t; b < rows / 2; b += BLOCK) {
        const int g = b & gmask, q = b >> glog, lo = q & ((1 << hl) - 1);
        const int i0 = ((((q >> hl) << (hl + 1)) | lo) << glog) | g, i1 = i0 + (1 << (hl + glog));
        const Fp u = lds_get(x, i0), w = lds_get(x, i1);
        lds_put(x, i0, fr_add(u, w));
        Fp d = fr_sub(u, w);
        if (hl) d = fr_mul(d, twiddle(table, n, inverse, (size_t)lo << (log_n - hl - 1)));
        lds_put(x, i1, d);
      }
      __syncthreads();
    }
#pragma unroll 1
    for (int i = t; i < rows; i += BLOCK) {
      const unsigned r = (unsigned)(i >> glog);
      const size_t j = jb + (size_t)(i & gmask), k = j & ns_mask;
      const int row = (int)((__brev(r) >> (32 - s)) << glog) | (i & gmask);
      store_plain(dst, n, ((j >> done) << (done + s)) + k + ((size_t)r << done), 0, lds_get(x, row));
    }
    __syncthreads();                                         // x is free for the next item
  }
}

// out_k = c s^k a_k over items (array, chunk of BLOCK * NTT_SCALE_LANE_ELEMS elements); a lane takes the elements BLOCK apart from its first.
// consts != NULL: s is read there (k_ntt_table left it), the lane forms c s^k0 by square-and-multiply and walks on with s^BLOCK;
// consts == NULL: s = 1, one product per element.  The input is taken mod r.
__global__ void __launch_bounds__(BLOCK) k_ntt_scale(const u64* in, u64* out, int log_n, size_t chunks, size_t items, Scalar c, const u64* consts) {
  const size_t n = (size_t)1 << log_n;
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t a = it / chunks;
    size_t k = (it - a * chunks) * BLOCK * NTT_SCALE_LANE_ELEMS + threadIdx.x;
    if (k >= n) continue;                                     // no barrier in this kernel
    const u64* src = in + a * 4 * n;
    u64* dst = out + a * 4 * n;
    Fp p = from_scalar(c), step = fr_one();
    if (consts) {
      const Fp sh = load_plain(consts, 1, 0, 0);
      Fp q = fr_one();
#pragma unroll 1
      for (int b = log_n - 1; b >= 0; --b) {
        q = fr_mul(q, q);
        if ((k >> b) & 1) q = fr_mul(q, sh);
      }
      p = fr_mul(p, q);
      step = sh;
#pragma unroll 1
      for (int b = 0; b < LOG_BLOCK; ++b) step = fr_mul(step, step);
    }
#pragma unroll 1
    for (int i = 0; i < NTT_SCALE_LANE_ELEMS && k < n; ++i, k += BLOCK) {
      store_plain(dst, n, k, 0, fr_mul(p, fr_reduce_plain(load_plain(src, n, k, 0))));
      if (consts && k + BLOCK < n) p = fr_mul(p, step);
    }
  }
}

static int32_t transform(const uint64_t* in, int log_n, size_t m, bool inverse, const uint64_t* shift, int stages, uint64_t* out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const bool shifted = shift != nullptr;
  const int n_pass = passes(log_n, stages), n_steps = steps(log_n, stages, inverse, shifted);
  host::Lease ws;
  const ScratchLayout l = scratch_layout(log_n, m, n_steps);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *consts = ws.at<u64>(l.consts), *table = ws.at<u64>(l.table), *buf = ws.at<u64>(l.buf);
  if (n_pass || shifted)
    k_ntt_table<<<dim3((unsigned)grid(table_blocks(log_n))), dim3(BLOCK), 0, st>>>(log_n, table, shift, inverse ? 1 : 0, consts);
  const Words4 ni = inverse ? n_inverse(log_n) : Words4{{1, 0, 0, 0}};
  const Scalar c = {{ni.w[0], ni.w[1], ni.w[2], ni.w[3]}};
  const u64* src = in;
  int step = 0;
  auto scale = [&]() {
    u64* dst = step_writes_out(n_steps, step) ? out : buf;
    const size_t items = scale_items(log_n, m);
    k_ntt_scale<<<dim3((unsigned)grid(items)), dim3(BLOCK), 0, st>>>(src, dst, log_n, scale_chunks(log_n), items, c, shifted ? consts : nullptr);
    src = dst;
    ++step;
  };
  if (scales(log_n, inverse, shifted) && !inverse) scale();
  for (int p = 0; p < n_pass; ++p, ++step) {
    u64* dst = step_writes_out(n_steps, step) ? out : buf;
    const int s = pass_stages(log_n, stages, p), glog = pass_group_log(log_n, s);
    const size_t items = pass_items(log_n, s, m);
    k_ntt_pass<<<dim3((unsigned)grid(items)), dim3(BLOCK), 0, st>>>(src, dst, log_n, s, pass_done_log(stages, p), glog, pass_tiles(log_n, s), items, table,
                                                                     inverse ? 1 : 0, src == in ? 1 : 0);
    src = dst;
  }
  if (inverse) scale();
  return host::finish(SYLOW_HIP_OK, ws);
}
}  // namespace ntt

namespace ntth {
// the table w_n^e, e < n / 2, [4][n / 2] (ntt_plan::table_words), for a unit that walks the same domain (g1_ntt.hip); log_n >= 1
int32_t build_table(int log_n, uint64_t* table, void* stream) {
  ntt::k_ntt_table<<<dim3((unsigned)ntt_plan::grid(ntt_plan::table_blocks(log_n))), dim3(BLOCK), 0, (hipStream_t)stream>>>(log_n, table, nullptr, 0, nullptr);
  LAUNCHED();
}
}  // namespace ntth

extern "C" {
int32_t sylow_hip_fr_ntt_batch_tuned(const uint64_t* in, int32_t log_n, size_t m, int32_t inverse, const uint64_t* shift, int32_t stages, uint64_t* out, void* stream) {
  using namespace ntt_plan;
  ARGCHK(log_n >= 0 && log_n <= NTT_LOG_N_MAX && (inverse == 0 || inverse == 1) && stages_ok(stages));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(in && out);
  const size_t bytes = mul_sat(batch_words(log_n, m), sizeof(uint64_t));
  ARGCHK(bytes != SAT);
  const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
  ARGCHK(a + bytes <= b || b + bytes <= a);                  // out must not overlap in: other blocks still read what this one writes
  return ntt::transform(in, log_n, m, inverse != 0, shift, stages_or_default(stages), out, stream);
}
int32_t sylow_hip_fr_ntt_batch(const uint64_t* in, int32_t log_n, size_t m, int32_t inverse, const uint64_t* shift, uint64_t* out, void* stream) {
  return sylow_hip_fr_ntt_batch_tuned(in, log_n, m, inverse, shift, -1, out, stream);
}
}  // extern "C"
