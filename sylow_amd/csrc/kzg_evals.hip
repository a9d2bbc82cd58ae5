// kzg_evals.hip -- KZG openings of polynomials held in EVALUATION form, and the batch inversion in Fr they rest on (include/sylow_hip.h,
//   "Fr: inverses that share one inversion" and "KZG, the prover's side, from evaluations"):
//   sylow_hip_fr_batch_inv        out_i = a_i^-1 (inv(0) = 0) by Montgomery's trick: the elements of a chunk share ONE inversion;
//   sylow_hip_kzg_quotient_evals_batch   y_j = f_j(z_j) by the barycentric formula and the values of (f_j - y_j) / (X - z_j) on the domain,
//                                  z_j inside the domain included (the d_i^-1 through the same chunk inversion);
//   sylow_hip_kzg_open_evals_batch       that quotient into scratch, then the commitment of kzg_prove.hip over a Lagrange-basis SRS.
// Geometry and scratch: kzg_evals_plan.hpp -- nothing here decides one.
#include "host.hpp"
#include "bn254_fr_block.hpp"
#include "bn254_fr_roots.hpp"
#include "kzg_evals_plan.hpp"
#include "ntt_plan.hpp"

namespace kze {
using namespace kzg_evals_plan;
static_assert(EVALS_BLOCK == BLOCK, "the kernels run one chunk per block of BLOCK lanes");
static_assert(EVALS_LOG_N_MAX == ntt_plan::NTT_LOG_N_MAX, "the domains of the transform");
constexpr int L = EVALS_LANE_ELEMS, CH = (int)EVALS_CHUNK, W_INV = EVALS_LOG_N_MAX;      // W_INV: the slot of w^-1

struct Scalar : FrArg {};      // a kernel names its parameter types in its symbol: this one stays a type of this namespace so that the symbol does not move
// elem, fr_inv_lone, block_inverses -- the chunk's ONE inversion -- and block_sum are bn254_fr_block.hpp's: fr_scan.hip and the weighted
// checks run the same

// ---- sylow_hip_fr_batch_inv ----------------------------------------------------------------------------------------------------------------
// A block per chunk, walked with a stride of whole blocks.  Forward, a lane multiplies its L elements together and keeps the L prefix
// products (registers: the loops are unrolled); an element = 0 mod r enters the chain as 1, an element past n too.  block_inverses turns the
// lane totals into their inverses.  Backward, out_i = run p_(i-1) and run *= a_i, the elements read a second time (from cache, mostly);
// the zero elements are written as 0.  out must not overlap a: the second read would meet the first stores.
__global__ void __launch_bounds__(BLOCK) k_fr_batch_inv(const u64* a, u64* out, size_t n, size_t n_chunks) {
  __shared__ u32 pre[BLOCK][8], suf[BLOCK][8], inv[1][8];
#pragma unroll 1
  for (size_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const size_t base = c * CH + (size_t)threadIdx.x * L;
    Fp p[L];
    Fp run = fr_one();
#pragma unroll
    for (int i = 0; i < L; ++i) {
      if (base + i < n) {
        const Fp v = elem(a, n, base + i);
        if (!fp_is_zero(v)) run = fr_mul(run, v);
      }
      p[i] = run;
    }
    Fp r = block_inverses(run, pre, suf, inv, live_lanes(n, c));
#pragma unroll
    for (int i = L - 1; i >= 0; --i) {
      const size_t k = base + i;
      if (k >= n) continue;
      const Fp v = elem(a, n, k);
      const bool zero = fp_is_zero(v);
      const Fp o = i ? fr_mul(r, p[i - 1]) : r;
      store_plain(out, n, k, 0, zero ? fr_zero() : o);
      if (i && !zero) r = fr_mul(r, v);
    }
    __syncthreads();                                         // pre, suf and inv are free for the next chunk
  }
}

// ---- the quotient from evaluations ---------------------------------------------------------------------------------------------------------
// roots [ROOT_SLOTS][4]: slot s < log_n holds w^(2^s), w = w_n; slot W_INV holds w^-1 = w^(n - 1), the product of them all.  ONE wavefront of
// block 0 squares the 2^28-th root down (28 squarings whatever log_n is, log_n products beside them); every thread of the grid clears hit
// slots to NO_HIT meanwhile.
__global__ void __launch_bounds__(BLOCK) k_evals_roots(int log_n, u64* roots, u64* hit, size_t m) {
  for (size_t j = TID; j < m; j += (size_t)gridDim.x * BLOCK) hit[j] = NO_HIT;
  if (blockIdx.x || threadIdx.x >= 64) return;
  // w_n by ntt_plan::root_squarings squarings, spelt out: behind a function the compiler closes this loop with the opposite branch
  Fp p = fp_from_limbs(BN_FR_ROOT28), wi = fr_one();
#pragma unroll 1
  for (int i = 0; i < ntt_plan::root_squarings(log_n); ++i) p = fr_mul(p, p);
#pragma unroll 1
  for (int s = 0; s < log_n; ++s) {
    if (threadIdx.x == 0) store_plain(roots + 4 * s, 1, 0, 0, p);
    wi = fr_mul(wi, p);
    p = fr_mul(p, p);
  }
  if (threadIdx.x == 0) store_plain(roots + 4 * W_INV, 1, 0, 0, wi);
}
// the slots a call filled, into LDS; the caller's next barrier publishes them
BN_DEV void load_roots(const u64* roots, int log_n, u32 (*pw)[8]) {
  const int s = threadIdx.x;
  if (s < log_n || s == W_INV) lds_put(pw, s, load_plain(roots + 4 * s, 1, 0, 0));
}
// w^e for e < n from its set bits
BN_DEV Fp root_power(const u32 (*pw)[8], int log_n, size_t e) {
  Fp p = fr_one();
#pragma unroll 1
  for (int s = 0; s < log_n; ++s)
    if ((e >> s) & 1) p = fr_mul(p, lds_get(pw, s));
  return p;
}

// Item (j, c): with d_i = z_j - w^i over the chunk's elements, the d_i^-1 (0 where d_i = 0: the hit, whose index goes to hit[j]) into dinv
// (the caller's q_out; NULL: not kept) and the chunk's part of  sum_i f_i w^i d_i^-1  into totals [4][items].  The lane walks w^i up by w on
// the way forward and down by w^-1 on the way back, so no power is held beside the L prefix products.
__global__ void __launch_bounds__(BLOCK) k_evals_dinv(const u64* evals, int log_n, size_t n_chunks, size_t items, const u64* zs, size_t m, const u64* roots,
                                                      u64* dinv, u64* totals, u64* hit) {
  __shared__ u32 pw[ROOT_SLOTS][8], pre[BLOCK][8], suf[BLOCK][8], inv[1][8];
  const size_t n = (size_t)1 << log_n;
  load_roots(roots, log_n, pw);
  __syncthreads();
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t j = it / n_chunks, c = it - j * n_chunks, base = c * CH + (size_t)threadIdx.x * L;
    const u64* f = evals + j * 4 * n;
    const Fp z = elem(zs, m, j);
    Fp x = base < n ? root_power(pw, log_n, base) : fr_one();
    Fp p[L];
    Fp run = fr_one();
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const size_t k = base + i;
      if (k < n) {
        const Fp d = fr_sub(z, x);
        if (fp_is_zero(d)) hit[j] = k;                       // at most one i of a polynomial: the w^i are distinct
        else run = fr_mul(run, d);
        if (i + 1 < L && k + 1 < n) x = fr_mul(x, lds_get(pw, 0));
      }
      p[i] = run;
    }
    Fp r = block_inverses(run, pre, suf, inv, live_lanes(n, c));
    Fp acc = fr_zero();
#pragma unroll
    for (int i = L - 1; i >= 0; --i) {
      const size_t k = base + i;
      if (k >= n) continue;
      const Fp d = fr_sub(z, x);
      const bool zero = fp_is_zero(d);
      const Fp o = zero ? fr_zero() : i ? fr_mul(r, p[i - 1]) : r;
      if (dinv) store_plain(dinv + j * 4 * n, n, k, 0, o);
      acc = fr_add(acc, fr_mul(fr_mul(elem(f, n, k), x), o));
      if (i) {
        if (!zero) r = fr_mul(r, d);
        x = fr_mul(x, lds_get(pw, W_INV));
      }
    }
    __syncthreads();                                         // pre is free for the sum
    const Fp s = block_sum(acc, pre);
    if (threadIdx.x == 0) store_plain(totals, items, it, 0, s);
  }
}
// A block per polynomial: S = the sum of its chunks' parts; then on one lane  y = f_k  for a hit at k, else  y = (z^n - 1) n^-1 S
// (log_n squarings of z).
__global__ void __launch_bounds__(BLOCK) k_evals_value(const u64* evals, int log_n, size_t n_chunks, size_t items, const u64* zs, size_t m, Scalar n_inv,
                                                       const u64* totals, const u64* hit, u64* y) {
  __shared__ u32 part[BLOCK][8];
  const size_t n = (size_t)1 << log_n;
#pragma unroll 1
  for (size_t j = blockIdx.x; j < m; j += gridDim.x) {
    Fp s = fr_zero();
#pragma unroll 1
    for (size_t c = threadIdx.x; c < n_chunks; c += BLOCK) s = fr_add(s, load_plain(totals, items, j * n_chunks + c, 0));
    s = block_sum(s, part);
    if (threadIdx.x == 0) {
      const u64 h = hit[j];
      Fp v;
      if (h != NO_HIT) {
        v = elem(evals + j * 4 * n, n, (size_t)h);
      } else {
        Fp zn = elem(zs, m, j);
#pragma unroll 1
        for (int i = 0; i < log_n; ++i) zn = fr_mul(zn, zn);
        v = fr_mul(fr_mul(fr_sub(zn, fr_one()), from_scalar(n_inv)), s);
      }
      store_plain(y, m, j, 0, v);
    }
  }
}
// Item (j, c):  q_i = (y_j - f_i) d_i^-1  over the d_i^-1 that k_evals_dinv left in q, in place (0 at a hit: its provisional value).  For a
// polynomial with a hit (block-uniform) the chunk's part of  sum_i q_i w^i  goes to totals as well.
__global__ void __launch_bounds__(BLOCK) k_evals_quot(const u64* evals, int log_n, size_t n_chunks, size_t items, size_t m, const u64* roots, const u64* y,
                                                      const u64* hit, u64* q, u64* totals) {
  __shared__ u32 pw[ROOT_SLOTS][8], part[BLOCK][8];
  const size_t n = (size_t)1 << log_n;
  load_roots(roots, log_n, pw);
  __syncthreads();
#pragma unroll 1
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t j = it / n_chunks, c = it - j * n_chunks, base = c * CH + (size_t)threadIdx.x * L;
    const u64* f = evals + j * 4 * n;
    u64* qj = q + j * 4 * n;
    const Fp yj = load_plain(y, m, j, 0);
    const bool repair = hit[j] != NO_HIT;
    Fp x = repair && base < n ? root_power(pw, log_n, base) : fr_one();
    Fp acc = fr_zero();
#pragma unroll 1
    for (int i = 0; i < L; ++i) {
      const size_t k = base + i;
      if (k >= n) break;
      const Fp v = fr_mul(fr_sub(yj, elem(f, n, k)), load_plain(qj, n, k, 0));
      store_plain(qj, n, k, 0, v);
      if (repair) {
        acc = fr_add(acc, fr_mul(v, x));
        if (i + 1 < L && k + 1 < n) x = fr_mul(x, lds_get(pw, 0));
      }
    }
    if (repair) {
      const Fp s = block_sum(acc, part);
      if (threadIdx.x == 0) store_plain(totals, items, it, 0, s);
    }
  }
}
// A block per polynomial, only those with a hit at k:  q_k = -w^-k sum_(i != k) q_i w^i  (the provisional q_k = 0 added nothing), which is
// f'(w^k): the quotient's value where the division is 0 / 0.
__global__ void __launch_bounds__(BLOCK) k_evals_repair(int log_n, size_t n_chunks, size_t items, size_t m, const u64* roots, const u64* totals, const u64* hit,
                                                        u64* q) {
  __shared__ u32 pw[ROOT_SLOTS][8], part[BLOCK][8];
  const size_t n = (size_t)1 << log_n;
  load_roots(roots, log_n, pw);
  __syncthreads();
#pragma unroll 1
  for (size_t j = blockIdx.x; j < m; j += gridDim.x) {
    const u64 h = hit[j];
    if (h == NO_HIT) continue;                               // block-uniform
    Fp s = fr_zero();
#pragma unroll 1
    for (size_t c = threadIdx.x; c < n_chunks; c += BLOCK) s = fr_add(s, load_plain(totals, items, j * n_chunks + c, 0));
    s = block_sum(s, part);
    if (threadIdx.x == 0) store_plain(q + j * 4 * n, n, (size_t)h, 0, fr_neg(fr_mul(root_power(pw, log_n, (n - (size_t)h) & (n - 1)), s)));
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
static int32_t quotient_evals(const uint64_t* evals, int log_n, size_t m, const uint64_t* z, uint64_t* q_out, uint64_t* y_out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const size_t n_chunks = poly_chunks(log_n), its = items(log_n, m);
  host::Lease ws;
  const QuotientLayout l = quotient_layout(log_n, m, y_out != nullptr);
  int32_t rc = ws.acquire(l.bytes, st);
  if (rc != SYLOW_HIP_OK) return rc;
  u64 *roots = ws.at<u64>(l.roots), *totals = ws.at<u64>(l.totals), *hit = ws.at<u64>(l.hit), *y = y_out ? y_out : ws.at<u64>(l.y);
  const ntt_plan::Words4 ni = ntt_plan::n_inverse(log_n);
  const Scalar n_inv = {{ni.w[0], ni.w[1], ni.w[2], ni.w[3]}};
  const dim3 per_item((unsigned)grid(its)), per_poly((unsigned)grid(m));
  k_evals_roots<<<dim3((unsigned)grid((m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st>>>(log_n, roots, hit, m);
  k_evals_dinv<<<per_item, dim3(BLOCK), 0, st>>>(evals, log_n, n_chunks, its, z, m, roots, q_out, totals, hit);
  k_evals_value<<<per_poly, dim3(BLOCK), 0, st>>>(evals, log_n, n_chunks, its, z, m, n_inv, totals, hit, y);
  if (q_out) {
    k_evals_quot<<<per_item, dim3(BLOCK), 0, st>>>(evals, log_n, n_chunks, its, m, roots, y, hit, q_out, totals);
    k_evals_repair<<<per_poly, dim3(BLOCK), 0, st>>>(log_n, n_chunks, its, m, roots, totals, hit, q_out);
  }
  return host::finish(SYLOW_HIP_OK, ws);
}
}  // namespace kze

extern "C" {
int32_t sylow_hip_fr_batch_inv(const uint64_t* a, uint64_t* out, size_t n, void* stream) {
  using namespace kzg_evals_plan;
  if (!n) return SYLOW_HIP_OK;
  ARGCHK(a && out);
  const size_t bytes = fr_array_bytes(n);
  ARGCHK(bytes != SAT && !overlaps((uintptr_t)a, (uintptr_t)out, bytes));      // the way back reads a again: out must not overlap it
  kze::k_fr_batch_inv<<<dim3((unsigned)batch_inv_grid(n)), dim3(BLOCK), 0, (hipStream_t)stream>>>(a, out, n, chunks(n));
  LAUNCHED();
}
int32_t sylow_hip_kzg_quotient_evals_batch(const uint64_t* evals, int32_t log_n, size_t m, const uint64_t* z, uint64_t* q_out, uint64_t* y_out, void* stream) {
  using namespace kzg_evals_plan;
  ARGCHK(log_n >= 0 && log_n <= EVALS_LOG_N_MAX); if (!m) return SYLOW_HIP_OK;
  ARGCHK(evals && z && (q_out || y_out));
  const size_t bytes = mul_sat(batch_words(log_n, m), sizeof(uint64_t));
  ARGCHK(bytes != SAT);
  ARGCHK(!q_out || !overlaps((uintptr_t)evals, (uintptr_t)q_out, bytes));      // other blocks still read what this one writes
  return kze::quotient_evals(evals, log_n, m, z, q_out, y_out, stream);
}
int32_t sylow_hip_kzg_open_evals_batch(const uint64_t* srs_lagrange_xy, const uint64_t* evals, int32_t log_n, size_t m, const uint64_t* z,
                                       uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream) {
  using namespace kzg_evals_plan;
  ARGCHK(log_n >= 0 && log_n <= EVALS_LOG_N_MAX); if (!m) return SYLOW_HIP_OK;
  ARGCHK(srs_lagrange_xy && evals && z && y_out && pi_xy && pi_inf);
  const size_t bytes = open_scratch_bytes(log_n, m);
  ARGCHK(bytes != SAT);
  host::Lease ws;
  int32_t rc = ws.acquire(bytes, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint64_t* q = ws.at<uint64_t>(0);
  rc = kze::quotient_evals(evals, log_n, m, z, q, y_out, stream);
  if (rc == SYLOW_HIP_OK) rc = kzgph::commit_canonical(srs_lagrange_xy, q, elems(log_n), m, pi_xy, pi_inf, stream);
  return host::finish(rc, ws);
}
}  // extern "C"
