// msm_bucket.hpp -- one large multi-scalar multiplication Q = sum_i k_i P_i by the bucket method (Pippenger) on the carry-free core, once for
// both groups.  Everything here is a template on a geometry policy G; msm.hip instantiates it with its one-lane G1 policy, g2_msm.hpp (the
// tail of plk_group.hip) with its lane-pair G2 policy.  The build has no relocatable device code: a policy type lives in ONE unit, so each
// unit compiles, and launches, its own copies of the kernels.  Nothing below names a group.  G states:
//   F, wrap, limbs   the coordinate type (a point is Proj<F>), how an F29 becomes one and where its nine limbs are
//   Ops              the group law's ops policy: the complete formulas proj_add_lazy / proj_double_lazy, and zero / one / neg
//   LANES            lanes per point.  Thread g works on coordinate role(g) of element elem(g); every array of points is
//                    a[word * LANES * count + LANES * i + role], 27 words per lane, and a launch over x elements covers LANES * x threads
//   MOD_R            whether the scalars are reduced mod r on top of Fp::new: true where every point has order r, i.e. on E(Fp); false on
//                    the twist, whose points need not have order r -- there the digits are those of k mod p itself
//   prepare, finish  affine SoA words -> this lane's (x : y : 1) in carry-free form; the projective result -> canonical affine words + flag
//   DEFAULT_MIN, default_window, REDUCE_WAVES   the tuning that differs: the size from which the bucket route is the default, the default
//                    window width, and the waves per SIMD k_msm_bucket_reduce is compiled for
//
// Per chunk of points (one chunk unless the scratch budget is short; every chunk adds into the same buckets):
//   k_msm_prep       G::prepare once per point, so that the W additions of a point convert nothing; one 80-byte record per point and
//                    lane (x, y, 2 words of padding): a random gather is five 16-byte loads from two cache lines, not 18 4-byte loads from
//                    18 rows of an SoA array
//   k_msm_hist       scalar -> k mod p (-> mod r) -> W signed c-bit digits in [-2^(c-1), 2^(c-1)]; count[w][|d| - 1] += 1 (zero digits drop out)
//   k_msm_scan_*     ONE flat exclusive scan over all W * 2^(c-1) buckets of (segments << 32 | entries), segments = ceil(entries / MSM_SEG)
//   k_msm_scatter    the same digits again: index | sign << 31 into the bucket's slot range (a counting sort; order inside a bucket is free)
//   k_msm_seg        one point's lanes per segment of <= MSM_SEG entries of one bucket: the complete addition (proj_add_lazy) with Z = 1
//                    operands, in registers; a bucket of one segment adds straight into its bucket, longer buckets leave one partial per segment
//   k_msm_seg_join   one point's lanes per bucket of 2 .. JOIN_LANE_MAX segments: bucket += its partials
//   k_msm_seg_join_wide  one BLOCK per bucket of more segments: the partials split over its BLOCK / LANES points, then a tree in LDS -- a hot
//                    bucket (all scalars equal, scalars from {0, 1}, the narrow top window) costs ns / 256 + 8 dependent additions (ns / 128 + 7 on
//                    lane pairs), not ns
// Then once:
//   k_msm_bucket_reduce  running sums sum_m m B_m over MSM_RUN contiguous buckets per point's lanes, corrected by (offset) x (range sum)
//   k_msm_window_sum     one block per window: the partials -> S_w
//   k_msm_combine        Horner over the windows (c doublings + one addition each) on one point's lanes, then G::finish
// The complete formulas throughout: a doubling, an identity or a cancelling pair inside a bucket needs no special case.
// tools/msm_model.py is the host-side model of the recoding, the plan and the scratch formula.
#pragma once
#include "host.hpp"

namespace msm {
constexpr int MSM_SEG = 32;            // entries per accumulation segment
constexpr u32 JOIN_LANE_MAX = 8;       // segments a bucket may have to be joined by one point's lanes; more go to k_msm_seg_join_wide
constexpr int MSM_RUN = 16;            // buckets per point's lanes in the running-sum reduction
constexpr int MSM_C_MIN = 4;           // window widths the _tuned entry points accept
constexpr int MSM_C_MAX = 16;
constexpr int SCAN_ITEMS = 4, SCAN_TILE = BLOCK * SCAN_ITEMS;   // 1024 entries per scan block
constexpr size_t MSM_DEFAULT_BUDGET = (size_t)1 << 30;
constexpr size_t PROJ_LANE_WORDS = 27; // words (i32) per lane of a projective point
constexpr size_t PT_LANE_WORDS = 20;   // words (i32) per lane of a prepared affine point: x, y, padding to 80 bytes
template <class G> constexpr size_t PROJ_WORDS = PROJ_LANE_WORDS * G::LANES;   // a bucket, a segment partial, a reduction partial, a window sum
template <class G> constexpr size_t PT_WORDS = PT_LANE_WORDS * G::LANES;
template <class G> constexpr u32 POINTS = BLOCK / G::LANES;                    // points a block works on
template <class G> using Pt = Proj<typename G::F>;

// ------------------------------------------------------------------ recode ----------
// scalar i as an Fp value (Fp::new: k >= p is reduced), and with MOD_R then mod the group order (every point of E(Fp) has order r) --
// k < 2^256 straight mod r would differ for k >= p
template <class G>
BN_DEV void msm_scalar(u32 (&k)[8], const u64* ks, size_t n, size_t i) {
  load_scalar(k, ks, n, i);
  if (G::MOD_R) cond_sub_const(k, 0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u);   // r (k < p < 2r)
}
// bits [bit, bit + c) of k, c <= 16 (word index through selects: no dynamically indexed register array)
BN_DEV u32 msm_bits(const u32 (&k)[8], int bit, int c) {
  const int q = bit >> 5, s = bit & 31;
  u32 lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { lo = j == q ? k[j] : lo; hi = j == q + 1 ? k[j] : hi; }
  return (u32)((((u64)hi << 32) | lo) >> s) & ((1u << c) - 1u);
}
// the signed digit of window w given the carry out of window w - 1 (in / out): d in [-2^(c-1), 2^(c-1)]; k < 2^254 and W c >= 255 leave
// no carry out of the top window
BN_DEV int msm_digit(const u32 (&k)[8], int w, int c, int& carry) {
  int d = (int)msm_bits(k, w * c, c) + carry;
  carry = d > (1 << (c - 1));
  return d - (carry << c);
}
// atomicAdd(&ctr[key], 1) for every active lane with `on`, returning the old value, with the lanes of a wavefront that share a key served by ONE
// atomic (up to AGG_ROUNDS distinct keys per wavefront; the rest one atomic per lane).  Hot buckets -- every scalar equal, scalars from {0, 1},
// the few buckets of a narrow top window -- otherwise queue 64 atomics per wavefront on one address.  Call with the whole wavefront converged.
constexpr int AGG_ROUNDS = 4;
BN_DEV u32 agg_atomic_inc(u32* ctr, u32 key, bool on) {
  u32 pos = 0;
  bool done = !on;
#pragma unroll 1
  for (int r = 0; r < AGG_ROUNDS; ++r) {
    const unsigned long long act = __ballot(!done);
    if (!act) return pos;
    const int leader = __ffsll((long long)act) - 1;
    const u32 lk = (u32)__shfl((int)key, leader);
    const bool mine = !done && key == lk;
    const unsigned long long grp = __ballot(mine);
    u32 first = 0;
    if ((int)__lane_id() == leader) first = atomicAdd(&ctr[lk], (u32)__popcll(grp));
    first = (u32)__shfl((int)first, leader);
    if (mine) {
      pos = first + __builtin_amdgcn_mbcnt_hi((u32)(grp >> 32), __builtin_amdgcn_mbcnt_lo((u32)grp, 0u));
      done = true;
    }
  }
  if (!done) pos = atomicAdd(&ctr[key], 1u);
  return pos;
}
template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_hist(const uint8_t* pinf, const u64* ks, size_t n, size_t base, size_t nc, int c, int W, u32* cnt) {
  const size_t t = TID;
  if (t >= nc) return;
  const size_t i = base + t;
  const bool skip = pinf && pinf[i];                    // stays in the loop: agg_atomic_inc wants the wavefront converged
  u32 k[8];
  msm_scalar<G>(k, ks, n, i);
  const size_t B = (size_t)1 << (c - 1);
  int carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int d = skip ? 0 : msm_digit(k, w, c, carry);
    (void)agg_atomic_inc(cnt, (u32)((size_t)w * B + (size_t)((d < 0 ? -d : d) - 1)), d != 0);
  }
}
template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_scatter(const uint8_t* pinf, const u64* ks, size_t n, size_t base, size_t nc, int c, int W, u32* cursor, u32* idx) {
  const size_t t = TID;
  if (t >= nc) return;
  const size_t i = base + t;
  const bool skip = pinf && pinf[i];                    // stays in the loop: agg_atomic_inc wants the wavefront converged
  u32 k[8];
  msm_scalar<G>(k, ks, n, i);
  const size_t B = (size_t)1 << (c - 1);
  int carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int d = skip ? 0 : msm_digit(k, w, c, carry);
    const u32 pos = agg_atomic_inc(cursor, (u32)((size_t)w * B + (size_t)((d < 0 ? -d : d) - 1)), d != 0);
    if (d) idx[pos] = (u32)t | (d < 0 ? 0x80000000u : 0u);
  }
}
// ------------------------------------------------------------------ scan ----------
// exclusive scan of one tile of SCAN_TILE u64 values in place; returns the tile total (thread-uniform)
BN_DEV u64 tile_exscan(u64 (&v)[SCAN_ITEMS], u64* lds) {
  const int t = threadIdx.x;
  u64 s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) { const u64 x = v[j]; v[j] = s; s += x; }
  lds[t] = s;
  __syncthreads();
  for (int off = 1; off < BLOCK; off <<= 1) {
    const u64 x = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += x;
    __syncthreads();
  }
  const u64 before = lds[t] - s, total = lds[BLOCK - 1];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) v[j] += before;
  return total;
}
// counts -> packed (segments << 32 | entries), tile-exclusive scan into off, tile totals into tops
template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_scan_tiles(const u32* cnt, size_t N, u64* off, u64* tops) {
  __shared__ u64 lds[BLOCK];
  const size_t b0 = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
  u64 v[SCAN_ITEMS];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    const u64 e = b0 + j < N ? cnt[b0 + j] : 0;
    v[j] = ((e + MSM_SEG - 1) / MSM_SEG) << 32 | e;
  }
  const u64 total = tile_exscan(v, lds);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) if (b0 + j < N) off[b0 + j] = v[j];
  if (threadIdx.x == 0) tops[blockIdx.x] = total;
}
// one block: exclusive scan of the m <= SCAN_TILE tile totals in place, grand total into *meta
template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_scan_tops(u64* tops, size_t m, u64* meta) {
  __shared__ u64 lds[BLOCK];
  const size_t b0 = (size_t)threadIdx.x * SCAN_ITEMS;
  u64 v[SCAN_ITEMS];
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) v[j] = b0 + j < m ? tops[b0 + j] : 0;
  const u64 total = tile_exscan(v, lds);
#pragma unroll
  for (int j = 0; j < SCAN_ITEMS; ++j) if (b0 + j < m) tops[b0 + j] = v[j];
  if (threadIdx.x == 0) *meta = total;
}
// tile offsets in; the scatter cursors (entry offsets) out
template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_scan_add(u64* off, size_t N, const u64* tops, u32* cursor) {
  const size_t b = TID;
  if (b >= N) return;
  const u64 o = off[b] + tops[b / SCAN_TILE];
  off[b] = o;
  cursor[b] = (u32)o;
}

// ------------------------------------------------------------------ point SoA and prepared records --------------
// a [27][LANES * count] i32: word q of element i, coordinate `role`, at a[q * LANES * count + LANES * i + role]
template <class G>
BN_DEV typename G::F ld9(const i32* a, size_t stride, size_t slot, int w0) {
  F29 r;
#pragma unroll
  for (int q = 0; q < 9; ++q) r.v[q] = a[(size_t)(w0 + q) * stride + slot];
  return G::wrap(r);
}
template <class G>
BN_DEV void st9(i32* a, size_t stride, size_t slot, int w0, const typename G::F& x) {
#pragma unroll
  for (int q = 0; q < 9; ++q) a[(size_t)(w0 + q) * stride + slot] = G::limbs(x).v[q];
}
template <class G>
BN_DEV Pt<G> ldp(const i32* a, size_t count, size_t i, int role) {
  const size_t stride = G::LANES * count, slot = G::LANES * i + (size_t)role;
  return Pt<G>{ld9<G>(a, stride, slot, 0), ld9<G>(a, stride, slot, 9), ld9<G>(a, stride, slot, 18)};
}
template <class G>
BN_DEV void stp(i32* a, size_t count, size_t i, int role, const Pt<G>& p) {
  const size_t stride = G::LANES * count, slot = G::LANES * i + (size_t)role;
  st9<G>(a, stride, slot, 0, p.x); st9<G>(a, stride, slot, 9, p.y); st9<G>(a, stride, slot, 18, p.z);
}
template <class G> BN_DEV Pt<G> msm_add(const Pt<G>& a, const Pt<G>& b) { return proj_add_lazy<typename G::Ops>(a, b); }
template <class G> BN_DEV Pt<G> msm_dbl(const Pt<G>& a) { return proj_double_lazy<typename G::Ops>(a); }

template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_prep(const u64* pxy, size_t n, size_t base, size_t nc, int4* pts) {
  const size_t g = TID, t = G::elem(g);
  const int role = G::role(g);
  if (t >= nc) return;
  const Pt<G> p = G::prepare(pxy, n, base + t, role);
  const F29 &x = G::limbs(p.x), &y = G::limbs(p.y);
  int4* d = pts + t * (PT_WORDS<G> / 4) + (size_t)role * (PT_LANE_WORDS / 4);
  d[0] = make_int4(x.v[0], x.v[1], x.v[2], x.v[3]);
  d[1] = make_int4(x.v[4], x.v[5], x.v[6], x.v[7]);
  d[2] = make_int4(x.v[8], y.v[0], y.v[1], y.v[2]);
  d[3] = make_int4(y.v[3], y.v[4], y.v[5], y.v[6]);
  d[4] = make_int4(y.v[7], y.v[8], 0, 0);
}
// prepared point t as (x : +-y : 1), this lane's coordinates
template <class G>
BN_DEV Pt<G> msm_point(const int4* __restrict__ pts, u32 t, bool neg, int role) {
  const int4* s = pts + (size_t)t * (PT_WORDS<G> / 4) + (size_t)role * (PT_LANE_WORDS / 4);
  const int4 a = s[0], b = s[1], c = s[2], d = s[3], e = s[4];
  Pt<G> p{G::wrap(F29{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x}}), G::wrap(F29{{c.y, c.z, c.w, d.x, d.y, d.z, d.w, e.x, e.y}}), G::Ops::one()};
  if (neg) p.y = G::Ops::neg(p.y);
  return p;
}

// ------------------------------------------------------------------ bucket accumulation ----------
template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_bucket_init(i32* bk, size_t N) {
  const size_t g = TID, b = G::elem(g);
  const int role = G::role(g);
  if (b >= N) return;
  stp<G>(bk, N, b, role, proj_zero<typename G::Ops>());
}
// point s = segment s of the flat segment order: its bucket is the last b with seg_off(b) <= s (empty buckets share the next one's offset)
template <class G>
__global__ void HEAVY_BOUNDS k_msm_seg(const u64* off, const u32* cnt, size_t N, const u64* meta, size_t seg_cap, const u32* idx, const int4* pts,
                                       i32* bk, i32* part) {
  const size_t g = TID, s = G::elem(g);
  const int role = G::role(g);
  const u64 total = *meta;
  if (s >= (total >> 32) || s >= seg_cap) return;
  size_t lo = 0, hi = N - 1;                            // seg_off(0) = 0 <= s
  while (lo < hi) {
    const size_t mid = (lo + hi + 1) / 2;
    if ((off[mid] >> 32) <= s) lo = mid; else hi = mid - 1;
  }
  const size_t b = lo;
  const u64 o = off[b];
  const u32 e = cnt[b];
  const u32 j = (u32)(s - (o >> 32));
  const u32 first = (u32)o + j * MSM_SEG, last = min((u32)o + e, first + MSM_SEG);
  Pt<G> acc = msm_point<G>(pts, idx[first] & 0x7fffffffu, idx[first] >> 31, role);
#pragma unroll 1
  for (u32 q = first + 1; q < last; ++q) {
    const u32 u = idx[q];
    acc = msm_add<G>(acc, msm_point<G>(pts, u & 0x7fffffffu, u >> 31, role));
  }
  if (e <= MSM_SEG) stp<G>(bk, N, b, role, msm_add<G>(ldp<G>(bk, N, b, role), acc));   // the bucket's only segment: these lanes own it
  else stp<G>(part, seg_cap, s, role, acc);
}
template <class G>
__global__ void HEAVY_BOUNDS k_msm_seg_join(const u64* off, const u32* cnt, size_t N, size_t seg_cap, i32* bk, const i32* part) {
  const size_t g = TID, b = G::elem(g);
  const int role = G::role(g);
  if (b >= N) return;
  const u32 e = cnt[b];
  if (e <= MSM_SEG || e > JOIN_LANE_MAX * MSM_SEG) return;
  const size_t s0 = (size_t)(off[b] >> 32), ns = (e + MSM_SEG - 1) / MSM_SEG;
  Pt<G> acc = ldp<G>(bk, N, b, role);
#pragma unroll 1
  for (size_t j = 0; j < ns; ++j) acc = msm_add<G>(acc, ldp<G>(part, seg_cap, s0 + j, role));
  stp<G>(bk, N, b, role, acc);
}
// the block's POINTS points -> their sum, returned to every one of them (a level per barrier; lds: PROJ_WORDS * POINTS = 27 * BLOCK words,
// free again on return)
template <class G>
BN_DEV Pt<G> block_sum(const Pt<G>& mine, i32* lds, u32 p, int role) {
  stp<G>(lds, POINTS<G>, p, role, mine);
  __syncthreads();
  for (u32 h = POINTS<G> / 2; h > 0; h >>= 1) {
    if (p < h) stp<G>(lds, POINTS<G>, p, role, msm_add<G>(ldp<G>(lds, POINTS<G>, p, role), ldp<G>(lds, POINTS<G>, p + h, role)));
    __syncthreads();
  }
  const Pt<G> r = ldp<G>(lds, POINTS<G>, 0, role);
  __syncthreads();
  return r;
}
// blocks stride over tiles of BLOCK buckets; each collects its tile's buckets of > JOIN_LANE_MAX segments and joins them one after the other,
// every one with all of its POINTS points
template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_seg_join_wide(const u64* off, const u32* cnt, size_t N, size_t seg_cap, i32* bk, const i32* part) {
  __shared__ i32 lds[PROJ_WORDS<G> * POINTS<G>];
  __shared__ u32 heavy[BLOCK];
  __shared__ u32 n_heavy;
  const int t = threadIdx.x, role = G::role((u32)t);
  const u32 p = G::elem((u32)t);
  for (size_t base = (size_t)blockIdx.x * BLOCK; base < N; base += (size_t)gridDim.x * BLOCK) {
    if (t == 0) n_heavy = 0;
    __syncthreads();
    if (base + t < N && cnt[base + t] > JOIN_LANE_MAX * MSM_SEG) heavy[atomicAdd(&n_heavy, 1u)] = (u32)t;
    __syncthreads();
    const u32 m = n_heavy;
    for (u32 h = 0; h < m; ++h) {
      const size_t b = base + heavy[h];
      const size_t s0 = (size_t)(off[b] >> 32), ns = (cnt[b] + MSM_SEG - 1) / MSM_SEG;
      Pt<G> acc = proj_zero<typename G::Ops>();
#pragma unroll 1
      for (size_t j = p; j < ns; j += POINTS<G>) acc = msm_add<G>(acc, ldp<G>(part, seg_cap, s0 + j, role));
      acc = block_sum<G>(acc, lds, p, role);
      if (p == 0) stp<G>(bk, N, b, role, msm_add<G>(ldp<G>(bk, N, b, role), acc));
    }
    __syncthreads();                                    // every thread has read n_heavy before it is reset
  }
}

// ------------------------------------------------------------------ window reduction and combination ----------
// point (w, t): buckets t R .. t R + R - 1 of window w (magnitudes t R + 1 .. t R + R).  Running sums from the top give sum_j (j + 1) B_j;
// adding t R times the range sum makes it sum_m m B_m.  Partial -> red[w T + t].
template <class G>
__global__ void __launch_bounds__(BLOCK, G::REDUCE_WAVES) k_msm_bucket_reduce(const i32* bk, size_t N, int W, size_t B, size_t R, i32* red) {
  const size_t T = B / R, g = G::elem(TID);
  const int role = G::role(TID);
  if (g >= (size_t)W * T) return;
  const size_t w = g / T, t = g % T, base = w * B + t * R;
  Pt<G> run = proj_zero<typename G::Ops>(), acc = proj_zero<typename G::Ops>();
#pragma unroll 1
  for (size_t j = R; j-- > 0;) {
    run = msm_add<G>(run, ldp<G>(bk, N, base + j, role));
    acc = msm_add<G>(acc, run);
  }
  const u32 m = (u32)(t * R);                           // < 2^15
  if (m) {
    Pt<G> q = proj_zero<typename G::Ops>();
#pragma unroll 1
    for (int bit = 31 - __builtin_clz(m); bit >= 0; --bit) {
      q = msm_dbl<G>(q);
      if ((m >> bit) & 1u) q = msm_add<G>(q, run);
    }
    acc = msm_add<G>(acc, q);
  }
  stp<G>(red, (size_t)W * T, g, role, acc);
}
// block w: S_w = sum of the T partials of window w (serial per point, then a tree in LDS)
template <class G>
__global__ void __launch_bounds__(BLOCK) k_msm_window_sum(const i32* red, int W, size_t T, i32* win) {
  __shared__ i32 lds[PROJ_WORDS<G> * POINTS<G>];
  const size_t w = blockIdx.x, count = (size_t)W * T;
  const u32 p = G::elem((u32)threadIdx.x);
  const int role = G::role((u32)threadIdx.x);
  Pt<G> acc = proj_zero<typename G::Ops>();
#pragma unroll 1
  for (size_t j = p; j < T; j += POINTS<G>) acc = msm_add<G>(acc, ldp<G>(red, count, w * T + j, role));
  acc = block_sum<G>(acc, lds, p, role);
  if (p == 0) stp<G>(win, (size_t)W, w, role, acc);
}
template <class G>
__global__ void __launch_bounds__(64) k_msm_combine(const i32* win, int W, int c, u64* oxy, uint8_t* oinf) {
  if (G::elem((u32)threadIdx.x) != 0) return;          // one point: its LANES lanes
  const int role = G::role((u32)threadIdx.x);
  Pt<G> acc = ldp<G>(win, (size_t)W, (size_t)W - 1, role);
#pragma unroll 1
  for (int w = W - 2; w >= 0; --w) {
#pragma unroll 1
    for (int j = 0; j < c; ++j) acc = msm_dbl<G>(acc);
    acc = msm_add<G>(acc, ldp<G>(win, (size_t)W, (size_t)w, role));
  }
  G::finish(oxy, oinf, role, acc);
}

// ================================================================== host ======================
// ------------------------------------------------------------------ the plan of one call ----------
// (tools/msm_model.py mirrors every formula here.)
struct Plan {
  int c, W;
  size_t B, N, R, T, nc, seg_cap, bytes;
};
// bits of a scalar < 2^254 that the top window holds: few bits = few buckets that every point of that window falls into
inline int top_bits(int c) { return 254 - c * ((255 + c - 1) / c - 1); }
// c0 = floor(log2 n) - 4 clamped to [8, 16]; of c0, c0 - 1, c0 + 1 (inside [8, 16]) the one with the widest top window, c0 on ties
// (c0 = 12 -> 13, 14 -> 15: their top windows hold 2 bits, 13's and 15's 7 and 14)
inline int default_window(size_t n) {
  int lg = 0;
  while (lg < 62 && ((size_t)2 << lg) <= n) ++lg;
  const int c0 = lg - 4 < 8 ? 8 : (lg - 4 > MSM_C_MAX ? MSM_C_MAX : lg - 4);
  int best = c0;
  for (int c : {c0 - 1, c0 + 1})
    if (c >= 8 && c <= MSM_C_MAX && top_bits(c) > top_bits(best)) best = c;
  return best;
}
inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t seg_bound(int W, size_t N, size_t nc) { const size_t e = (size_t)W * nc; return e / MSM_SEG + 1 + (N < e ? N : e); }
// bytes of the fixed part (buckets, scan, reduction) and of a chunk of nc points
template <class G>
inline size_t fixed_bytes(int W, size_t N, size_t T) {
  const size_t tiles = (N + SCAN_TILE - 1) / SCAN_TILE;
  return align_up(N * 4) + align_up(N * 8) + align_up(N * 4) + align_up(tiles * 8) + align_up(8) + align_up(N * PROJ_WORDS<G> * 4) +
         align_up((size_t)W * T * PROJ_WORDS<G> * 4) + align_up((size_t)W * PROJ_WORDS<G> * 4);
}
template <class G>
inline size_t chunk_bytes(int W, size_t N, size_t nc) {
  return align_up(nc * PT_WORDS<G> * 4) + align_up((size_t)W * nc * 4) + align_up(seg_bound(W, N, nc) * PROJ_WORDS<G> * 4);
}
// the bucket route's plan for n points under `budget` bytes; false when not even a chunk of 256 points fits
template <class G>
inline bool plan(size_t n, int c, size_t budget, Plan& p) {
  p.c = c; p.W = (255 + c - 1) / c; p.B = (size_t)1 << (c - 1); p.N = (size_t)p.W * p.B;
  p.R = p.B < (size_t)MSM_RUN ? p.B : (size_t)MSM_RUN; p.T = p.B / p.R;
  const size_t fixed = fixed_bytes<G>(p.W, p.N, p.T);
  size_t nc = n < ((size_t)1 << 31) / (size_t)p.W ? n : ((size_t)1 << 31) / (size_t)p.W;   // chunk-local indices and entry offsets stay below 2^31
  const size_t floor_nc = n < 256 ? n : 256;
  if (fixed + chunk_bytes<G>(p.W, p.N, floor_nc) > budget) return false;
  if (fixed + chunk_bytes<G>(p.W, p.N, nc) > budget) {      // largest chunk that fits (chunk_bytes is monotone in nc)
    size_t lo = floor_nc, hi = nc;
    while (lo < hi) {
      const size_t mid = lo + (hi - lo + 1) / 2;
      if (fixed + chunk_bytes<G>(p.W, p.N, mid) <= budget) lo = mid; else hi = mid - 1;
    }
    nc = lo;
  }
  p.nc = nc;
  p.seg_cap = seg_bound(p.W, p.N, nc);
  p.bytes = fixed + chunk_bytes<G>(p.W, p.N, nc);
  return true;
}

// ------------------------------------------------------------------ the launch sequence ----------
template <class G>
int32_t bucket_route(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, const Plan& P, void* base, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  uint8_t* q = (uint8_t*)base;
  auto take = [&](size_t bytes) { void* r = q; q += align_up(bytes); return r; };
  const size_t tiles = (P.N + SCAN_TILE - 1) / SCAN_TILE;
  u32* cnt = (u32*)take(P.N * 4);
  u64* off = (u64*)take(P.N * 8);
  u32* cursor = (u32*)take(P.N * 4);
  u64* tops = (u64*)take(tiles * 8);
  u64* meta = (u64*)take(8);
  i32* bk = (i32*)take(P.N * PROJ_WORDS<G> * 4);
  i32* red = (i32*)take((size_t)P.W * P.T * PROJ_WORDS<G> * 4);
  i32* win = (i32*)take((size_t)P.W * PROJ_WORDS<G> * 4);
  int4* pts = (int4*)take(P.nc * PT_WORDS<G> * 4);
  u32* idx = (u32*)take((size_t)P.W * P.nc * 4);
  i32* part = (i32*)take(P.seg_cap * PROJ_WORDS<G> * 4);
  const hipStream_t st = (hipStream_t)stream;
  k_msm_bucket_init<G><<<GRID(G::LANES * P.N)>>>(bk, P.N);
  for (size_t b0 = 0; b0 < n; b0 += P.nc) {
    const size_t nc = n - b0 < P.nc ? n - b0 : P.nc;
    HIPCHK(hipMemsetAsync(cnt, 0, P.N * 4, st));
    k_msm_prep<G><<<GRID(G::LANES * nc)>>>(p_xy, n, b0, nc, pts);
    k_msm_hist<G><<<GRID(nc)>>>(p_inf, k, n, b0, nc, P.c, P.W, cnt);
    k_msm_scan_tiles<G><<<dim3((unsigned)tiles), dim3(BLOCK), 0, st>>>(cnt, P.N, off, tops);
    k_msm_scan_tops<G><<<1, BLOCK, 0, st>>>(tops, tiles, meta);
    k_msm_scan_add<G><<<GRID(P.N)>>>(off, P.N, tops, cursor);
    k_msm_scatter<G><<<GRID(nc)>>>(p_inf, k, n, b0, nc, P.c, P.W, cursor, idx);
    // the segment count is only known on the device: launch its bound (seg_bound of THIS chunk), surplus lanes leave at once
    const size_t segs = seg_bound(P.W, P.N, nc);
    k_msm_seg<G><<<GRID(G::LANES * segs)>>>(off, cnt, P.N, meta, P.seg_cap, idx, pts, bk, part);
    k_msm_seg_join<G><<<GRID(G::LANES * P.N)>>>(off, cnt, P.N, P.seg_cap, bk, part);
    const size_t tiles_b = (P.N + BLOCK - 1) / BLOCK;
    k_msm_seg_join_wide<G><<<dim3((unsigned)(tiles_b < 1024 ? tiles_b : 1024)), dim3(BLOCK), 0, st>>>(off, cnt, P.N, P.seg_cap, bk, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return host::fail(e, G::CHUNK_LAUNCH);
  }
  k_msm_bucket_reduce<G><<<GRID(G::LANES * (size_t)P.W * P.T)>>>(bk, P.N, P.W, P.B, P.R, red);
  k_msm_window_sum<G><<<dim3((unsigned)P.W), dim3(BLOCK), 0, st>>>(red, P.W, P.T, win);
  k_msm_combine<G><<<1, 64, 0, st>>>(win, P.W, P.c, out_xy, out_inf);
  LAUNCHED();
}
// A _tuned entry point: the bucket route from min_n points on (min_n_arg < 0: G::DEFAULT_MIN) at `window` (< 0: G::default_window) when a plan
// fits the scratch budget, else the unit's per-point route `small`
template <class G, class Small>
int32_t tuned(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, int32_t window, int64_t min_n_arg, uint64_t* out_xy, uint8_t* out_inf,
              void* stream, Small small) {
  ARGCHK(out_xy && out_inf && (n == 0 || (p_xy && k)));
  ARGCHK(window < 0 || (window >= MSM_C_MIN && window <= MSM_C_MAX));
  const size_t min_n = min_n_arg < 0 ? G::DEFAULT_MIN : (size_t)min_n_arg;
  if (n > 0 && n >= min_n) {
    const size_t lim = host::scratch_limit();
    Plan P;
    if (plan<G>(n, window < 0 ? G::default_window(n) : window, lim ? lim : MSM_DEFAULT_BUDGET, P)) {
      host::Lease ws;
      int32_t rc = ws.acquire(P.bytes, (hipStream_t)stream);
      if (rc != SYLOW_HIP_OK) return rc;
      rc = bucket_route<G>(p_xy, p_inf, k, n, P, ws.p, out_xy, out_inf, stream);
      return host::finish(rc, ws);
    }
  }
  return small();
}
}  // namespace msm
