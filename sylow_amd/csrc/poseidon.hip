// poseidon.hip -- batched Poseidon over Fr (the circomlib instance: x^5, t = 2 .. 17, R_F = 8, R_P per width) and binary Merkle trees whose
// node is hash([left, right]) (include/sylow_poseidon.h):
//   sylow_poseidon_prepare               the parameter table of a width: the host's Grain draws, and the t^2 inverses of M on the device;
//   sylow_poseidon_permute_batch         n permutations;            sylow_poseidon_hash_batch   element 0 of the permutation of [init, in..];
//   sylow_poseidon_merkle_build_batch    m trees, one launch per level over (tree, node) items;
//   sylow_poseidon_merkle_open_batch     the siblings of q leaves: a gather;
//   sylow_poseidon_merkle_root_batch / _verify_batch   the walk of q paths, `depth` dependent hashes each.
// ONE round body in two shapes with identical words.  NARROW: a lane per permutation, the state in registers, the rounds a rolled loop, the
// round constants and M read through wave-uniform pointers.  WIDE: a lane per state element in a group of group_lanes(t) lanes of a
// wavefront; lane i does its own S-box and row i of the mix and gets the other elements by shuffles.  Canonical arithmetic only: the S-box
// is fr_mul three times, a row of the mix is t calls of mul_acc and one fr_reduce_wide.  Geometry and routes: poseidon_plan.hpp -- nothing
// here decides one.
#include "host.hpp"
#include "bn254_fr_acc.hpp"
#include "bn254_fr_dev.hpp"
#include "poseidon_plan.hpp"
#include "../../include/sylow_poseidon.h"

#include <vector>

namespace pos {
using namespace poseidon_plan;
static_assert(POS_BLOCK == BLOCK, "the kernels run blocks of BLOCK lanes");
static_assert(SYLOW_POSEIDON_T_MIN == T_MIN && SYLOW_POSEIDON_T_MAX == T_MAX && SYLOW_POSEIDON_DEPTH_MAX == DEPTH_MAX, "the header's bounds are the plan's");
// THE ACCUMULATOR AT t = 17.  mul_acc states its bound for 16 terms; a row of the mix adds t <= 17 products of canonical values to a zeroed
// accumulator: 17 (r - 1)^2 + (r - 1) < 2^512 (r^2 < 0.58 2^508; tests/test_poseidon_model.py checks the integers), so the 16 limbs hold the
// sum, the top limb takes the last carry without a carry out, and fr_reduce_wide takes any value below 2^512.  A column still has at most 8
// products and one limb of acc.
static_assert(T_MAX <= 17, "17 r^2 + r < 2^512 is the bound the mix relies on");

// element e of a parameter table: 4 consecutive words
BN_DEV Fp tab_elem(const u64* tab, size_t e) {
  const u64* p = tab + FR_WORDS * e;
  Fp r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const u64 w = p[k];
    r.v[2 * k] = (u32)w;
    r.v[2 * k + 1] = (u32)(w >> 32);
  }
  return r;
}
BN_DEV Fp elem(const u64* a, size_t n, size_t k) { return fr_reduce_plain(load_plain(a, n, k, 0)); }
BN_DEV Fp sbox(const Fp& x) {
  const Fp x2 = fr_mul(x, x), x4 = fr_mul(x2, x2);
  return fr_mul(x4, x);
}

// ---- the narrow body: every index into the state is a constant, so the state stays in registers ---------------------------------------------
template <int T> BN_DEV void permute_narrow(Fp (&s)[T], const u64* __restrict__ tab) {
  constexpr int RP = partial_rounds(T), R = rounds(T);
  const u64* M = tab + FR_WORDS * matrix_elem(T);
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    const u64* c = tab + FR_WORDS * (size_t)T * (size_t)r;
#pragma unroll
    for (int i = 0; i < T; ++i) s[i] = fr_add(s[i], tab_elem(c, i));
    s[0] = sbox(s[0]);
    if (r < FULL_HALF || r >= FULL_HALF + RP) {                // wave-uniform
#pragma unroll
      for (int i = 1; i < T; ++i) s[i] = sbox(s[i]);
    }
    Fp o[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
      u32 acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < T; ++j) mul_acc(acc, tab_elem(M, (size_t)i * T + j), s[j]);      // T <= 17 terms: the bound above
      o[i] = fr_reduce_wide(acc);
    }
#pragma unroll
    for (int i = 0; i < T; ++i) s[i] = o[i];
  }
}

// ---- the wide body: this lane holds element i of the state of the group whose first lane of the wavefront is `base`.  EVERY lane of the
// wavefront calls it (the shuffles sit in uniform control flow): an idle lane of a group brings i = t - 1 and any value, and a group
// without an item brings zeros; neither is read by a lane that stores -------------------------------------------------------------------------
BN_DEV Fp shfl_fp(const Fp& a, int lane) {
  Fp r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = (u32)__shfl((int)a.v[k], lane);
  return r;
}
BN_DEV Fp permute_wide(Fp s, int i, int base, int t, const u64* __restrict__ tab) {
  const int rp = partial_rounds(t), R = rounds(t);
  const u64* M = tab + FR_WORDS * matrix_elem(t);
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    s = fr_add(s, tab_elem(tab, (size_t)t * r + i));
    if (i == 0 || r < FULL_HALF || r >= FULL_HALF + rp) s = sbox(s);
    u32 acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (int j = 0; j < t; ++j) mul_acc(acc, tab_elem(M, (size_t)i * t + j), shfl_fp(s, base + j));   // t <= 17 terms: the bound above
    s = fr_reduce_wide(acc);
  }
  return s;
}
// the lane's place in its group
struct Lane {
  int i, base, group;                            // element index, first lane of the group in the wavefront, group index in the block
};
BN_DEV Lane wide_lane(int t) {
  const int g = group_lanes(t), i = (int)threadIdx.x % g;
  return Lane{i, ((int)threadIdx.x % POS_WAVE) - i, (int)threadIdx.x / g};
}

// ---- permutations and hashes.  hash = 0: state [t][4][n] -> out [t][4][n].  hash = 1: [init or 0, in [t - 1][4][n]] -> element 0, out [4][n] ---
template <int T> __global__ void __launch_bounds__(BLOCK) k_pos_narrow(const u64* __restrict__ tab, const u64* in, const u64* init, int hash, size_t n, u64* out) {
#pragma unroll 1
  for (size_t it = TID; it < n; it += (size_t)gridDim.x * BLOCK) {
    Fp s[T];
    s[0] = hash ? (init ? elem(init, n, it) : fr_zero()) : elem(in, n, it);
#pragma unroll
    for (int i = 1; i < T; ++i) s[i] = elem(in + FR_WORDS * n * (size_t)(hash ? i - 1 : i), n, it);
    permute_narrow<T>(s, tab);
    store_plain(out, n, it, 0, s[0]);
    if (!hash) {
#pragma unroll
      for (int i = 1; i < T; ++i) store_plain(out + FR_WORDS * n * (size_t)i, n, it, 0, s[i]);
    }
  }
}
__global__ void __launch_bounds__(BLOCK) k_pos_wide(const u64* __restrict__ tab, int t, const u64* in, const u64* init, int hash, size_t n, u64* out) {
  const Lane l = wide_lane(t);
  const size_t gpb = (size_t)groups_per_block(t), n_tiles = tiles(t, n, ROUTE_WIDE);
#pragma unroll 1
  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {          // block-uniform: every lane of a wavefront walks the same tiles
    const size_t it = tile * gpb + (size_t)l.group;
    const bool live = it < n && l.i < t;                                        // an idle lane of a group and a group past n load and store nothing
    Fp s = fr_zero();
    if (live) {
      if (!hash) s = elem(in + FR_WORDS * n * (size_t)l.i, n, it);
      else if (l.i > 0) s = elem(in + FR_WORDS * n * (size_t)(l.i - 1), n, it);
      else if (init) s = elem(init, n, it);
    }
    s = permute_wide(s, l.i < t ? l.i : t - 1, l.base, t, tab);
    if (live && (!hash || l.i == 0)) store_plain(out + (hash ? 0 : FR_WORDS * n * (size_t)l.i), n, it, 0, s);
  }
}

// ---- a level of m trees.  A level is read and written through a Plane: word w of node k of tree j at p[j tree + w word + off + k] -----------
struct Plane {
  u64* p;
  size_t tree, word, off;
};
BN_DEV Fp plane_get(const Plane& a, size_t j, size_t k) {
  const u64* b = a.p + j * a.tree + a.off + k;
  Fp r;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const u64 x = b[(size_t)w * a.word];
    r.v[2 * w] = (u32)x;
    r.v[2 * w + 1] = (u32)(x >> 32);
  }
  return fr_reduce_plain(r);
}
BN_DEV void plane_put(const Plane& a, size_t j, size_t k, const Fp& v) {
  u64* b = a.p + j * a.tree + a.off + k;
#pragma unroll
  for (int w = 0; w < 4; ++w) b[(size_t)w * a.word] = (u64)v.v[2 * w] | ((u64)v.v[2 * w + 1] << 32);
}
// item (tree j, node k) of a level of `nodes` nodes: dst(j, k) = hash([src(j, 2 k), src(j, 2 k + 1)]); root_out [4][m] (or NULL) takes the
// same value, on the level that has one node
__global__ void __launch_bounds__(BLOCK) k_pos_level_narrow(const u64* __restrict__ tab, Plane src, Plane dst, size_t nodes, size_t items, u64* root_out, size_t m) {
#pragma unroll 1
  for (size_t it = TID; it < items; it += (size_t)gridDim.x * BLOCK) {
    const size_t j = it / nodes, k = it % nodes;
    Fp s[MERKLE_T] = {fr_zero(), plane_get(src, j, 2 * k), plane_get(src, j, 2 * k + 1)};
    permute_narrow<MERKLE_T>(s, tab);
    plane_put(dst, j, k, s[0]);
    if (root_out) store_plain(root_out, m, j, 0, s[0]);
  }
}
__global__ void __launch_bounds__(BLOCK) k_pos_level_wide(const u64* __restrict__ tab, Plane src, Plane dst, size_t nodes, size_t items, u64* root_out, size_t m) {
  const Lane l = wide_lane(MERKLE_T);
  const size_t gpb = (size_t)groups_per_block(MERKLE_T), n_tiles = tiles(MERKLE_T, items, ROUTE_WIDE);
#pragma unroll 1
  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const size_t it = tile * gpb + (size_t)l.group;
    const bool live = it < items;
    const size_t j = live ? it / nodes : 0, k = live ? it % nodes : 0;
    Fp s = fr_zero();
    if (live && (l.i == 1 || l.i == 2)) s = plane_get(src, j, 2 * k + (size_t)(l.i - 1));
    s = permute_wide(s, l.i < MERKLE_T ? l.i : MERKLE_T - 1, l.base, MERKLE_T, tab);
    if (live && l.i == 0) {
      plane_put(dst, j, k, s);
      if (root_out) store_plain(root_out, m, j, 0, s);
    }
  }
}

// ---- the siblings of q leaves: lane (level k, query i) copies one node, mod r.  leaves [m][4][n], nodes [m][4][n - 1].  A query whose tree
// or index is out of range reads nothing, gets a zero row and status bit 0 -----------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) k_pos_open(const u64* leaves, const u64* nodes, int depth, size_t m, const u64* tree, const u64* index, size_t q, size_t items,
                                                    u64* sib, uint8_t* status) {
  const size_t n = elems(depth);
#pragma unroll 1
  for (size_t it = TID; it < items; it += (size_t)gridDim.x * BLOCK) {
    const size_t k = it / q, i = it % q;
    const u64 j = tree[i], x = index[i];
    const bool bad = j >= (u64)m || x >= (u64)n;
    Fp v = fr_zero();
    if (!bad) {
      const size_t pos = (size_t)(x >> k) ^ 1;
      v = k == 0 ? elem(leaves + (size_t)j * FR_WORDS * n, n, pos) : elem(nodes + (size_t)j * FR_WORDS * (n - 1), n - 1, level_offset(depth, (int)k) + pos);
    }
    store_plain(sib + k * FR_WORDS * q, q, i, 0, v);
    if (k == 0) status[i] = bad ? STATUS_OUT_OF_RANGE : 0;
  }
}

// ---- the walk of q paths: cur = leaf; level k: cur = hash(bit k of index ? [sibling_k, cur] : [cur, sibling_k]).  root_out [4][q] (or NULL)
// takes the root, zeros where the index is out of range; ok [q] (or NULL) takes [cur == roots[n_roots == 1 ? 0 : i] mod r], 0 where the status
// is not 0 -------------------------------------------------------------------------------------------------------------------------------------
BN_DEV void path_close(const Fp& cur, bool bad, size_t i, size_t q, const u64* roots, size_t n_roots, u64* root_out, uint8_t* ok, uint8_t* status) {
  if (root_out) store_plain(root_out, q, i, 0, bad ? fr_zero() : cur);
  if (ok) ok[i] = !bad && fp_eq(cur, elem(roots, n_roots, n_roots == 1 ? 0 : i)) ? 1 : 0;
  status[i] = bad ? STATUS_OUT_OF_RANGE : 0;
}
__global__ void __launch_bounds__(BLOCK) k_pos_path_narrow(const u64* __restrict__ tab, const u64* leaf, const u64* index, const u64* sib, int depth, size_t q,
                                                           const u64* roots, size_t n_roots, u64* root_out, uint8_t* ok, uint8_t* status) {
#pragma unroll 1
  for (size_t i = TID; i < q; i += (size_t)gridDim.x * BLOCK) {
    const u64 x = index[i];
    Fp cur = elem(leaf, q, i);
#pragma unroll 1
    for (int k = 0; k < depth; ++k) {
      const Fp sb = elem(sib + (size_t)k * FR_WORDS * q, q, i);
      const bool right = (x >> k) & 1;
      Fp s[MERKLE_T] = {fr_zero(), right ? sb : cur, right ? cur : sb};
      permute_narrow<MERKLE_T>(s, tab);
      cur = s[0];
    }
    path_close(cur, x >= (u64)elems(depth), i, q, roots, n_roots, root_out, ok, status);
  }
}
__global__ void __launch_bounds__(BLOCK) k_pos_path_wide(const u64* __restrict__ tab, const u64* leaf, const u64* index, const u64* sib, int depth, size_t q,
                                                         const u64* roots, size_t n_roots, u64* root_out, uint8_t* ok, uint8_t* status) {
  const Lane l = wide_lane(MERKLE_T);
  const size_t gpb = (size_t)groups_per_block(MERKLE_T), n_tiles = tiles(MERKLE_T, q, ROUTE_WIDE);
#pragma unroll 1
  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const size_t i = tile * gpb + (size_t)l.group;
    const bool live = i < q;
    const u64 x = live ? index[i] : 0;
    Fp cur = live ? elem(leaf, q, i) : fr_zero();                               // every lane of the group holds the running node
#pragma unroll 1
    for (int k = 0; k < depth; ++k) {
      const Fp sb = live ? elem(sib + (size_t)k * FR_WORDS * q, q, i) : fr_zero();
      const bool right = (x >> k) & 1;
      Fp s = l.i == 1 ? (right ? sb : cur) : l.i == 2 ? (right ? cur : sb) : fr_zero();
      s = permute_wide(s, l.i < MERKLE_T ? l.i : MERKLE_T - 1, l.base, MERKLE_T, tab);
      cur = shfl_fp(s, l.base);
    }
    if (live && l.i == 0) path_close(cur, x >= (u64)elems(depth), i, q, roots, n_roots, root_out, ok, status);
  }
}

// M[i][j] = (xs[i] + ys[j])^-1 in place over the t^2 sums the host uploaded; count elements of 4 consecutive words
__global__ void __launch_bounds__(BLOCK) k_pos_invert(u64* sums, size_t count) {
  const size_t e = TID;
  if (e >= count) return;
  const Fp v = fr_inv(tab_elem(sums, e));
#pragma unroll
  for (int k = 0; k < 4; ++k) sums[FR_WORDS * e + k] = (u64)v.v[2 * k] | ((u64)v.v[2 * k + 1] << 32);
}

// ---- launches --------------------------------------------------------------------------------------------------------------------------------
static unsigned blocks_for(int t, size_t items, int route, long long max_blocks) { return (unsigned)grid(tiles(t, items, route), max_blocks); }

template <int T> static void narrow_launch(int t, unsigned blocks, hipStream_t st, const u64* tab, const u64* in, const u64* init, int hash, size_t n, u64* out) {
  if constexpr (T >= T_MIN) {
    if (t == T) k_pos_narrow<T><<<dim3(blocks), dim3(BLOCK), 0, st>>>(tab, in, init, hash, n, out);
    else narrow_launch<T - 1>(t, blocks, st, tab, in, init, hash, n, out);
  }
}
// n permutations (hash = 0) or hashes (hash = 1) of width t on the route the plan chooses
static int32_t run(const u64* tab, int t, const u64* in, const u64* init, int hash, size_t n, int route_pin, long long max_blocks, u64* out, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const int route = choose_route(t, n, route_pin, -1);
  const unsigned blocks = blocks_for(t, n, route, max_blocks);
  if (route == ROUTE_WIDE) k_pos_wide<<<dim3(blocks), dim3(BLOCK), 0, st>>>(tab, t, in, init, hash, n, out);
  else narrow_launch<NARROW_T_MAX>(t, blocks, st, tab, in, init, hash, n, out);
  LAUNCHED();
}
static int32_t path_run(const u64* tab, const u64* leaf, const u64* index, const u64* sib, int depth, size_t q, const u64* roots, size_t n_roots, int route_pin,
                        long long max_blocks, u64* root_out, uint8_t* ok, uint8_t* status, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const int route = choose_route(MERKLE_T, q, route_pin, -1);
  const unsigned blocks = blocks_for(MERKLE_T, q, route, max_blocks);
  if (route == ROUTE_WIDE) k_pos_path_wide<<<dim3(blocks), dim3(BLOCK), 0, st>>>(tab, leaf, index, sib, depth, q, roots, n_roots, root_out, ok, status);
  else k_pos_path_narrow<<<dim3(blocks), dim3(BLOCK), 0, st>>>(tab, leaf, index, sib, depth, q, roots, n_roots, root_out, ok, status);
  LAUNCHED();
}
static_assert(narrow_ok(MERKLE_T), "the trees have both routes");
}  // namespace pos

extern "C" {
int32_t sylow_poseidon_table_words(int32_t t) { return poseidon_plan::width_ok(t) ? (int32_t)poseidon_plan::table_words(t) : 0; }

int32_t sylow_poseidon_prepare(int32_t t, uint64_t* table_out, void* stream) {
  using namespace poseidon_plan;
  ARGCHK(width_ok(t) && table_out);
  const hipStream_t st = (hipStream_t)stream;
  const poseidon_params::Draws d = poseidon_params::draw(t);
  std::vector<uint64_t> host(table_words(t));
  size_t at = 0;
  for (const auto* part : {&d.constants, &d.sums})
    for (const auto& v : *part)
      for (int k = 0; k < 4; ++k) host[at++] = v.w[k];
  HIPCHK(hipMemcpyAsync(table_out, host.data(), table_bytes(t), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));                                             // `host` leaves with this frame: the one synchronisation of the unit
  const size_t cells = (size_t)t * (size_t)t;
  pos::k_pos_invert<<<dim3((unsigned)ceil_div(cells, POS_BLOCK)), dim3(BLOCK), 0, st>>>(table_out + FR_WORDS * matrix_elem(t), cells);
  LAUNCHED();
}

int32_t sylow_poseidon_permute_batch_tuned(const uint64_t* table, int32_t t, const uint64_t* state, size_t n, int32_t route, int64_t max_blocks, uint64_t* out,
                                           void* stream) {
  using namespace poseidon_plan;
  ARGCHK(width_ok(t) && route_ok(route) && max_blocks_ok(max_blocks));
  if (!n) return SYLOW_HIP_OK;
  ARGCHK(table && state && out && state_bytes(t, n) != SAT);
  const host::Range in[2] = {{(uintptr_t)table, table_bytes(t)}, {(uintptr_t)state, state_bytes(t, n)}}, outs[1] = {{(uintptr_t)out, state_bytes(t, n)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  return pos::run(table, t, state, nullptr, 0, n, route, max_blocks, out, stream);
}
int32_t sylow_poseidon_permute_batch(const uint64_t* table, int32_t t, const uint64_t* state, size_t n, uint64_t* out, void* stream) {
  return sylow_poseidon_permute_batch_tuned(table, t, state, n, -1, -1, out, stream);
}

int32_t sylow_poseidon_hash_batch_tuned(const uint64_t* table, int32_t k, const uint64_t* inputs, const uint64_t* init, size_t n, int32_t route, int64_t max_blocks,
                                        uint64_t* out, void* stream) {
  using namespace poseidon_plan;
  ARGCHK(inputs_ok(k) && route_ok(route) && max_blocks_ok(max_blocks));
  if (!n) return SYLOW_HIP_OK;
  ARGCHK(table && inputs && out && state_bytes(k, n) != SAT);
  const host::Range in[3] = {{(uintptr_t)table, table_bytes(k + 1)}, {(uintptr_t)inputs, state_bytes(k, n)}, {(uintptr_t)init, fr_bytes(n)}},
                    outs[1] = {{(uintptr_t)out, fr_bytes(n)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  return pos::run(table, k + 1, inputs, init, 1, n, route, max_blocks, out, stream);
}
int32_t sylow_poseidon_hash_batch(const uint64_t* table, int32_t k, const uint64_t* inputs, const uint64_t* init, size_t n, uint64_t* out, void* stream) {
  return sylow_poseidon_hash_batch_tuned(table, k, inputs, init, n, -1, -1, out, stream);
}

int32_t sylow_poseidon_merkle_build_batch_tuned(const uint64_t* table, const uint64_t* leaves, int32_t depth, size_t m, int64_t wide_max, int64_t max_blocks,
                                                uint64_t* nodes_out, uint64_t* root_out, void* stream) {
  using namespace poseidon_plan;
  ARGCHK(depth_ok(depth) && max_blocks_ok(max_blocks));
  if (!m) return SYLOW_HIP_OK;
  ARGCHK(table && leaves && nodes_out && leaves_bytes(depth, m) != SAT);
  const host::Range in[2] = {{(uintptr_t)table, table_bytes(MERKLE_T)}, {(uintptr_t)leaves, leaves_bytes(depth, m)}},
                    outs[2] = {{(uintptr_t)nodes_out, nodes_bytes(depth, m)}, {(uintptr_t)root_out, fr_bytes(m)}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = elems(depth), stride = node_count(depth);
  for (int k = 1; k <= depth; ++k) {                                            // one launch per level over all m trees
    const pos::Plane src = k == 1 ? pos::Plane{const_cast<uint64_t*>(leaves), FR_WORDS * n, n, 0} : pos::Plane{nodes_out, FR_WORDS * stride, stride, level_offset(depth, k - 1)};
    const pos::Plane dst = {nodes_out, FR_WORDS * stride, stride, level_offset(depth, k)};
    const size_t nodes = level_nodes(depth, k), items = level_items(depth, k, m);
    const int route = choose_route(MERKLE_T, items, -1, wide_max);             // each level by its own item count
    const unsigned blocks = pos::blocks_for(MERKLE_T, items, route, max_blocks);
    uint64_t* const ro = k == depth ? root_out : nullptr;
    if (route == ROUTE_WIDE) pos::k_pos_level_wide<<<dim3(blocks), dim3(BLOCK), 0, st>>>(table, src, dst, nodes, items, ro, m);
    else pos::k_pos_level_narrow<<<dim3(blocks), dim3(BLOCK), 0, st>>>(table, src, dst, nodes, items, ro, m);
  }
  LAUNCHED();
}
int32_t sylow_poseidon_merkle_build_batch(const uint64_t* table, const uint64_t* leaves, int32_t depth, size_t m, uint64_t* nodes_out, uint64_t* root_out,
                                          void* stream) {
  return sylow_poseidon_merkle_build_batch_tuned(table, leaves, depth, m, -1, -1, nodes_out, root_out, stream);
}

int32_t sylow_poseidon_merkle_open_batch(const uint64_t* leaves, const uint64_t* nodes, int32_t depth, size_t m, const uint64_t* tree, const uint64_t* index,
                                         size_t q, uint64_t* siblings_out, uint8_t* status, void* stream) {
  using namespace poseidon_plan;
  ARGCHK(depth_ok(depth));
  if (!q) return SYLOW_HIP_OK;
  ARGCHK(tree && index && siblings_out && status && (!m || (leaves && nodes)));
  ARGCHK(leaves_bytes(depth, m) != SAT && path_bytes(depth, q) != SAT);
  const host::Range in[4] = {{(uintptr_t)(m ? leaves : nullptr), leaves_bytes(depth, m)}, {(uintptr_t)(m ? nodes : nullptr), nodes_bytes(depth, m)},
                             {(uintptr_t)tree, index_bytes(q)}, {(uintptr_t)index, index_bytes(q)}},
                    outs[2] = {{(uintptr_t)siblings_out, path_bytes(depth, q)}, {(uintptr_t)status, q}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  const size_t items = mul_sat((size_t)depth, q);
  pos::k_pos_open<<<dim3((unsigned)grid(ceil_div(items, POS_BLOCK), -1)), dim3(BLOCK), 0, (hipStream_t)stream>>>(leaves, nodes, depth, m, tree, index, q, items,
                                                                                                                 siblings_out, status);
  LAUNCHED();
}

int32_t sylow_poseidon_merkle_root_batch(const uint64_t* table, const uint64_t* leaf, const uint64_t* index, const uint64_t* siblings, int32_t depth, size_t q,
                                         uint64_t* root_out, uint8_t* status, void* stream) {
  using namespace poseidon_plan;
  ARGCHK(depth_ok(depth));
  if (!q) return SYLOW_HIP_OK;
  ARGCHK(table && leaf && index && siblings && root_out && status && path_bytes(depth, q) != SAT);
  const host::Range in[4] = {{(uintptr_t)table, table_bytes(MERKLE_T)}, {(uintptr_t)leaf, fr_bytes(q)}, {(uintptr_t)index, index_bytes(q)},
                             {(uintptr_t)siblings, path_bytes(depth, q)}},
                    outs[2] = {{(uintptr_t)root_out, fr_bytes(q)}, {(uintptr_t)status, q}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  return pos::path_run(table, leaf, index, siblings, depth, q, nullptr, 1, -1, -1, root_out, nullptr, status, stream);
}

int32_t sylow_poseidon_merkle_verify_batch_tuned(const uint64_t* table, const uint64_t* leaf, const uint64_t* index, const uint64_t* siblings, int32_t depth,
                                                 size_t q, const uint64_t* roots, size_t n_roots, int32_t route, int64_t max_blocks, uint8_t* ok, uint8_t* status,
                                                 void* stream) {
  using namespace poseidon_plan;
  ARGCHK(depth_ok(depth) && route_ok(route) && max_blocks_ok(max_blocks));
  if (!q) return SYLOW_HIP_OK;
  ARGCHK(n_roots_ok(n_roots, q));
  ARGCHK(table && leaf && index && siblings && roots && ok && status && path_bytes(depth, q) != SAT);
  const host::Range in[5] = {{(uintptr_t)table, table_bytes(MERKLE_T)}, {(uintptr_t)leaf, fr_bytes(q)}, {(uintptr_t)index, index_bytes(q)},
                             {(uintptr_t)siblings, path_bytes(depth, q)}, {(uintptr_t)roots, fr_bytes(n_roots)}},
                    outs[2] = {{(uintptr_t)ok, q}, {(uintptr_t)status, q}};
  ARGCHK(host::outputs_disjoint(in, outs, disjoint));
  return pos::path_run(table, leaf, index, siblings, depth, q, roots, n_roots, route, max_blocks, nullptr, ok, status, stream);
}
int32_t sylow_poseidon_merkle_verify_batch(const uint64_t* table, const uint64_t* leaf, const uint64_t* index, const uint64_t* siblings, int32_t depth, size_t q,
                                           const uint64_t* roots, size_t n_roots, uint8_t* ok, uint8_t* status, void* stream) {
  return sylow_poseidon_merkle_verify_batch_tuned(table, leaf, index, siblings, depth, q, roots, n_roots, -1, -1, ok, status, stream);
}
}  // extern "C"
