/*
 * sylow_poseidon.h -- C ABI of BATCHED POSEIDON OVER Fr AND OF POSEIDON MERKLE TREES (poseidon.hip; widths, routes, grids and the levels of a
 * tree in poseidon_plan.hpp; the parameter generator in poseidon_params.hpp).  It includes sylow_hip.h and shares its conventions (device
 * pointers, word-major struct-of-arrays, the `@shape` lines, stream-ordered calls, SYLOW_HIP_E_* return values) and adds nothing to it.  The
 * entry points live in the same libsylow_hip.so.
 *
 * WHY A HEADER AND A PREFIX OF ITS OWN.  The sets of sylow_hip_*, sylow_plonk_*, sylow_popen_* and sylow_pverify_* symbols are closed: the
 * tests pin every exported name of each prefix to its binding table.  So the hash gets the prefix sylow_poseidon_ and this header, a tenth
 * binding table, and NO SYMBOL UNDER AN OLDER PREFIX IS ADDED.
 *
 * THE INSTANCE is circomlib's / circomlibjs's, so hashes agree with deployed circuits:
 *   field Fr, S-box x^5, state width t = 2 .. 17 (1 .. 16 inputs), R_F = 8 full rounds (four before and four after the partial ones) and
 *   R_P = 56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68 partial rounds for t = 2 .. 17.
 *   A round: add the round constants; the S-box on every element (full round) or on element 0 only (partial round); then the mix
 *   new[i] = sum_j M[i][j] state[j].  M IS NOT SYMMETRIC.
 *   hash(in_0 .. in_(k-1)) = element 0 of the permutation of [init, in_0, .., in_(k-1)], t = k + 1, init = 0 unless the caller gives one
 *   (circomlibjs's initState: a caller chains longer inputs through it).
 *   The round constants and M come from the Poseidon paper's Grain LFSR (seed fields 1, 0, 254, t, R_F, R_P, thirty ones; poseidon_params.hpp
 *   states every step), M[i][j] = (xs[i] + ys[j])^-1 from the first draw of 2 t distinct values.  KNOWN ANSWERS: published circomlib values
 *   pin t = 2, 3, 4, 5, 7 and 17 (tests/golden/poseidon_kats.json).  THE OTHER WIDTHS REST ON THE SAME GENERATOR AND HAVE NO EXTERNAL KNOWN
 *   ANSWER OF THEIR OWN.
 *
 * THE LIBRARY KEEPS NO HIDDEN STATE: the caller owns the parameter table of a width (sylow_poseidon_prepare) and every other call takes it.
 * A TABLE PREPARED FOR ANOTHER t IS A CONTRACT VIOLATION: the call reads table_words(t) words of it and computes another function.  The
 * Merkle calls take the t = 3 table.
 *
 * Conventions:
 *   Fr arrays:   word-major struct-of-arrays [4][n]; a batch of states [t][4][n]: element i of item j at words (4 i + w) n + j.
 *   scalars:     any 256-bit words, taken mod r; outputs canonical.
 *   routes:      NARROW (0), a lane per permutation; WIDE (1), a lane per state element.  THE WORDS DEPEND ON NEITHER THE ROUTE NOR A PIN.  A
 *                width above the narrow route's limit (poseidon_plan.hpp: NARROW_T_MAX) runs wide whatever the pin.
 *   status:      [q] bytes.  Bit 0 (0x01): tree >= m or index >= 2^depth.  No other bit is defined.
 *   calls:       stream-ordered; THE HOT CALLS NEVER SYNCHRONISE and lease no scratch (nothing here needs any); sylow_poseidon_prepare
 *                SYNCHRONISES THE STREAM ONCE, after uploading what the host drew.  n = 0, m = 0 or q = 0: nothing is launched.
 *                SYLOW_HIP_E_ARG, nothing enqueued and nothing written, for: NULL where an array is required, t outside 2 .. 17 (k outside
 *                1 .. 16), depth outside 1 .. 28, n_roots neither 1 nor q, a route other than < 0, 0, 1, max_blocks = 0, and any output whose
 *                bytes overlap an input's or another output's.
 */
#ifndef SYLOW_POSEIDON_H
#define SYLOW_POSEIDON_H

#include "sylow_hip.h"

#define SYLOW_POSEIDON_T_MIN 2
#define SYLOW_POSEIDON_T_MAX 17
#define SYLOW_POSEIDON_DEPTH_MAX 28

#ifdef __cplusplus
extern "C" {
#endif

/* The u64 words of the parameter table of width t: 4 ((8 + R_P) t + t t); 0 for a t outside 2 .. 17.  Host arithmetic. */
int32_t sylow_poseidon_table_words(int32_t t);

/* Fills the caller's device table: the (8 + R_P) t round constants, round-major, then M row by row, canonical, AN ELEMENT AS 4 CONSECUTIVE
 * WORDS (every lane reads the same element at a time).  The Grain generator runs on the host; the t^2 sums xs[i] + ys[j] are uploaded with the
 * constants, THE STREAM IS SYNCHRONISED ONCE, and one launch inverts the sums in place (a^(r-2), as sylow_hip_fr_inv_batch). */
/* @shape table_out=u64[*] */
int32_t sylow_poseidon_prepare(int32_t t, uint64_t* table_out, void* stream);

/* out = the permutation of n states of width t: state and out [t][4][n]. */
/* @shape table=u64[*] state=u64[4*t*n] out=u64[4*t*n] */
int32_t sylow_poseidon_permute_batch(const uint64_t* table, int32_t t, const uint64_t* state, size_t n, uint64_t* out, void* stream);
/* The same with the plan pinned.  route: < 0 the default (wide up to a measured n, narrow beyond), 0 narrow, 1 wide.  max_blocks: the blocks
 * of the launch (>= 1, < 0 = the default); fewer blocks walk the batch with a grid stride.  The words depend on neither. */
/* @shape table=u64[*] state=u64[4*t*n] out=u64[4*t*n] */
int32_t sylow_poseidon_permute_batch_tuned(const uint64_t* table, int32_t t, const uint64_t* state, size_t n, int32_t route, int64_t max_blocks,
                                           uint64_t* out, void* stream);

/* out [4][n] = hash of the k inputs of every item under the table of t = k + 1: inputs [k][4][n]; init [4][n] or NULL (zeros). */
/* @shape table=u64[*] inputs=u64[4*k*n] init=u64[4*n]? out=u64[4*n] */
int32_t sylow_poseidon_hash_batch(const uint64_t* table, int32_t k, const uint64_t* inputs, const uint64_t* init, size_t n, uint64_t* out, void* stream);
/* @shape table=u64[*] inputs=u64[4*k*n] init=u64[4*n]? out=u64[4*n] */
int32_t sylow_poseidon_hash_batch_tuned(const uint64_t* table, int32_t k, const uint64_t* inputs, const uint64_t* init, size_t n, int32_t route,
                                        int64_t max_blocks, uint64_t* out, void* stream);

/* m binary trees of n = 2^depth leaves, node = hash([left, right]) under the t = 3 table.  leaves [m][4][n]; nodes_out [m][4][n - 1] holds
 * levels 1 .. depth one after another, level k (n / 2^k nodes) starting at n - 2^(depth - k + 1), THE ROOT THE LAST ELEMENT; root_out [4][m]
 * or NULL takes the roots as well.  ONE LAUNCH PER LEVEL over all m trees, items (tree, node); each level picks its route by its own item
 * count. */
/* @shape table=u64[*] leaves=u64[4*m*2**depth] nodes_out=u64[4*m*(2**depth-1)] root_out=u64[4*m]? */
int32_t sylow_poseidon_merkle_build_batch(const uint64_t* table, const uint64_t* leaves, int32_t depth, size_t m, uint64_t* nodes_out, uint64_t* root_out,
                                          void* stream);
/* The same with the plan pinned.  wide_max: the item count up to which a level runs wide (< 0 = the default; 0: every level narrow). */
/* @shape table=u64[*] leaves=u64[4*m*2**depth] nodes_out=u64[4*m*(2**depth-1)] root_out=u64[4*m]? */
int32_t sylow_poseidon_merkle_build_batch_tuned(const uint64_t* table, const uint64_t* leaves, int32_t depth, size_t m, int64_t wide_max, int64_t max_blocks,
                                                uint64_t* nodes_out, uint64_t* root_out, void* stream);

/* The siblings of q leaves: query i names leaf index[i] of tree tree[i]; siblings_out [depth][4][q], level 0 (a leaf) first, canonical;
 * status [q].  A gather.  tree >= m or index >= n: status bit 0, the row is zeros, and NOTHING IS READ OUTSIDE THE ARRAYS, whatever the
 * index arrays hold.  leaves and nodes may be NULL when m = 0. */
/* @shape leaves=u64[4*m*2**depth] nodes=u64[4*m*(2**depth-1)] tree=u64[q] index=u64[q] siblings_out=u64[4*depth*q] status=u8[q] */
int32_t sylow_poseidon_merkle_open_batch(const uint64_t* leaves, const uint64_t* nodes, int32_t depth, size_t m, const uint64_t* tree, const uint64_t* index,
                                         size_t q, uint64_t* siblings_out, uint8_t* status, void* stream);

/* root_out [4][q]: the root every path leads to.  leaf [4][q], siblings [depth][4][q]; bit k of index set: the node is the RIGHT child at
 * level k.  `depth` dependent hashes per query.  index >= 2^depth: status bit 0 and a zero row. */
/* @shape table=u64[*] leaf=u64[4*q] index=u64[q] siblings=u64[4*depth*q] root_out=u64[4*q] status=u8[q] */
int32_t sylow_poseidon_merkle_root_batch(const uint64_t* table, const uint64_t* leaf, const uint64_t* index, const uint64_t* siblings, int32_t depth, size_t q,
                                         uint64_t* root_out, uint8_t* status, void* stream);

/* ok [q]: the recomputed root equals roots[n_roots == 1 ? 0 : i] mod r; roots [4][n_roots], n_roots = 1 or q.  ok IS 0 WHEREVER status != 0. */
/* @shape table=u64[*] leaf=u64[4*q] index=u64[q] siblings=u64[4*depth*q] roots=u64[4*n_roots] ok=u8[q] status=u8[q] */
int32_t sylow_poseidon_merkle_verify_batch(const uint64_t* table, const uint64_t* leaf, const uint64_t* index, const uint64_t* siblings, int32_t depth,
                                           size_t q, const uint64_t* roots, size_t n_roots, uint8_t* ok, uint8_t* status, void* stream);
/* The same with the plan pinned: route and max_blocks as for the hash. */
/* @shape table=u64[*] leaf=u64[4*q] index=u64[q] siblings=u64[4*depth*q] roots=u64[4*n_roots] ok=u8[q] status=u8[q] */
int32_t sylow_poseidon_merkle_verify_batch_tuned(const uint64_t* table, const uint64_t* leaf, const uint64_t* index, const uint64_t* siblings, int32_t depth,
                                                 size_t q, const uint64_t* roots, size_t n_roots, int32_t route, int64_t max_blocks, uint8_t* ok,
                                                 uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_POSEIDON_H */
