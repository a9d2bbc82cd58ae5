/*
 * sylow_hip_fr_scan.h -- C ABI of the SCANS OVER Fr -- running sums and running products of rows, and of a ratio num_i / den_i formed on the
 * way -- and of the running product every PLONK-family prover needs between its wire commitments and its quotient: the polynomial z of the
 * copy-constraint argument (fr_scan.hip; items, tiles, grids and scratch in fr_scan_plan.hpp).  An extension of sylow_hip.h: it includes
 * that header, shares its conventions (device pointers, word-major struct-of-arrays, the `@shape` lines, stream-ordered calls,
 * SYLOW_HIP_E_* return values) and adds nothing to it.  The entry points live in the same libsylow_hip.so.
 *
 * With w the n-th root of sylow_hip_fr_ntt_batch for n = 2^log_n, W wire columns w_j, the identity columns k_j w^i (k_j = shifts_j: coset
 * representatives the caller chooses, e.g. 1, 5, 7, ...), the permutation columns sigma_j and the challenges beta and gamma:
 *     z_0 = 1,     z_(i+1) = z_i  prod_j (w_j(i) + beta k_j w^i + gamma)  /  prod_j (w_j(i) + beta sigma_j(i) + gamma)
 * The copy constraints hold exactly when z closes: z_n = 1 (up to the soundness error of beta and gamma).  plookup and halo2 lookups are
 * the same running product of another ratio; logUp is the running SUM of a ratio: both are sylow_hip_fr_ratio_scan_batch.
 * SOUNDNESS: THE LIBRARY DRAWS NO CHALLENGE.  beta and gamma MUST BE DRAWN AFTER THE WIRE COMMITMENTS ARE FIXED (Fiat-Shamir over the
 * transcript that holds them); a prover who knows them before it chooses its wires can make z close for wires that break the constraints.
 *
 * Conventions (the Fr blocks of sylow_hip.h):
 *   rows:        [m][4][len], row j an Fr SoA array of stride len, the rows one after another.  Scalars [4][count].  Inputs are ANY 256-bit
 *                words, taken mod r; outputs are canonical.
 *   op:          0 = sum (identity 0), 1 = product (identity 1).
 *   inverses:    the library's inv(0) = 0.  A denominator that is 0 mod r enters the shared inversion as 1 and does not disturb its
 *                neighbours; its own term is 0, so a product row is 0 from the element after it on, and bit 0 of the row's status is set.
 *   status:      [m] bytes.  Bit 0: some den_i = 0 mod r in the row.  Bit 1 (the permutation entry alone): z_n != 1.  0 = the copy
 *                constraints hold.
 *   calls:       stream-ordered, no host synchronisation; scratch leased per call, summed in saturating arithmetic and refused before the
 *                lease.  m = 0: nothing is launched and nothing written.  SYLOW_HIP_E_ARG, nothing enqueued and nothing written, for: NULL
 *                where an array is required, len = 0, op or exclusive outside {0, 1}, log_n outside 0 .. 28, W outside
 *                1 .. SYLOW_HIP_PLONK_WIRES_MAX, max_blocks = 0, totals_tile = 0 or above 256, and any output whose bytes overlap an
 *                input's or another output's.
 *
 * The scan is three stream-ordered launches and NO BLOCK EVER WAITS FOR ANOTHER.  A block owns a chunk of 2048 elements of a row, 256
 * lanes of 8.  Phase 1: a lane folds its 8 elements, the block scans the 256 lane totals through LDS, the chunk-local scan goes to `out`
 * and the chunk's total to scratch.  Phase 2: one block per row walks the row's chunk totals, totals_tile at a time, carrying the running
 * value across the tiles, and leaves every chunk's prefix.  Phase 3: every element of a chunk after the first is combined with its chunk's
 * prefix.  A row of one chunk is done after phase 1.
 */
#ifndef SYLOW_HIP_FR_SCAN_H
#define SYLOW_HIP_FR_SCAN_H

#include "sylow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SYLOW_HIP_PLONK_WIRES_MAX 32

/* The scan of m rows of len elements.  exclusive = 0: out_j[k] = a_j[0] o .. o a_j[k].  exclusive = 1: out_j[k] = a_j[0] o .. o a_j[k-1],
 * the identity at k = 0.  total_out [4][m] (may be NULL): a_j[0] o .. o a_j[len-1], whatever `exclusive` is. */
/* @shape a=u64[4*len*m] out=u64[4*len*m] total_out=u64[4*m]? */
int32_t sylow_hip_fr_scan_batch(const uint64_t* a, size_t len, size_t m, int32_t op, int32_t exclusive, uint64_t* out, uint64_t* total_out, void* stream);
/* The same with the plan pinned.  max_blocks: the blocks of a launch of this unit's kernels (>= 1, < 0 = the default).  totals_tile: the
 * chunk totals phase 2 scans per step (1 .. 256, < 0 = the default).  The words depend on neither. */
/* @shape a=u64[4*len*m] out=u64[4*len*m] total_out=u64[4*m]? */
int32_t sylow_hip_fr_scan_batch_tuned(const uint64_t* a, size_t len, size_t m, int32_t op, int32_t exclusive, int64_t max_blocks, int32_t totals_tile,
                                      uint64_t* out, uint64_t* total_out, void* stream);

/* The scan of a ratio: t_i = num_i den_i^-1 (num NULL: every num_i = 1), and out is ALWAYS the exclusive scan of t: out_j[0] is the
 * identity and out_j[k] = t_0 o .. o t_(k-1).  total_out [4][m] (may be NULL): the value "out_j[len]", t_0 o .. o t_(len-1).  status [m].
 * Phase 1 fuses the shared inversion with the scan: the denominators of a chunk share ONE inversion as in sylow_hip_fr_batch_inv, the
 * ratios and their chunk-local scan are formed in registers, and the denominators are read twice: no array of inverses and no array of
 * ratios ever reaches memory. */
/* @shape num=u64[4*len*m]? den=u64[4*len*m] out=u64[4*len*m] total_out=u64[4*m]? status=u8[m] */
int32_t sylow_hip_fr_ratio_scan_batch(const uint64_t* num, const uint64_t* den, size_t len, size_t m, int32_t op, uint64_t* out, uint64_t* total_out,
                                      uint8_t* status, void* stream);
/* The same with the plan pinned, as sylow_hip_fr_scan_batch_tuned. */
/* @shape num=u64[4*len*m]? den=u64[4*len*m] out=u64[4*len*m] total_out=u64[4*m]? status=u8[m] */
int32_t sylow_hip_fr_ratio_scan_batch_tuned(const uint64_t* num, const uint64_t* den, size_t len, size_t m, int32_t op, int64_t max_blocks, int32_t totals_tile,
                                            uint64_t* out, uint64_t* total_out, uint8_t* status, void* stream);

/* The identity columns of the permutation argument: out [W][4][n], out_j[i] = shifts_j w^i, shifts [4][W].  sigma is these values
 * permuted: position (j, i) of sigma holds the identity value of the position the copy cycle sends it to. */
/* @shape shifts=u64[4*W] out=u64[4*2**log_n*W] */
int32_t sylow_hip_plonk_identity_batch(const uint64_t* shifts, int32_t log_n, int32_t W, uint64_t* out, void* stream);

/* z for m instances over ONE permutation.  wires [m][W][4][n]: column j of instance s at row s W + j.  sigma [W][4][n], shared by the
 * instances.  shifts [4][W].  beta and gamma [4][m], one pair per instance, DRAWN BY THE CALLER AFTER THE WIRE COMMITMENTS ARE FIXED.
 * z_out [m][4][n]: z_0 = 1 and z_(i+1) as above: the exclusive product scan of num_i / den_i.  total_out [4][m] (may be NULL): z_n.
 * status [m]: bit 0 a denominator was 0, bit 1 z_n != 1; 0 = the copy constraints hold.
 * In order: the table of the n / 2 roots; one launch that writes num_i and den_i, the products over the W columns, into scratch (w^i is
 * one load from the table: no power is formed per element); then the three phases of sylow_hip_fr_ratio_scan_batch. */
/* @shape wires=u64[4*2**log_n*W*m] sigma=u64[4*2**log_n*W] shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] z_out=u64[4*2**log_n*m] total_out=u64[4*m]? status=u8[m] */
int32_t sylow_hip_plonk_permutation_batch(const uint64_t* wires, const uint64_t* sigma, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma,
                                          int32_t log_n, int32_t W, size_t m, uint64_t* z_out, uint64_t* total_out, uint8_t* status, void* stream);
/* The same with the plan pinned, as sylow_hip_fr_scan_batch_tuned. */
/* @shape wires=u64[4*2**log_n*W*m] sigma=u64[4*2**log_n*W] shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] z_out=u64[4*2**log_n*m] total_out=u64[4*m]? status=u8[m] */
int32_t sylow_hip_plonk_permutation_batch_tuned(const uint64_t* wires, const uint64_t* sigma, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma,
                                                int32_t log_n, int32_t W, size_t m, int64_t max_blocks, int32_t totals_tile, uint64_t* z_out, uint64_t* total_out,
                                                uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_HIP_FR_SCAN_H */
