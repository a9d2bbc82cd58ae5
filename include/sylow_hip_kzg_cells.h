/*
 * sylow_hip_kzg_cells.h -- C ABI of the check of MANY CELLS OF MANY KZG BLOBS AS ONE BOOLEAN over shared commitments (kzg_cells.hip; items,
 * grids, slices, route and scratch in kzg_cells_plan.hpp).  An extension of sylow_hip.h: it includes that header, shares its conventions
 * (device pointers, word-major struct-of-arrays, the `@shape` lines, stream-ordered calls, SYLOW_HIP_E_* return values) and adds nothing to
 * it.  The entry points live in the same libsylow_hip.so.
 *
 * The domain of n = c l points, c = 2^log_c, l = 2^log_l, is cut into c cells as in sylow_hip_kzg_cosets.h: with w the n-th root of
 * sylow_hip_fr_ntt_batch for log_n = log_c + log_l and v = w^l, cell i < c holds the l values of a blob on the roots of X^l - v^i.  Row k of a
 * batch is (cell index i_k < c, commitment index b_k < n_com, l values, proof pi_k, weight r_k); R_k is the interpolant of its values.  The
 * per-row check of sylow_hip_kzg_cosets.h, weighted and summed, is
 *     e( sum_b W_b C_b - A(tau) G1gen + sum_k (r_k v^(i_k)) pi_k , G2gen ) e( -sum_k r_k pi_k , tau^l G2gen ) == 1
 *     W_b = sum_(k: b_k = b) r_k          A(X) = sum_k r_k R_k(X),  deg A < l
 * and EVERY SUM IS TAKEN IN Fr BEFORE ANYTHING TOUCHES THE CURVE: one commitment of l terms for the whole batch, one multi-scalar
 * multiplication over n_com + rows terms and one over rows, where the per-row route commits l terms per row.  The inverse transform is
 * linear and the cells of one coset share their twist, so
 *     S_i[j] = sum_(k: i_k = i) r_k val_k[j]   (c arrays of l values),   a_i = the inverse transform of l points of S_i,
 *     A[t] = sum_(i<c) a_i[t] (w^-t)^i.
 * SOUNDNESS, as sylow_hip_kzg_batch_verify_weighted: the caller draws the weights AFTER the rows are fixed (e.g. 64 or 128 random bits
 * each); THE LIBRARY DRAWS NONE.  If every row is valid the result is the identity; if any is not, the test passes with probability at most
 * 2^-(bits of the weights), provided tau_l_g2_xy is in the r-torsion.  A WEIGHT OF 0 REMOVES A ROW: a caller localises a bad cell by
 * masking weights (halves of the batch, say) through the same entry point.
 *
 * Conventions (those of sylow_hip_kzg_cosets.h):
 *   idx, com_idx: [rows] uint64.  A row with idx >= c or com_idx >= n_com ADDS NOTHING TO ANY SUM, and clears the range flag unless its
 *                weight is 0 mod r.  Repeated rows are legal.
 *   vals:        [rows][4][l], row k an Fr SoA array of stride l.  weights [4][rows].  Scalars are ANY 256-bit words, taken mod r; outputs
 *                are canonical.
 *   points:      c_xy [8][n_com] and pi_xy [8][rows] words with optional flag arrays c_inf [n_com], pi_inf [rows]; the identity is a set
 *                flag; coordinate words >= p are reduced like Fp::new.  srs_g1_xy [8][l] = tau^k G1gen, k < l, a packed prefix without
 *                flags.  tau_l_g2_xy [16] = tau^l G2gen, TRUSTED input from the ceremony: the library makes no G2 powers.
 *   calls:       stream-ordered, no host synchronisation; scratch leased per call, summed in saturating arithmetic and refused before the
 *                lease.  rows = 0: the sums are zero, the points the identity, the flag set, as sylow_hip_kzg_batch_verify_weighted at
 *                n = 0 (idx, com_idx, vals, weights, pi_xy may then be NULL; c_xy may be NULL when n_com = 0).
 *                SYLOW_HIP_E_ARG, nothing enqueued, for: NULL where a pointer is required, log_c < 0, log_l < 0,
 *                log_c + log_l > SYLOW_HIP_KZG_CELLS_LOG_N_MAX, route > 1, max_blocks == 0, outputs that overlap inputs or each other.
 */
#ifndef SYLOW_HIP_KZG_CELLS_H
#define SYLOW_HIP_KZG_CELLS_H

#include "sylow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SYLOW_HIP_KZG_CELLS_LOG_N_MAX 27

/* The Fr half.  w_out [4][n_com]: W_b, zero for a commitment no row names.  a_out [4][l]: the coefficients of A.  r_out [4][rows]: r_k mod
 * r, and rz_out [4][rows]: r_k v^(i_k); both 0 for a dropped row.  in_range_out [1]: 1 unless a row with a weight that is not 0 mod r has
 * idx >= c or com_idx >= n_com.
 * In order: one launch per row (range test, weight mod r, r v^i with v^i from the twiddle table of c points, the keys and their counts);
 * the rows grouped by commitment and, on the column route, by cell -- counts, starts and a permutation, on the device; W_b as a keyed sum;
 * then A by one of two routes with the same words:
 *   by columns (rows >= c): S_i[j] by a keyed multiply-accumulate -- a lane owns column j of key i and walks the rows of its group through
 *     the permutation, weights staged through LDS, up to 16 products unreduced per Barrett reduction; work items are (key, column)
 *     flattened, and long groups are cut into slices summed by one more launch where c l items do not fill the device -- then ONE inverse
 *     sylow_hip_fr_ntt_batch of c arrays of l points and the Horner fold over i, cut into chunks over adjacent lanes;
 *   by rows (rows < c): sylow_hip_kzg_coset_interp_batch of the rows, then sylow_hip_fr_lincomb_batch with one group. */
/* @shape idx=u64[rows] com_idx=u64[rows] vals=u64[4*2**log_l*rows] weights=u64[4*rows] w_out=u64[4*n_com] a_out=u64[4*2**log_l] r_out=u64[4*rows] rz_out=u64[4*rows] in_range_out=u8[1] */
int32_t sylow_hip_kzg_cells_fold_batch(const uint64_t* idx, const uint64_t* com_idx, const uint64_t* vals, const uint64_t* weights, int32_t log_c, int32_t log_l,
                                       size_t rows, size_t n_com, uint64_t* w_out, uint64_t* a_out, uint64_t* r_out, uint64_t* rz_out, uint8_t* in_range_out,
                                       void* stream);
/* The same with the plan pinned.  route: 0 = by rows, 1 = by columns, < 0 = the rule above.  max_blocks: the blocks of a launch of this
 * unit's kernels (>= 1, < 0 = the default).  The words depend on neither. */
/* @shape idx=u64[rows] com_idx=u64[rows] vals=u64[4*2**log_l*rows] weights=u64[4*rows] w_out=u64[4*n_com] a_out=u64[4*2**log_l] r_out=u64[4*rows] rz_out=u64[4*rows] in_range_out=u8[1] */
int32_t sylow_hip_kzg_cells_fold_batch_tuned(const uint64_t* idx, const uint64_t* com_idx, const uint64_t* vals, const uint64_t* weights, int32_t log_c, int32_t log_l,
                                             size_t rows, size_t n_com, int32_t route, int64_t max_blocks, uint64_t* w_out, uint64_t* a_out, uint64_t* r_out,
                                             uint64_t* rz_out, uint8_t* in_range_out, void* stream);
/* The fold, then the curve: F = sum_b W_b C_b + sum_k (r_k v^(i_k)) pi_k - A(tau) G1gen into f_xy [8] + f_inf [1] and P = sum_k r_k pi_k
 * into p_xy [8] + p_inf [1]; in_range_out [1] as above.  (F, z = 0, y = 0, P) is ONE ROW of the single-point verifiers
 * (sylow_hip_kzg_verify_batch / _line_table_batch) under tau^l G2gen: a cached line table of that point serves a whole batch of cells.
 * In order: the fold into scratch, one launch that concatenates the n_com + rows bases and scalars, one sylow_hip_g1_msm over them,
 * sylow_hip_kzg_commit_batch(srs_g1_xy, a, l, 1), one sylow_hip_g1_sub_batch, and one sylow_hip_g1_msm over the proofs. */
/* @shape srs_g1_xy=u64[8*2**log_l] c_xy=u64[8*n_com] c_inf=u8[n_com]? idx=u64[rows] com_idx=u64[rows] vals=u64[4*2**log_l*rows] pi_xy=u64[8*rows] pi_inf=u8[rows]? weights=u64[4*rows] f_xy=u64[8] f_inf=u8[1] p_xy=u64[8] p_inf=u8[1] in_range_out=u8[1] */
int32_t sylow_hip_kzg_cells_reduce_batch(const uint64_t* srs_g1_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* idx, const uint64_t* com_idx,
                                         const uint64_t* vals, const uint64_t* pi_xy, const uint8_t* pi_inf, const uint64_t* weights, int32_t log_c, int32_t log_l,
                                         size_t rows, size_t n_com, uint64_t* f_xy, uint8_t* f_inf, uint64_t* p_xy, uint8_t* p_inf, uint8_t* in_range_out,
                                         void* stream);
/* The reduction, then sylow_hip_pairing_product_batch over (F, G2gen), (-P, tau^l G2gen) with skip_infinity = 1: two Miller loops and ONE
 * final exponentiation whatever rows is.  gt_out [48]: the Gt element, hence the words, that sylow_hip_kzg_batch_verify_weighted yields
 * over the rows of sylow_hip_kzg_cosets_reduce_batch when every row is in range; is_one [1] = [it is the identity] AND the range flag;
 * either may be NULL (not both).  in_range_out [1] (may be NULL) receives the range flag.  PRECONDITION: tau_l_g2_xy in G2 proper. */
/* @shape srs_g1_xy=u64[8*2**log_l] tau_l_g2_xy=u64[16] c_xy=u64[8*n_com] c_inf=u8[n_com]? idx=u64[rows] com_idx=u64[rows] vals=u64[4*2**log_l*rows] pi_xy=u64[8*rows] pi_inf=u8[rows]? weights=u64[4*rows] gt_out=u64[48]? is_one=u8[1]? in_range_out=u8[1]? */
int32_t sylow_hip_kzg_cells_verify_weighted(const uint64_t* srs_g1_xy, const uint64_t* tau_l_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* idx,
                                            const uint64_t* com_idx, const uint64_t* vals, const uint64_t* pi_xy, const uint8_t* pi_inf, const uint64_t* weights,
                                            int32_t log_c, int32_t log_l, size_t rows, size_t n_com, uint64_t* gt_out, uint8_t* is_one, uint8_t* in_range_out,
                                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_HIP_KZG_CELLS_H */
