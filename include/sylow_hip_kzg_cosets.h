/*
 * sylow_hip_kzg_cosets.h -- C ABI of the KZG proofs of ONE polynomial on EVERY COSET of its domain, and their verifier (kzg_cosets.hip;
 * items, planes, grids and scratch in kzg_cosets_plan.hpp).  An extension of sylow_hip.h: it includes that header, shares its conventions
 * (device pointers, word-major struct-of-arrays, the `@shape` lines, stream-ordered calls, SYLOW_HIP_E_* return values) and adds nothing to
 * it.  The entry points live in the same libsylow_hip.so.
 *
 * The domain of n = c l points, c = 2^log_c, l = 2^log_l, is cut into c cosets ("cells") of l points.  With w the n-th root of
 * sylow_hip_fr_ntt_batch for log_n = log_c + log_l, v = w^l and u = w^c:
 *     coset i < c = { w^(i + c j) : j < l }, the roots of Z_i = X^l - v^i;      q_i = f div Z_i,   R_i = f mod Z_i;
 *     pi_i = q_i(tau) G1gen: ONE G1 element for the l values of the cell, the values y[i + c j], j < l, of the forward transform of f.
 * The prover (the multi-proof form of Feist-Khovratovich): pi_i = sum_(t<c) v^(it) h_t, a forward G1 transform of c points, with
 * h_t = sum_k f_(k+(t+1)l) s_k; split by k = a + l u into l Toeplitz products of size c, each a cyclic convolution of 2c points against a
 * table that depends on the SRS alone.  2n products per polynomial, then transforms of 2c and c points.
 * The verifier: R_i has the coefficients r_k = l^-1 w^(-ik) sum_j val_j u^(-jk), and
 *     e(C - R_i(tau) G1gen, G2gen) e(-pi, tau^l G2gen - v^i G2gen) == 1   <=>   e(C - R_i(tau) G1gen + v^i pi, G2gen) e(-pi, tau^l G2gen) == 1,
 * the single-point check of sylow_hip_kzg_verify_batch / _line_table_batch / sylow_hip_kzg_batch_verify_weighted with tau_g2 := tau^l G2gen,
 * c := C - R_i(tau) G1gen, z := v^i, y := 0: one G2 point and one line table for the whole batch.
 * THE LIBRARY MAKES NO G2 POWERS: tau^l G2gen is trusted input from the ceremony, like tau_g2.
 *
 * Conventions (those of "KZG, the prover's side" in sylow_hip.h):
 *   Fr arrays:   [rows][4][len], row j an Fr SoA array of stride len.  Scalars are ANY 256-bit words, taken mod r; outputs are canonical.
 *   points:      [m][8][len] words + [m][len] flags; the identity is (0, 1) + flag; coordinate words >= p are reduced like Fp::new.
 *   calls:       stream-ordered, no host synchronisation; scratch leased per call, summed in saturating arithmetic and refused before the
 *                lease.  m = 0 / rows = 0: OK, nothing launched, nothing written.
 *                SYLOW_HIP_E_ARG, nothing enqueued, for: NULL where a pointer is required, log_c < 0, log_l < 0,
 *                log_c + log_l > SYLOW_HIP_KZG_COSETS_LOG_N_MAX, max_blocks == 0, planes_log > log_l, outputs that overlap inputs.
 */
#ifndef SYLOW_HIP_KZG_COSETS_H
#define SYLOW_HIP_KZG_COSETS_H

#include "sylow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SYLOW_HIP_KZG_COSETS_LOG_N_MAX 27

/* The table of an SRS for (log_c, log_l), once: srs_g1_xy [8][n] = tau^k G1gen (s_0 .. s_(n-l-1) are read), no flag array.
 * table_xy [l][8][2c] + table_inf [l][2c]: array a < l is the forward transform of x^(a), x^(a)_(2c-1-u) = s_(a + l u) for u <= c - 2 and the
 * identity elsewhere.  The l arrays go into scratch and through ONE sylow_hip_g1_ntt_batch call with m = l over 2c points, so the table is
 * word for word that call's output; at log_l = 0 it is sylow_hip_kzg_open_all_prepare's.  A SET FLAG IS AN OUTPUT, NOT AN ERROR. */
/* @shape srs_g1_xy=u64[8*2**(log_c+log_l)] table_xy=u64[16*2**(log_c+log_l)] table_inf=u8[2*2**(log_c+log_l)] */
int32_t sylow_hip_kzg_open_cosets_prepare(const uint64_t* srs_g1_xy, int32_t log_c, int32_t log_l, uint64_t* table_xy, uint8_t* table_inf, void* stream);
/* The c proofs of each of m polynomials, coeffs [m][4][n]: pi_xy [m][8][c] + pi_inf [m][c], proof i for coset i.  y_out [m][4][n] (may be
 * NULL) receives the forward Fr transform in natural order: value j of cell i is y[i + c j].  table_inf may be NULL (no flagged entry).
 * In order: the split of each polynomial into l residue arrays, scaled by (2c)^-1 and padded to 2c; ONE sylow_hip_fr_ntt_batch of m l
 * arrays; the product-sums fused with stage 0 of the inverse G1 transform of 2c points, over planes (below); the fold of the planes; the
 * remaining stages, the forward transform of c points and the closing kernel of sylow_hip_kzg_open_all_batch.  log_c = 0: the one proof is
 * the identity (one small launch).  A polynomial of degree below l has every proof flagged. */
/* @shape table_xy=u64[16*2**(log_c+log_l)] table_inf=u8[2*2**(log_c+log_l)]? coeffs=u64[4*2**(log_c+log_l)*m] y_out=u64[4*2**(log_c+log_l)*m]? pi_xy=u64[8*2**log_c*m] pi_inf=u8[2**log_c*m] */
int32_t sylow_hip_kzg_open_cosets_batch(const uint64_t* table_xy, const uint8_t* table_inf, const uint64_t* coeffs, int32_t log_c, int32_t log_l, size_t m,
                                        uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream);
/* The same with the plan pinned.  max_blocks: the blocks of a multiplying launch, as sylow_hip_g1_ntt_batch_tuned (>= 1, < 0 = the default).
 * planes_log: the product-sums of a butterfly are cut into 2^planes_log planes of l / 2^planes_log residues each, summed by one more launch;
 * 0 .. log_l, < 0 = the default (the smallest count that brings c m planes up to the resident lanes, 1 when c m fills them).  The words do
 * not depend on either. */
/* @shape table_xy=u64[16*2**(log_c+log_l)] table_inf=u8[2*2**(log_c+log_l)]? coeffs=u64[4*2**(log_c+log_l)*m] y_out=u64[4*2**(log_c+log_l)*m]? pi_xy=u64[8*2**log_c*m] pi_inf=u8[2**log_c*m] */
int32_t sylow_hip_kzg_open_cosets_batch_tuned(const uint64_t* table_xy, const uint8_t* table_inf, const uint64_t* coeffs, int32_t log_c, int32_t log_l, size_t m,
                                              int64_t max_blocks, int32_t planes_log, uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream);
/* The verifier's Fr half: for row j, the coefficients of R = the polynomial of degree below l with the values vals [rows][4][l] on coset
 * idx_j mod c, into r_out [rows][4][l] (canonical words; must not overlap vals).  in_range_out [rows] (may be NULL) receives 1 iff idx_j < c.
 * The inverse sylow_hip_fr_ntt_batch of l points, then one launch multiplies r_k by w^(-idx k) with running products (no exponentiation per
 * element). */
/* @shape vals=u64[4*2**log_l*rows] idx=u64[rows] r_out=u64[4*2**log_l*rows] in_range_out=u8[rows]? */
int32_t sylow_hip_kzg_coset_interp_batch(const uint64_t* vals, const uint64_t* idx, int32_t log_c, int32_t log_l, size_t rows, uint64_t* r_out,
                                         uint8_t* in_range_out, void* stream);
/* The rows the three single-point verifiers take with y = 0 under tau^l G2gen: cred_j = C_j - R_j(tau) G1gen into cred_xy [8][rows] +
 * cred_inf [rows] and z_j = v^idx_j into z_out [4][rows]; in_range_out as above (may be NULL).  srs_g1_xy [8][l] = [tau^k]_1, k < l, a
 * packed prefix without flags; c_xy [8][rows] with an optional flag array.  In order: the interpolation into scratch, R(tau) G1gen through
 * sylow_hip_kzg_commit_batch with len = l and m = rows, sylow_hip_g1_sub_batch. */
/* @shape srs_g1_xy=u64[8*2**log_l] c_xy=u64[8*rows] c_inf=u8[rows]? idx=u64[rows] vals=u64[4*2**log_l*rows] cred_xy=u64[8*rows] cred_inf=u8[rows] z_out=u64[4*rows] in_range_out=u8[rows]? */
int32_t sylow_hip_kzg_cosets_reduce_batch(const uint64_t* srs_g1_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* idx, const uint64_t* vals,
                                          int32_t log_c, int32_t log_l, size_t rows, uint64_t* cred_xy, uint8_t* cred_inf, uint64_t* z_out,
                                          uint8_t* in_range_out, void* stream);
/* ok_j = [ e(C_j - R_j(tau) G1gen, G2gen) e(-pi_j, tau^l G2gen - v^idx_j G2gen) == 1 ] AND [ idx_j < c ]: the reduction above into scratch,
 * then sylow_hip_kzg_verify_batch with tau_g2 := tau_l_g2_xy [16] = tau^l G2gen, y = 0.  A flagged pi (q = 0) is legal: the row is then valid
 * iff C = R(tau) G1gen.  PRECONDITION: tau_l_g2_xy in G2 proper. */
/* @shape srs_g1_xy=u64[8*2**log_l] tau_l_g2_xy=u64[16] c_xy=u64[8*rows] c_inf=u8[rows]? idx=u64[rows] vals=u64[4*2**log_l*rows] pi_xy=u64[8*rows] pi_inf=u8[rows]? ok=u8[rows] */
int32_t sylow_hip_kzg_verify_cosets_batch(const uint64_t* srs_g1_xy, const uint64_t* tau_l_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* idx,
                                          const uint64_t* vals, int32_t log_c, int32_t log_l, size_t rows, const uint64_t* pi_xy, const uint8_t* pi_inf,
                                          uint8_t* ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_HIP_KZG_COSETS_H */
