/*
 * sylow_hip_kzg_points.h -- C ABI of the KZG opening of ONE polynomial at SEVERAL points under ONE proof, and its verifier
 * (kzg_points.hip; items, grids, scratch and chunks in kzg_points_plan.hpp).  An extension of sylow_hip.h: it includes that header, shares
 * its conventions (device pointers, word-major struct-of-arrays, the `@shape` lines, stream-ordered calls, SYLOW_HIP_E_* return values) and
 * adds nothing to it.  The entry points live in the same libsylow_hip.so.
 *
 * For a polynomial f of len coefficients and k points z_0 .. z_{k-1}, distinct mod r:
 *     Z(X) = prod_i (X - z_i),     R = f mod Z (the interpolant of the values y_i = f(z_i)),     q = f div Z,
 *     a_i = 1 / prod_{l != i} (z_i - z_l)     (the barycentric weights),
 *     q_i = (f - y_i) / (X - z_i)             (what sylow_hip_kzg_quotient_batch computes).
 * Then  q = sum_i a_i q_i,  R = sum_i y_i a_i Z / (X - z_i)  and  f(tau) - R(tau) = q(tau) Z(tau).  The proof is pi = q(tau) G1gen, ONE G1
 * element for the k points, and the check is
 *     e(C - R(tau) G1gen, G2gen) e(-pi, Z(tau) G2gen) == 1,
 * which needs the powers [tau^i]_2, i <= k, of the SRS on the G2 side: the verifier's key.
 * THE LIBRARY DRAWS NO CHALLENGE AND TAKES THE SRS AS GIVEN: the points are the caller's, and both halves of the SRS are trusted input.
 *
 * Conventions (those of "KZG, the prover's side" in sylow_hip.h):
 *   polynomials: coeffs [m][4][len], polynomial j an Fr SoA array of stride len at coeffs + j * 4 * len.
 *   points:      z [4][m*k], Fr SoA of stride m*k, the element (row j, point i) at index j*k + i; y and the weights have the same layout.
 *                1 <= k <= SYLOW_HIP_KZG_POINTS_MAX.
 *   scalars:     coefficients, z and y are ANY 256-bit words, taken mod r.  Outputs in Fr are canonical words below r.
 *   words:       coordinate words >= p of points are reduced like Fp::new, as everywhere.
 *   points of the curve: taken as given: no on-curve check, no subgroup check.  Outputs as affine words + flags, the identity as (0, 1) + flag.
 *   repeats:     a row whose points are NOT distinct mod r is defined, and is not a valid opening: the weights come from inv(0) = 0, so
 *                every point that collides with another one gets the weight 0 and drops out of q and R.  The verifier rejects such a row
 *                whatever else it holds.
 *   calls:       stream-ordered, no host synchronisation; scratch leased per call.  m = 0 (n = 0): OK, nothing launched, nothing written.
 *                SYLOW_HIP_E_ARG, no launch, nothing written, for: NULL where a pointer is required, len = 0, k = 0,
 *                k > SYLOW_HIP_KZG_POINTS_MAX, sizes whose scratch does not fit size_t.
 */
#ifndef SYLOW_HIP_KZG_POINTS_H
#define SYLOW_HIP_KZG_POINTS_H

#include "sylow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SYLOW_HIP_KZG_POINTS_MAX 64      /* points of one opening, at most: a data-availability cell */

/* The barycentric weights a_{j,i} = 1 / prod_{l != i} (z_{j,i} - z_{j,l}) of m rows of k points: one small kernel forms the m k denominators,
 * sylow_hip_fr_batch_inv inverts them (inv(0) = 0).  distinct_out [m] (may be NULL) receives 1 iff no denominator of row j is 0 mod r, which
 * is iff the k points of the row are distinct mod r.  k = 1: the empty product, a = 1. */
/* @shape z=u64[4*m*k] a_out=u64[4*m*k] distinct_out=u8[m]? */
int32_t sylow_hip_kzg_points_weights_batch(const uint64_t* z, size_t k, size_t m, uint64_t* a_out, uint8_t* distinct_out, void* stream);
/* q_j = sum_i a_{j,i} q_{j,i} into q_out [m][4][len] (q_e = 0 written for e >= len - 1, as the single-point call does) and
 * y_{j,i} = f_j(z_{j,i}) into y_out [4][m*k].  For distinct points q_j = f_j div Z_j, which is 0 when len <= k.  Exact in Fr.  Either
 * output may be NULL, not both; q_out = NULL is evaluation at m k points.  q_out must NOT overlap coeffs (the byte ranges of 32 len m
 * bytes are compared).  The k Horner scans of a polynomial are independent: the totals and the carry level of
 * sylow_hip_kzg_quotient_batch run over (polynomial, point, chunk) items, then ONE kernel walks the k points of a chunk inside the block,
 * adds a_i h into per-lane accumulators and stores the quotient once.  No [m k][len] array exists; the scratch is the weights and, for
 * polynomials longer than one chunk of 2048, 64 bytes per (polynomial, point, chunk). */
/* @shape coeffs=u64[4*len*m] z=u64[4*m*k] q_out=u64[4*len*m]? y_out=u64[4*m*k]? */
int32_t sylow_hip_kzg_quotient_points_batch(const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z, size_t k,
                                            uint64_t* q_out, uint64_t* y_out, void* stream);
/* The opening of f_j at its k points: y_{j,i} and pi_j = commit(q_j) over srs_g1_xy [8][len] -- the quotient into leased scratch (32 len m
 * bytes), then the commitment of sylow_hip_kzg_commit_batch.  pi_j is flagged as the identity exactly when q_j = 0 (len <= k, or f_j of
 * degree below k). */
/* @shape srs_g1_xy=u64[8*len] coeffs=u64[4*len*m] z=u64[4*m*k] y_out=u64[4*m*k] pi_xy=u64[8*m] pi_inf=u8[m] */
int32_t sylow_hip_kzg_open_points_batch(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z, size_t k,
                                        uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream);
/* The verifier's Fr half for n rows, in polynomial layout: zpoly_out [n][4][k+1] = Z_j (monic: its coefficient k is 1) and
 * rpoly_out [n][4][k] = R_j = sum_i y_{j,i} a_{j,i} Z_j / (X - z_{j,i}); distinct_out [n] as above.  One wavefront per row, 2 k^2 products. */
/* @shape z=u64[4*n*k] y=u64[4*n*k] zpoly_out=u64[4*n*(k+1)] rpoly_out=u64[4*n*k] distinct_out=u8[n] */
int32_t sylow_hip_kzg_points_polys_batch(const uint64_t* z, const uint64_t* y, size_t k, size_t n, uint64_t* zpoly_out, uint64_t* rpoly_out,
                                         uint8_t* distinct_out, void* stream);
/* ok_j = [ e(C_j - R_j(tau) G1gen, G2gen) e(-pi_j, Z_j(tau) G2gen) == 1 ] AND [ the k points of row j are distinct mod r ].
 * srs_g1_xy [8][k] = [tau^i]_1, i < k; srs_g2_xy [16][k+1] = [tau^i]_2, i <= k: both WITHOUT flag arrays, packed prefixes of the SRS (the
 * SoA strides are k and k + 1).  c_xy [8][n] and pi_xy [8][n] with optional flag arrays.  In order: the Fr half into scratch; R(tau) G1gen
 * by the commitment of sylow_hip_kzg_commit_batch with len = k; Z(tau) G2gen by sylow_hip_g2_lincomb_batch, in chunks of whole rows that fit
 * sylow_hip_set_scratch_limit; sylow_hip_g1_sub_batch; the pair list; sylow_hip_multi_pairing_batch with skip_infinity = 1.  A flagged pi
 * (q = 0) is legal: the row is then valid iff C = R(tau) G1gen.  PRECONDITION: the G2 powers in G2 proper. */
/* @shape srs_g1_xy=u64[8*k] srs_g2_xy=u64[16*(k+1)] c_xy=u64[8*n] c_inf=u8[n]? z=u64[4*n*k] y=u64[4*n*k] pi_xy=u64[8*n] pi_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_kzg_verify_points_batch(const uint64_t* srs_g1_xy, const uint64_t* srs_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf,
                                          const uint64_t* z, const uint64_t* y, size_t k, size_t n, const uint64_t* pi_xy,
                                          const uint8_t* pi_inf, uint8_t* ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_HIP_KZG_POINTS_H */
