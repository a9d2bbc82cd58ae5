/*
 * sylow_hip_kzg_recover.h -- C ABI of the recovery of a KZG polynomial from ANY HALF of the cells of its domain (kzg_recover.hip; items,
 * staging, grids and scratch in kzg_recover_plan.hpp).  An extension of sylow_hip.h: it includes that header, shares its conventions
 * (device pointers, word-major struct-of-arrays, the `@shape` lines, stream-ordered calls, SYLOW_HIP_E_* return values) and adds nothing to
 * it.  The entry points live in the same libsylow_hip.so.
 *
 * The domain of n = c l points, c = 2^log_c, l = 2^log_l, is cut into c cells as in sylow_hip_kzg_cosets.h: with w the n-th root of
 * sylow_hip_fr_ntt_batch for log_n = log_c + log_l and v = w^l, cell i < c holds the values y[i + c j], j < l, the layout of `y_out` of
 * sylow_hip_kzg_open_cosets_batch.  A blob is a polynomial f of degree BELOW n / 2 -- the extension is fixed at 2x, no other rate is
 * served -- so any c / 2 cells determine it.  With M the missing cells of a row, |M| <= c / 2 (rounded down), and s = 5:
 *     Z(X) = prod_(i in M) (X^l - v^i) vanishes on exactly the missing cells.  It is a polynomial in X^l, so it takes c values on the
 *     domain and c on the coset s <w>:   zd[k] = prod_(i in M) (v^k - v^i),  0 exactly for k in M;
 *                                       zc[k] = prod_(i in M) (s^l v^k - v^i),  never 0.
 *     1. t[i + c j] = y[i + c j] zd[i]          missing cells become 0 whatever words they held
 *     2. P = the inverse transform of t          = f Z exactly: deg(f Z) < n / 2 + l |M| <= n
 *     3. e = the forward transform of P with shift s
 *     4. q[t] = e[t] zc[t mod c]^-1              c inversions per row, not n
 *     5. f = the inverse transform of q with shift s
 * The upper half of the n coefficients of step 5 is zero exactly when the present cells are the values of a polynomial of degree below
 * n / 2; with |M| = c / 2 every input is consistent with one.
 * THE VANISHING VALUES COST c |M| PRODUCTS PER ARRAY AND ROW, quadratic in c: log_c is capped at SYLOW_HIP_KZG_RECOVER_LOG_C_MAX.
 *
 * Conventions:
 *   Fr arrays:   [m][4][len], row j an Fr SoA array of stride len.  Scalars are ANY 256-bit words, taken mod r; outputs are canonical.
 *   calls:       stream-ordered, no host synchronisation; scratch leased per call, summed in saturating arithmetic and refused before the
 *                lease.  m = 0: OK, nothing launched, nothing written.
 *                SYLOW_HIP_E_ARG, nothing enqueued, for: NULL where a pointer is required, log_c < 0, log_l < 0, log_c + log_l < 1 (a
 *                domain of one point has no polynomial of degree below 1/2), log_c > SYLOW_HIP_KZG_RECOVER_LOG_C_MAX,
 *                log_c + log_l > SYLOW_HIP_KZG_RECOVER_LOG_N_MAX, outputs that overlap inputs or each other.
 */
#ifndef SYLOW_HIP_KZG_RECOVER_H
#define SYLOW_HIP_KZG_RECOVER_H

#include "sylow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SYLOW_HIP_KZG_RECOVER_LOG_C_MAX 12     /* the vanishing values cost c |M| products per row */
#define SYLOW_HIP_KZG_RECOVER_LOG_N_MAX 27

/* present [m][c] bytes, non-zero = the cell is held.  zd_out, zc_out [m][4][c] canonical words; status_out [m]:
 * 0 = recoverable, 1 = more than c/2 cells missing (zd row all zero, zc row all one).  One launch for the constants s and s^l, the table
 * of the transform of c points for the powers of v, and one launch for the values: two product chains per (row, k) over the missing
 * roots staged in LDS, cut over 16 lanes from 32 cells on. */
/* @shape present=u8[2**log_c*m] zd_out=u64[4*2**log_c*m] zc_out=u64[4*2**log_c*m] status_out=u8[m] */
int32_t sylow_hip_kzg_recover_vanish_batch(const uint8_t* present, int32_t log_c, int32_t log_l, size_t m,
                                           uint64_t* zd_out, uint64_t* zc_out, uint8_t* status_out, void* stream);

/* y [m][4][n] in the layout of open_cosets' y_out; words of missing cells are never part of the result.  coeffs_out [m][4][n]: the n
 * coefficients of step 5, canonical.  y_out (may be NULL): their forward transform, i.e. every cell, the missing ones restored.
 * status_out [m]: 0 = recovered (upper half zero), 1 = too few cells (row of coeffs_out and y_out all zero), 2 = the present cells are
 * not the values of a polynomial of degree below n/2 (coeffs_out is what step 5 yields, as the model says).
 * In order: the vanishing values into scratch, sylow_hip_fr_batch_inv of the m c values zc, step 1 into scratch, the transforms of steps
 * 2, 3 and 5 through sylow_hip_fr_ntt_batch with step 4 in place between them, the reduction of the upper halves, and the transform into
 * y_out. */
/* @shape y=u64[4*2**(log_c+log_l)*m] present=u8[2**log_c*m] coeffs_out=u64[4*2**(log_c+log_l)*m] y_out=u64[4*2**(log_c+log_l)*m]? status_out=u8[m] */
int32_t sylow_hip_kzg_recover_batch(const uint64_t* y, const uint8_t* present, int32_t log_c, int32_t log_l, size_t m,
                                    uint64_t* coeffs_out, uint64_t* y_out, uint8_t* status_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_HIP_KZG_RECOVER_H */
