/*
 * sylow_plonk.h -- C ABI of the PLONK PROVER SURFACE: for now the quotient polynomial t, the one polynomial a PLONK-family prover needs
 * between the grand product z (sylow_hip_fr_scan.h) and its openings (plonk_quotient.hip; rows, items, the degree bound, chunks and scratch
 * in plonk_quotient_plan.hpp).  It includes sylow_hip_fr_scan.h and shares its conventions (device pointers, word-major struct-of-arrays,
 * the `@shape` lines, stream-ordered calls, SYLOW_HIP_E_* return values) and adds nothing to it.  The entry points live in the same
 * libsylow_hip.so.
 *
 * WHY A HEADER AND A PREFIX OF ITS OWN.  The set of sylow_hip_* symbols is closed: the tests pin every exported sylow_hip_* name to one of
 * the six binding tables, those tables to their headers, and every prototype of sylow_hip.h to a row of the memory contract.  The prover
 * surface will grow (the quotient now, linearisation helpers later), so it gets the prefix sylow_plonk_ and this header, a seventh binding
 * table, and NO sylow_hip_* symbol is added.  The closing rounds -- evaluations, linearisation, the two openings -- are in sylow_popen.h.
 *
 * With n = 2^log_n, E = 2^log_e, N = E n (log_n + log_e <= 28), w_N the root of sylow_hip_fr_ntt_batch for N points and w_n = w_N^E, the
 * coset K = 5 <w_N> (5: the shift of sylow_hip_groth16_quotient_batch; X^n - 1 never vanishes on K), x_i = 5 w_N^i, W wire columns w_j
 * (2 <= W <= SYLOW_HIP_PLONK_WIRES_MAX), the shifts k_j and the permutation columns sigma_j of sylow_hip_plonk_permutation_batch, the
 * linear selectors q_0 .. q_(W-1), q_M and q_C, the public-input polynomial PI and the caller's challenges beta, gamma and alpha:
 *     gate     = q_M w_0 w_1 + sum_j q_j w_j + q_C + PI
 *     perm     = z(X) prod_j (w_j + beta k_j X + gamma)  -  z(w_n X) prod_j (w_j + beta sigma_j + gamma)
 *     boundary = L_1(X) (z(X) - 1)
 *     t(X)     = [ gate + alpha perm + alpha^2 boundary ] / (X^n - 1)
 * SOUNDNESS: THE LIBRARY DRAWS NO CHALLENGE.  beta and gamma MUST BE DRAWN AFTER THE WIRE COMMITMENTS ARE FIXED, and alpha AFTER THE
 * COMMITMENT TO z IS FIXED (Fiat-Shamir over the transcript that holds them); a prover who knows them before it chooses its wires or its z
 * can make t a polynomial for wires that break the constraints.
 *
 * Conventions (the Fr blocks of sylow_hip.h):
 *   arrays:      [rows][4][len], row j an Fr SoA array of stride len, the rows one after another.  Scalars [4][count].  Inputs are ANY
 *                256-bit words, taken mod r; outputs are canonical.
 *   table:       per circuit, [2 W + 3][4][N] then [4][E].  Rows 0 .. W+1: the selectors q_0 .. q_(W-1), q_M, q_C; rows W+2 .. 2W+1: sigma;
 *                row 2W+2: L_1 -- each the values on K, in natural order, word for word what sylow_hip_fr_ntt_batch(forward, shift = 5,
 *                log_n + log_e) returns for the zero-padded coefficients sylow_hip_fr_ntt_batch(inverse, log_n) returns for the values on
 *                <w_n> (L_1: the values 1, 0, .., 0).  The tail: zinv_k = (5^n w_E^k - 1)^-1 for k < E, w_E = w_N^n: X^n - 1 takes only
 *                these E values on K, at point i the one of index i mod E.
 *   status:      [m] bytes.  Bit 0: some coefficient of t_out at an index above D - n is not 0, D the degree bound of the numerator below:
 *                X^n - 1 does not divide the numerator, the constraints do not hold, and no commitment to t is worth a multi-scalar
 *                multiplication.  When D < N the converse holds too: status 0 means X^n - 1 divides.  WHEN D >= N -- the normal case for
 *                blinded wires, W = 3 and E = 4 -- t_out is the polynomial of degree < N that agrees with the quotient on K, and STATUS 0
 *                DOES NOT PROVE DIVISIBILITY: the numerator is folded mod X^N - 5^N before the tail is read.
 *   calls:       stream-ordered, no host synchronisation; scratch leased per call, summed in saturating arithmetic and refused before the
 *                lease.  m = 0: nothing is launched and nothing written.  SYLOW_HIP_E_ARG, nothing enqueued and nothing written, for: NULL
 *                where an array is required, log_n or log_e below 0 or log_n + log_e above 28, W outside
 *                2 .. SYLOW_HIP_PLONK_WIRES_MAX, max_blocks = 0, len_w or len_z outside 1 .. N, D - n >= N, and any output whose bytes
 *                overlap an input's or another output's.  SYLOW_HIP_E_HIP, nothing enqueued, when the scratch limit
 *                (sylow_hip_set_scratch_limit; 1 GB by default) does not hold one instance of sylow_plonk_quotient_batch.
 */
#ifndef SYLOW_PLONK_H
#define SYLOW_PLONK_H

#include "sylow_hip_fr_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The table of ONE circuit, once per circuit.  selectors [W + 2][4][n]: the values on <w_n> of q_0 .. q_(W-1), q_M, q_C, in this order.
 * sigma [W][4][n]: exactly the sigma of sylow_hip_plonk_permutation_batch.  table: as above.  In order: three inverse transforms of n points
 * (the selectors, sigma, L_1), the zero-padding, ONE forward transform of 2 W + 3 arrays of N points onto K, and one launch for zinv. */
/* @shape selectors=u64[4*2**log_n*(W+2)] sigma=u64[4*2**log_n*W] table=u64[4*2**(log_n+log_e)*(2*W+3)+4*2**log_e] */
int32_t sylow_plonk_quotient_prepare(const uint64_t* selectors, const uint64_t* sigma, int32_t log_n, int32_t log_e, int32_t W, uint64_t* table, void* stream);

/* The fused kernel alone, for m instances over one table.  wires_ext [m][W][4][N] (column j of instance s at row s W + j), z_ext [m][4][N]
 * and pi_ext [m][4][N] (may be NULL: PI = 0): the VALUES on K in natural order, point i at x_i.  shifts [4][W].  beta, gamma and alpha
 * [4][m], one triple per instance, THE CALLER'S (see SOUNDNESS).  t_ext_out [m][4][N]:
 *     t_ext[i] = (gate + alpha perm + alpha^2 boundary)(x_i) zinv[i mod E],     z(w_n X) at point i being z_ext[(i + E) mod N]
 * so the output must not overlap any input.  One lane per point; a lane streams over the columns -- w_j, sigma_j and q_j by coalesced
 * 8-byte loads from the four word planes -- with three accumulators, so W = 32 costs no more registers than W = 3; the gate sum is added
 * unreduced, one Barrett reduction per at most 16 products.  One launch, and one for the table of the N / 2 roots in leased scratch. */
/* @shape table=u64[4*2**(log_n+log_e)*(2*W+3)+4*2**log_e] wires_ext=u64[4*2**(log_n+log_e)*W*m] z_ext=u64[4*2**(log_n+log_e)*m] pi_ext=u64[4*2**(log_n+log_e)*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] t_ext_out=u64[4*2**(log_n+log_e)*m] */
int32_t sylow_plonk_quotient_evals_batch(const uint64_t* table, const uint64_t* wires_ext, const uint64_t* z_ext, const uint64_t* pi_ext, const uint64_t* shifts,
                                         const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, int32_t log_n, int32_t log_e, int32_t W, size_t m,
                                         uint64_t* t_ext_out, void* stream);
/* The same with the plan pinned.  max_blocks: the blocks of the launch (>= 1, < 0 = the default).  The words do not depend on it. */
/* @shape table=u64[4*2**(log_n+log_e)*(2*W+3)+4*2**log_e] wires_ext=u64[4*2**(log_n+log_e)*W*m] z_ext=u64[4*2**(log_n+log_e)*m] pi_ext=u64[4*2**(log_n+log_e)*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] t_ext_out=u64[4*2**(log_n+log_e)*m] */
int32_t sylow_plonk_quotient_evals_batch_tuned(const uint64_t* table, const uint64_t* wires_ext, const uint64_t* z_ext, const uint64_t* pi_ext,
                                               const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, int32_t log_n,
                                               int32_t log_e, int32_t W, size_t m, int64_t max_blocks, uint64_t* t_ext_out, void* stream);

/* The full route from COEFFICIENTS.  wires [m][W][4][len_w], z [m][4][len_z] and pi [m][4][n] (may be NULL): the coefficients, lowest
 * first.  The lengths are free in 1 .. N, so the caller can blind: a(X) + (b_1 X + b_2)(X^n - 1) has len_w = n + 2, and z with three
 * blinders len_z = n + 3.  t_out [m][4][N]: the coefficients of the polynomial of degree < N that equals the numerator over X^n - 1 on K.
 * status [m]: see above.  The degree bound of the numerator is
 *     D = max( (len_z - 1) + W max(len_w - 1, 1),   2 (len_w - 1) + n - 1,   n + len_z - 2 )
 * and D - n >= N is SYLOW_HIP_E_ARG.
 * In order, per chunk of whole instances that fits the scratch limit: the W + 1 (+ 1 with pi) arrays of every instance zero-padded into
 * leased scratch; ONE forward transform over them onto K; the fused kernel; ONE inverse transform from K into t_out; and, once for the
 * call, a small kernel that ORs the tail of t_out into the status -- every status byte is written.  The words depend neither on the
 * chunks nor on max_blocks. */
/* @shape table=u64[4*2**(log_n+log_e)*(2*W+3)+4*2**log_e] wires=u64[4*len_w*W*m] z=u64[4*len_z*m] pi=u64[4*2**log_n*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] t_out=u64[4*2**(log_n+log_e)*m] status=u8[m] */
int32_t sylow_plonk_quotient_batch(const uint64_t* table, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* pi,
                                   const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, int32_t log_n, int32_t log_e,
                                   int32_t W, size_t m, uint64_t* t_out, uint8_t* status, void* stream);
/* The same with the plan pinned, as sylow_plonk_quotient_evals_batch_tuned. */
/* @shape table=u64[4*2**(log_n+log_e)*(2*W+3)+4*2**log_e] wires=u64[4*len_w*W*m] z=u64[4*len_z*m] pi=u64[4*2**log_n*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] t_out=u64[4*2**(log_n+log_e)*m] status=u8[m] */
int32_t sylow_plonk_quotient_batch_tuned(const uint64_t* table, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* pi,
                                         const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, int32_t log_n,
                                         int32_t log_e, int32_t W, size_t m, int64_t max_blocks, uint64_t* t_out, uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_PLONK_H */
