/*
 * sylow_popen.h -- C ABI of PLONK'S CLOSING ROUNDS: once a prover has committed to the quotient t (sylow_plonk.h) it evaluates its
 * polynomials at the challenge zeta, forms the linearisation polynomial r and sends two opening proofs (plonk_open.hip; slots, rows, items,
 * chunks and scratch in plonk_open_plan.hpp).  It includes sylow_plonk.h and shares its conventions (device pointers, word-major
 * struct-of-arrays, the `@shape` lines, stream-ordered calls, SYLOW_HIP_E_* return values) and adds nothing to it.  The entry points live in
 * the same libsylow_hip.so.
 *
 * WHY A HEADER AND A PREFIX OF ITS OWN.  The set of sylow_hip_* symbols is closed, and so is the set of sylow_plonk_* symbols: the tests pin
 * every exported name of either prefix to its binding table and every prototype of sylow_plonk.h to its five names.  So the closing rounds
 * get the prefix sylow_popen_ and this header, an eighth binding table, and NO sylow_hip_* AND NO sylow_plonk_* symbol is added.
 *
 * With n = 2^log_n, E = 2^log_e, N = E n (log_n + log_e <= 28), w_n the root of sylow_hip_fr_ntt_batch for n points, W wire polynomials w_j
 * (2 <= W <= SYLOW_HIP_PLONK_WIRES_MAX) and the grand product z as COEFFICIENTS, lowest first, the public-input polynomial PI, the quotient t
 * as sylow_plonk_quotient_batch writes it (N coefficients, t_e(X) = sum_{k<n} t[e n + k] X^k its E chunks), the circuit's q_0 .. q_(W-1),
 * q_M, q_C and sigma_0 .. sigma_(W-1) as coefficients of length n, the shifts k_j and the caller's challenges beta, gamma, alpha, zeta, v:
 *     evaluations   a_j = w_j(zeta), j < W;   s_j = sigma_j(zeta), j < W - 1;   zw = z(zeta w_n);   p = PI(zeta), 0 without public inputs
 *     scalars       ZH = zeta^n - 1;   L1 = ZH inv(n (zeta - 1)), inv(0) = 0;
 *                   A = prod_{j<W} (a_j + beta k_j zeta + gamma);   B = prod_{j<W-1} (a_j + beta s_j + gamma)
 *     r(X) = a_0 a_1 q_M(X) + sum_j a_j q_j(X) + q_C(X) + p
 *          + alpha [ A z(X) - B zw (a_(W-1) + beta sigma_(W-1)(X) + gamma) ]
 *          + alpha^2 L1 (z(X) - 1)
 *          - ZH sum_{e<E} zeta^(e n) t_e(X)
 *     F(X) = r(X) + sum_{j<W} v^(1+j) w_j(X) + sum_{j<W-1} v^(W+1+j) sigma_j(X)
 *     W_zeta = commit((F - F(zeta)) / (X - zeta)),     W_omega = commit((z - zw) / (X - zeta w_n))
 * r(zeta) = 0 exactly when the numerator of sylow_plonk.h at zeta equals t(zeta) (zeta^n - 1).
 * SOUNDNESS: THE LIBRARY DRAWS NO CHALLENGE.  zeta MUST BE DRAWN AFTER THE COMMITMENTS TO THE CHUNKS OF t ARE FIXED, and v AFTER THE
 * EVALUATIONS ARE FIXED (Fiat-Shamir over the transcript that holds them); beta, gamma and alpha are those of sylow_plonk.h.
 * sylow_popen_open_batch TAKES v BESIDE zeta, BEFORE IT HAS WRITTEN THE EVALUATIONS: a caller whose v depends on them calls
 * sylow_popen_evaluate_batch, draws v, calls sylow_popen_linearise_batch and then sylow_hip_kzg_open_batch itself.
 *
 * Conventions (the Fr blocks of sylow_hip.h):
 *   arrays:      [rows][4][len], row j an Fr SoA array of stride len, the rows one after another.  Scalars [4][count].  Inputs are ANY
 *                256-bit words, taken mod r; outputs are canonical.
 *   ctable:      per circuit, [2 W + 2][4][n]: the coefficients of q_0 .. q_(W-1), q_M, q_C, then of sigma_0 .. sigma_(W-1), word for word what
 *                sylow_hip_fr_ntt_batch(inverse, log_n) returns for the values on <w_n>.  ALL m INSTANCES READ IT IN PLACE.
 *   evals:       [4][(2 W + 1) m], instance-major, slot c of instance s at element (2 W + 1) s + c: a_0 .. a_(W-1), s_0 .. s_(W-2), zw, p.
 *   status:      [m] bytes.  Bit 0: r(zeta) != 0 -- the witness, t or the evaluations are inconsistent, and no proof is worth a multi-scalar
 *                multiplication.  Bit 1: zeta^n = 1 -- the challenge lies in the domain, L1 is not L_1(zeta): draw another.  The outputs
 *                are written by the formulas above in both cases.
 *   calls:       stream-ordered, no host synchronisation; scratch leased per call, summed in saturating arithmetic and refused before the
 *                lease.  m = 0: nothing is launched and nothing written.  SYLOW_HIP_E_ARG, nothing enqueued and nothing written, for: NULL
 *                where an array is required, log_n or log_e below 0 or log_n + log_e above 28, W outside
 *                2 .. SYLOW_HIP_PLONK_WIRES_MAX, max_blocks = 0, len_w or len_z outside 1 .. N (1 .. 2^28 for sylow_popen_evaluate_batch,
 *                which takes no log_e), len_out below max(n, len_z), and below len_w as well when f_out is given, the same for len_f,
 *                and any output whose bytes overlap an input's or another output's.  SYLOW_HIP_E_HIP, nothing enqueued, when the scratch
 *                limit (sylow_hip_set_scratch_limit; 1 GB by default) does not hold one instance of sylow_popen_open_batch.
 */
#ifndef SYLOW_POPEN_H
#define SYLOW_POPEN_H

#include "sylow_plonk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The coefficient table of ONE circuit, once per circuit.  selectors [W + 2][4][n] and sigma [W][4][n]: exactly the inputs of
 * sylow_plonk_quotient_prepare.  ctable: as above.  Two inverse transforms of n points, W + 2 and W arrays, straight into ctable: no copy
 * and no scratch beyond the transforms' own. */
/* @shape selectors=u64[4*2**log_n*(W+2)] sigma=u64[4*2**log_n*W] ctable=u64[4*2**log_n*(2*W+2)] */
int32_t sylow_popen_prepare(const uint64_t* selectors, const uint64_t* sigma, int32_t log_n, int32_t W, uint64_t* ctable, void* stream);

/* The 2 W + 1 evaluations of m instances in ONE pass.  wires [m][W][4][len_w], z [m][4][len_z], pi [m][4][n] (may be NULL: p = 0), zeta
 * [4][m], THE CALLER'S (see SOUNDNESS).  Items are (instance, row, chunk of 2048 coefficients): a lane runs Horner over 8 consecutive
 * coefficients, the block folds its 256 lane values with powers of the point, and a second small launch folds the chunk partials -- no
 * block waits for another.  The rows of one launch are the instance's wires, z and pi at their own lengths and the sigma rows of ctable,
 * read in place; the point is zeta for every row but z, which is evaluated at zeta w_n. */
/* @shape ctable=u64[4*2**log_n*(2*W+2)] wires=u64[4*len_w*W*m] z=u64[4*len_z*m] pi=u64[4*2**log_n*m]? zeta=u64[4*m] evals_out=u64[4*(2*W+1)*m] */
int32_t sylow_popen_evaluate_batch(const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* pi,
                                   const uint64_t* zeta, int32_t log_n, int32_t W, size_t m, uint64_t* evals_out, void* stream);
/* The same with the plan pinned.  max_blocks: the blocks of a launch (>= 1, < 0 = the default).  The words do not depend on it. */
/* @shape ctable=u64[4*2**log_n*(2*W+2)] wires=u64[4*len_w*W*m] z=u64[4*len_z*m] pi=u64[4*2**log_n*m]? zeta=u64[4*m] evals_out=u64[4*(2*W+1)*m] */
int32_t sylow_popen_evaluate_batch_tuned(const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* pi,
                                         const uint64_t* zeta, int32_t log_n, int32_t W, size_t m, int64_t max_blocks, uint64_t* evals_out, void* stream);

/* r and F of m instances.  t [m][4][N]; evals: what sylow_popen_evaluate_batch wrote (any words, taken mod r); shifts [4][W]; beta, gamma,
 * alpha, zeta and v [4][m].  r_out and f_out [m][4][len_out], zero above the polynomial's own length; either may be NULL, not both; wires
 * and v are required exactly when f_out is given and are not read otherwise.  The scalars ZH, L1, A, B and the weights of every row are
 * formed ON THE DEVICE (a block per instance; no inversion: L1 = inv(n) prod_i (1 + zeta^(2^i)) for zeta != 1), then ONE fused kernel:
 * items are (instance, tile of 256 columns), a lane owns
 * one column k and streams over the rows by coalesced 8-byte loads from the four word planes -- the shared rows of ctable, z, the E chunks of
 * t at e n + k, the wires -- each guarded by its own length, with two unreduced 16-limb accumulators (r, and what F adds), one Barrett
 * reduction per at most 16 products.  r(zeta) is then evaluated from r's coefficients for the status; every status byte is written, and it
 * is the same whichever outputs are requested. */
/* @shape ctable=u64[4*2**log_n*(2*W+2)] wires=u64[4*len_w*W*m]? z=u64[4*len_z*m] t=u64[4*2**(log_n+log_e)*m] evals=u64[4*(2*W+1)*m] shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] zeta=u64[4*m] v=u64[4*m]? r_out=u64[4*len_out*m]? f_out=u64[4*len_out*m]? status=u8[m] */
int32_t sylow_popen_linearise_batch(const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* t,
                                    const uint64_t* evals, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha,
                                    const uint64_t* zeta, const uint64_t* v, int32_t log_n, int32_t log_e, int32_t W, size_t m, size_t len_out,
                                    uint64_t* r_out, uint64_t* f_out, uint8_t* status, void* stream);
/* The same with the plan pinned, as sylow_popen_evaluate_batch_tuned. */
/* @shape ctable=u64[4*2**log_n*(2*W+2)] wires=u64[4*len_w*W*m]? z=u64[4*len_z*m] t=u64[4*2**(log_n+log_e)*m] evals=u64[4*(2*W+1)*m] shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] zeta=u64[4*m] v=u64[4*m]? r_out=u64[4*len_out*m]? f_out=u64[4*len_out*m]? status=u8[m] */
int32_t sylow_popen_linearise_batch_tuned(const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z, const uint64_t* t,
                                          const uint64_t* evals, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha,
                                          const uint64_t* zeta, const uint64_t* v, int32_t log_n, int32_t log_e, int32_t W, size_t m, size_t len_out,
                                          int64_t max_blocks, uint64_t* r_out, uint64_t* f_out, uint8_t* status, void* stream);

/* The full route under the monomial SRS srs_g1_xy [8][len_f], len_f >= max(n, len_z, len_w): evals_out as sylow_popen_evaluate_batch
 * writes them, w_zeta [8][m] + flags [m] and w_omega [8][m] + flags [m], status [m].  Per chunk of whole instances that fits the scratch
 * limit: the evaluations; the scalars and weights; the fused kernel, which writes F and a zero-padded copy of z into leased scratch of row
 * length len_f in one pass; sylow_hip_kzg_open_batch over the rows of F at zeta, and over the rows of z at zeta w_n.  THE PROOFS ARE WORD
 * FOR WORD what sylow_hip_kzg_open_batch yields for those polynomials, and depend neither on the chunks nor on a plan parameter.  Bit 0 of
 * the status is read from F(zeta) - sum_j v^(1+j) a_j - sum_j v^(W+1+j) s_j, which IS r(zeta).  v IS TAKEN BESIDE zeta (see SOUNDNESS). */
/* @shape srs_g1_xy=u64[8*len_f] ctable=u64[4*2**log_n*(2*W+2)] wires=u64[4*len_w*W*m] z=u64[4*len_z*m] pi=u64[4*2**log_n*m]? t=u64[4*2**(log_n+log_e)*m] shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] zeta=u64[4*m] v=u64[4*m] evals_out=u64[4*(2*W+1)*m] w_zeta_xy=u64[8*m] w_zeta_inf=u8[m] w_omega_xy=u64[8*m] w_omega_inf=u8[m] status=u8[m] */
int32_t sylow_popen_open_batch(const uint64_t* srs_g1_xy, const uint64_t* ctable, const uint64_t* wires, size_t len_w, const uint64_t* z, size_t len_z,
                               const uint64_t* pi, const uint64_t* t, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma,
                               const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, int32_t log_n, int32_t log_e, int32_t W, size_t m,
                               size_t len_f, uint64_t* evals_out, uint64_t* w_zeta_xy, uint8_t* w_zeta_inf, uint64_t* w_omega_xy, uint8_t* w_omega_inf,
                               uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_POPEN_H */
