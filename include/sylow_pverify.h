/*
 * sylow_pverify.h -- C ABI of THE BATCHED PLONK VERIFIER: many proofs of ONE circuit, as they come out of sylow_plonk.h and sylow_popen.h,
 * checked as per-proof flags or as one sound boolean (plonk_verify.hip; terms, slots, columns, chunks and scratch in plonk_verify_plan.hpp).
 * It includes sylow_popen.h and shares its conventions (device pointers, word-major struct-of-arrays, the `@shape` lines, stream-ordered
 * calls, SYLOW_HIP_E_* return values) and adds nothing to it.  The entry points live in the same libsylow_hip.so.
 *
 * WHY A HEADER AND A PREFIX OF ITS OWN.  The sets of sylow_hip_*, of sylow_plonk_* and of sylow_popen_* symbols are closed: the tests pin
 * every exported name of each prefix to its binding table and every prototype of the two PLONK headers to its names.  So the verifier gets
 * the prefix sylow_pverify_ and this header, a ninth binding table, and NO sylow_hip_*, NO sylow_plonk_* AND NO sylow_popen_* symbol is
 * added.  NO PAIRING, GROUP-LAW OR MSM KERNEL IS NEW: the G1 and pairing work goes through sylow_hip_g1_lincomb_batch, sylow_hip_g1_msm,
 * sylow_hip_kzg_verify_batch and sylow_hip_pairing_product_batch; the new device code is the verifier's Fr side and the gather that feeds them.
 *
 * W, n = 2^log_n, E = 2^log_e, w_n, the shifts k_j, the challenges beta, gamma, alpha, zeta, v, the evaluations a_j (j < W), s_j (j < W - 1)
 * and zw, and the scalars ZH, L1, A, B are those of sylow_popen.h.  One more challenge u is the caller's.  The verifying key is the
 * commitments [q_0] .. [q_(W-1)], [q_M], [q_C], [sigma_0] .. [sigma_(W-1)], in ctable row order; a proof's points are [w_0] .. [w_(W-1)],
 * [z], [t_0] .. [t_(E-1)], W_zeta, W_omega.  The prover's F satisfies F(zeta) = sum_j v^(1+j) a_j + sum_{j<W-1} v^(W+1+j) s_j exactly when
 * r(zeta) = 0, so a verifier checks the two openings ([F], zeta, F(zeta), W_zeta) and ([z], zeta w_n, zw, W_omega), folded with u:
 *   1. p from the public inputs.  pub holds the l = n_pub values of PI on rows 0 .. l - 1 of the domain, PI is 0 on every other row,
 *      0 <= l <= n:   p = sum_{j<l} pub_j L_j(zeta),   L_j(zeta) = w_n^j ZH inv(n (zeta - w_n^j)), inv(0) = 0  (j = 0: the L1 above).
 *   2. the T = 3 W + E + 5 term scalars of C, the 2 W + 2 key points first, then the W + E + 3 proof points; with B' = alpha B zw:
 *        [q_j], j < W           a_j                          [w_j]     v^(1+j)
 *        [q_M]                  a_0 a_1                      [z]       alpha A + alpha^2 L1 + u
 *        [q_C]                  1                            [t_e]     -ZH zeta^(e n)
 *        [sigma_j], j < W - 1   v^(W+1+j)                    W_zeta    zeta
 *        [sigma_(W-1)]          -beta B'                     W_omega   u zeta w_n
 *   3. the value (the constant parts of r go here, not to a generator term):
 *        y = sum_j v^(1+j) a_j + sum_{j<W-1} v^(W+1+j) s_j + u zw - [ p - B' (a_(W-1) + gamma) - alpha^2 L1 ]
 *   4. the row:   C = sum_terms k_c P_c,   pi = W_zeta + u W_omega,   ok = [ e(C - y G1gen, G2gen) e(-pi, tau G2gen) == 1 ],
 *      the boolean sylow_hip_kzg_verify_batch returns for the row (C, z = 0, y, pi); a zero scalar is legal there by that call's contract.
 *      For u != 0 drawn after the proof, ok holds exactly when both openings verify, up to the usual 1 / r.
 *   5. the weighted form, with weights rho_i over m proofs:
 *        M1 = sum_{c shared} (sum_i rho_i k_(c,i)) VK_c + sum_i sum_{c own} (rho_i k_(c,i)) P_(c,i)
 *        M2 = sum_i rho_i W_zeta,i + sum_i (rho_i u_i) W_omega,i,      s = sum_i rho_i y_i
 *      and the Gt value of the two literal pairs (M1 - s G1gen, G2gen) and (-M2, tau G2gen), identity pairs left out: the move of
 *      sylow_hip_kzg_batch_verify_weighted.
 * SOUNDNESS: THE LIBRARY DRAWS NO CHALLENGE.  beta, gamma, alpha, zeta AND v ARE THOSE OF THE TRANSCRIPT (sylow_plonk.h and sylow_popen.h
 * say when each is drawn).  u IS DRAWN AFTER W_zeta AND W_omega ARE FIXED and may be the verifier's own randomness.  THE WEIGHTS ARE DRAWN
 * AFTER ALL PROOFS ARE FIXED.  With u = 0 the second opening is not checked at all.
 *
 * Conventions (those of sylow_popen.h and of the KZG block of sylow_hip.h):
 *   vk_xy:       [8][2 W + 2] affine points + optional flags vk_inf [2 W + 2]: a selector that is the zero polynomial commits to the identity.
 *   proof_xy:    [8][(W + E + 3) m], slot-major: slot c of proof i at index c m + i; optional flags proof_inf [(W + E + 3) m].
 *   evals:       [4][(2 W + 1) m], EXACTLY THE LAYOUT sylow_popen_evaluate_batch WRITES; SLOT 2 W (p) IS NOT READ, so a prover's output
 *                feeds in without reshaping -- the verifier forms p itself, from pub.
 *   pub:         [4][n_pub m], input-major (input j of proof i at j m + i) as the Groth16 inputs; NULL when n_pub = 0.
 *   shifts [4][W]; beta, gamma, alpha, zeta, v, u [4][m]; tau_g2_xy [16][1].
 *   scalars:     any 256-bit words, taken mod r; outputs canonical.  Coordinate words >= p are reduced like Fp::new.  Points are taken as
 *                given (no on-curve check); tau_g2 must lie in G2 proper.  A flagged point is the identity whatever its words hold.
 *   status:      [m] bytes.  Bit 1 (0x02): zeta^n = 1, as in sylow_popen.h -- the outputs are still written by the formulas, and ok for that
 *                proof is FORCED TO 0.  No other bit is defined.
 *   calls:       stream-ordered, no host synchronisation; scratch leased per call, summed in saturating arithmetic and refused before the
 *                lease.  m = 0: nothing is launched that reads an array; the weighted call yields the identity.  SYLOW_HIP_E_ARG, nothing
 *                enqueued and nothing written, for: NULL where an array is required, log_n or log_e below 0 or log_n + log_e above 28, W
 *                outside 2 .. SYLOW_HIP_PLONK_WIRES_MAX, n_pub above n, max_blocks = 0, and any output whose bytes overlap an input's or
 *                another output's.  SYLOW_HIP_E_HIP, nothing enqueued, when the scratch limit (sylow_hip_set_scratch_limit; 1 GB by
 *                default) does not hold one proof of sylow_pverify_fold_batch.
 */
#ifndef SYLOW_PVERIFY_H
#define SYLOW_PVERIFY_H

#include "sylow_popen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Steps 1 to 3 for m proofs: k_out [4][T m], term-major (term c of proof i at c m + i) in the order of step 2, y_out [4][m], status [m],
 * all canonical.  The n_pub m denominators zeta_i - w_n^j are formed by one launch and inverted TOGETHER by the shared-inverse batch inversion
 * (sylow_hip_fr_batch_inv: one inversion per chunk of 2048, inv(0) = 0), not by a power each.  Then ONE pass, a lane per proof: zeta^n and ZH
 * by log_n squarings, L1 without an inversion (inv(n) prod_i (1 + zeta^(2^i)), as sylow_popen_linearise_batch forms it), p, A, B, the powers
 * of v and of zeta^n as running products, and the T scalars -- every load from the [4][.] planes of the challenges and of pub and every store
 * to k_out is an 8-byte word at consecutive proofs on consecutive lanes. */
/* @shape evals=u64[4*(2*W+1)*m] pub=u64[4*n_pub*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] zeta=u64[4*m] v=u64[4*m] u=u64[4*m] k_out=u64[4*(3*W+2**log_e+5)*m] y_out=u64[4*m] status=u8[m] */
int32_t sylow_pverify_scalars_batch(const uint64_t* evals, const uint64_t* pub, size_t n_pub, const uint64_t* shifts, const uint64_t* beta,
                                    const uint64_t* gamma, const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, const uint64_t* u,
                                    int32_t log_n, int32_t log_e, int32_t W, size_t m, uint64_t* k_out, uint64_t* y_out, uint8_t* status, void* stream);
/* The same with the plan pinned.  max_blocks: the blocks of a launch (>= 1, < 0 = the default).  The words do not depend on it. */
/* @shape evals=u64[4*(2*W+1)*m] pub=u64[4*n_pub*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] zeta=u64[4*m] v=u64[4*m] u=u64[4*m] k_out=u64[4*(3*W+2**log_e+5)*m] y_out=u64[4*m] status=u8[m] */
int32_t sylow_pverify_scalars_batch_tuned(const uint64_t* evals, const uint64_t* pub, size_t n_pub, const uint64_t* shifts, const uint64_t* beta,
                                          const uint64_t* gamma, const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, const uint64_t* u,
                                          int32_t log_n, int32_t log_e, int32_t W, size_t m, int64_t max_blocks, uint64_t* k_out, uint64_t* y_out,
                                          uint8_t* status, void* stream);

/* The KZG row of every proof (step 4): c_xy [8][m] + c_inf [m], pi_xy [8][m] + pi_inf [m], y_out [4][m], status [m].  C AND pi ARE
 * BIT-IDENTICAL TO sylow_hip_g1_lincomb_batch over the literal terms -- n_jobs = m and n_terms = T for C, n_terms = 2 with the scalars
 * (1, u mod r) for pi.  Per chunk of whole proofs that fits the scratch limit: the scalars; ONE gather kernel that writes the term-major
 * base and flag arrays into leased scratch (the key points replicated once per proof, the proof's points copied); then
 * sylow_hip_g1_lincomb_batch twice.  The words depend neither on the chunks nor on a plan parameter. */
/* @shape vk_xy=u64[8*(2*W+2)] vk_inf=u8[2*W+2]? proof_xy=u64[8*(W+2**log_e+3)*m] proof_inf=u8[(W+2**log_e+3)*m]? evals=u64[4*(2*W+1)*m] pub=u64[4*n_pub*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] zeta=u64[4*m] v=u64[4*m] u=u64[4*m] c_xy=u64[8*m] c_inf=u8[m] pi_xy=u64[8*m] pi_inf=u8[m] y_out=u64[4*m] status=u8[m] */
int32_t sylow_pverify_fold_batch(const uint64_t* vk_xy, const uint8_t* vk_inf, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint64_t* evals,
                                 const uint64_t* pub, size_t n_pub, const uint64_t* shifts, const uint64_t* beta, const uint64_t* gamma,
                                 const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, const uint64_t* u, int32_t log_n, int32_t log_e,
                                 int32_t W, size_t m, uint64_t* c_xy, uint8_t* c_inf, uint64_t* pi_xy, uint8_t* pi_inf, uint64_t* y_out, uint8_t* status,
                                 void* stream);

/* ok [m]: the boolean of step 4 for every proof, and status [m].  The fold into leased scratch, then
 * sylow_hip_kzg_verify_batch(tau_g2_xy, C, z = zeros, y, pi), then a small kernel that clears ok where status bit 1 is set.  The routes by
 * batch size are therefore those of sylow_hip_kzg_verify_batch, unchanged, and the flags are the same on every route. */
/* @shape tau_g2_xy=u64[16] vk_xy=u64[8*(2*W+2)] vk_inf=u8[2*W+2]? proof_xy=u64[8*(W+2**log_e+3)*m] proof_inf=u8[(W+2**log_e+3)*m]? evals=u64[4*(2*W+1)*m] pub=u64[4*n_pub*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] zeta=u64[4*m] v=u64[4*m] u=u64[4*m] ok=u8[m] status=u8[m] */
int32_t sylow_pverify_verify_batch(const uint64_t* tau_g2_xy, const uint64_t* vk_xy, const uint8_t* vk_inf, const uint64_t* proof_xy, const uint8_t* proof_inf,
                                   const uint64_t* evals, const uint64_t* pub, size_t n_pub, const uint64_t* shifts, const uint64_t* beta,
                                   const uint64_t* gamma, const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v, const uint64_t* u, int32_t log_n,
                                   int32_t log_e, int32_t W, size_t m, uint8_t* ok, uint8_t* status, void* stream);

/* The weighted form (step 5): weights [4][m], gt_out [48][1] and is_one [1], either of which may be NULL, not both, and status [m].  The
 * scalars of all m proofs; ONE kernel that forms rho_i k for the proof's own terms, rho_i and rho_i u_i, and the partial sums of the 2 W + 2
 * key columns and of s per block, and a second that joins them (the two levels of sylow_hip_kzg_batch_verify_weighted); sylow_hip_g1_msm over
 * the (W + E + 3) m own terms, read IN PLACE from proof_xy, and over the 2 m opening points; sylow_hip_g1_lincomb_batch (n_jobs = 1) over
 * the 2 W + 2 key points; one sylow_hip_g1_add_batch; sylow_hip_g1_generator_mul_batch for s and one sylow_hip_g1_sub_batch; the pair
 * list; and sylow_hip_pairing_product_batch with skip_infinity = 1.  A weight of 0 mod r removes a proof.  A proof whose status bit 1 is set makes
 * is_one 0 unless its weight is 0 mod r; gt_out is the value of the formulas either way.  m = 0: the identity, is_one = 1. */
/* @shape tau_g2_xy=u64[16] vk_xy=u64[8*(2*W+2)] vk_inf=u8[2*W+2]? proof_xy=u64[8*(W+2**log_e+3)*m] proof_inf=u8[(W+2**log_e+3)*m]? evals=u64[4*(2*W+1)*m] pub=u64[4*n_pub*m]? shifts=u64[4*W] beta=u64[4*m] gamma=u64[4*m] alpha=u64[4*m] zeta=u64[4*m] v=u64[4*m] u=u64[4*m] weights=u64[4*m] gt_out=u64[48]? is_one=u8[1]? status=u8[m] */
int32_t sylow_pverify_batch_verify_weighted(const uint64_t* tau_g2_xy, const uint64_t* vk_xy, const uint8_t* vk_inf, const uint64_t* proof_xy,
                                            const uint8_t* proof_inf, const uint64_t* evals, const uint64_t* pub, size_t n_pub, const uint64_t* shifts,
                                            const uint64_t* beta, const uint64_t* gamma, const uint64_t* alpha, const uint64_t* zeta, const uint64_t* v,
                                            const uint64_t* u, const uint64_t* weights, int32_t log_n, int32_t log_e, int32_t W, size_t m,
                                            uint64_t* gt_out, uint8_t* is_one, uint8_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_PVERIFY_H */
