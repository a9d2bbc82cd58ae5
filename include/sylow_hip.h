/*
 * sylow_hip.h -- C ABI of the MI355X-native batched BN254 pairing / BLS-verify engine.
 *
 * This is the drop-in boundary for the one data-parallel hot path of warlock-labs/sylow
 * (src/fields -> src/groups -> src/pairing.rs -> src/svdw.rs / src/hasher.rs -> lib.rs
 * sign/verify).  The reference has no FFI of its own (100 % safe Rust, `deny(unsafe_code)`,
 * src/lib.rs:63); each entry point below names the reference item whose *batched* form it
 * computes, i.e. what a `sylow-hip` Rust shim binds with `extern "C"`.
 *
 * Conventions
 *  - Every array argument is a DEVICE pointer (hipMalloc / sylow_hip_malloc / a torch tensor's
 *    data_ptr()).  Nothing here takes torch types.
 *  - Field elements cross the boundary as canonical integers in [0, p) (what sylow's
 *    `Fp::value().to_words()` yields, src/fields/fp.rs:232-234): 4 little-endian uint64 limbs.
 *    Inputs >= p are reduced mod p exactly like `Fp::new` (fp.rs:199-201).
 *  - Struct-of-arrays, word-major: a batch of n objects made of W 64-bit words is a uint64
 *    array of shape [W][n]; word w of element i is at base[w * n + i].  Word order inside an
 *    object is the reference's nesting order, least-significant limb first:
 *      Fp   : W =  4  (limb0..limb3)
 *      Fp2  : W =  8  (c0 limbs, c1 limbs)                      fields/fp2.rs
 *      Fp6  : W = 24  (c0.c0, c0.c1, c1.c0, c1.c1, c2.c0, c2.c1) fields/fp6.rs
 *      Fp12 : W = 48  (c0 as Fp6, c1 as Fp6)  == Gt             fields/fp12.rs, groups/gt.rs
 *      G1 affine    : W =  8 (x, y)      + uint8 infinity flag array (may be NULL = none)
 *      G2 affine    : W = 16 (x.c0, x.c1, y.c0, y.c1) + uint8 infinity flag array
 *      G1 projective: W = 12 (x, y, z);  G2 projective: W = 24
 *    The canonical affine encoding of the identity is (0, 1, inf=1) (groups/group.rs:271-277).
 *  - Memory: a call reads and writes only the extents the `@shape` line in front of its prototype gives (name=type[elements], `?` = may
 *    be NULL): it never touches a byte outside them, so a neighbouring buffer is safe (alignment aside: only pointers as aligned as
 *    hipMalloc's are tested).  On success every element of every output array is written, whatever
 *    the buffer held before: flags and status bytes that are 0, identity rows as (0, 1), outputs of rows that failed.  Arrays declared
 *    `const` are not modified.  (tests/test_gpu_memory_contract.py runs every entry point between guard bands under two fill patterns.)
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *    asynchronous on that stream; use sylow_hip_stream_sync or your own events.
 *  - Threads: entry points may be called concurrently from several host threads and on several streams.  The
 *    few calls that need device scratch (pairing_product*, fp12_product_final_exp, evm_ecpairing,
 *    bls_verify_same_signer, *_all) lease a private block per call; blocks are recycled in stream order through
 *    HIP events, never by synchronising a stored stream handle.
 *  - Return value: 0 on success, negative SYLOW_HIP_E_* otherwise.  No call throws or aborts.
 *    Per-element failures are reported through `status` byte arrays using codes that mirror
 *    sylow's GroupError (groups/group.rs:38-47).
 */
#ifndef SYLOW_HIP_H
#define SYLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYLOW_HIP_OK 0
#define SYLOW_HIP_E_HIP (-1)      /* a HIP runtime call failed; see sylow_hip_last_error() */
#define SYLOW_HIP_E_ARG (-2)      /* bad argument (NULL pointer, n == 0 where not allowed, ...) */
#define SYLOW_HIP_E_NO_DEVICE (-3)

/* per-element status codes (mirror GroupError, groups/group.rs:38-47) */
#define SYLOW_HIP_ST_OK 0
#define SYLOW_HIP_ST_NOT_ON_CURVE 1
#define SYLOW_HIP_ST_NOT_IN_SUBGROUP 2
#define SYLOW_HIP_ST_CANNOT_HASH 3
#define SYLOW_HIP_ST_DECODE_ERROR 4

/* ---- runtime ------------------------------------------------------------------------------ */
int32_t sylow_hip_init(int32_t device);                 /* hipSetDevice + arch check (gfx950) */
/* One process driving several GPUs: checks every listed device (gfx950) and makes device_ids[0] current.  All per-device
 * state (scratch workspace, generator line tables) is created lazily on the device that is current when a call needs it. */
int32_t sylow_hip_init_devices(const int32_t* device_ids, int32_t n_dev);
/* Launches go to the CALLING THREAD's current HIP device.  Hosts that switch devices (or share the process with code that
 * does) call this before a batch of entry points; pointers passed to a call must belong to that device. */
int32_t sylow_hip_set_device(int32_t device);
/* Frees every scratch block, completion event and generator table on every device (after a device synchronise).  The library
 * stays usable: state is rebuilt on demand.  EXCLUSIVE: while another host thread is inside an entry point that holds a scratch
 * block the call frees nothing and returns SYLOW_HIP_E_ARG. */
int32_t sylow_hip_shutdown(void);
/* Frees the current device's idle scratch blocks larger than keep_bytes whose last user has completed (blocks grow with the largest
 * batch seen and are otherwise kept for reuse until sylow_hip_shutdown).  Never touches a block that is in use and does not hold the
 * library's lock while the driver frees (hipFree may wait for the device: the CALLER can block, other host threads' entry points do not). */
int32_t sylow_hip_trim(size_t keep_bytes);
/* Bounds the one scratch user whose size is NOT proportional to its input: the line tables of the multi-pair routes (multi_pairing_batch,
 * glued_miller_loop_batch, evm_ecpairing_batch with >= 2 pairs per job, pairing_product*, the aggregate verifiers; 19.5 KB per pair, by
 * default as many whole rounds of 2^16 jobs as fit 12 GB).  With a limit the job slices shrink to what fits (slower below one round of
 * k-slot jobs = 1.28 GB * k: the table-driven loop then runs under-filled), and a batch-wide product whose chunks no longer fit takes the
 * in-register schedule (no table at all, ~25 % more Miller-loop work).  The limit also bounds sylow_hip_g1_msm's working set (default
 * 1 GB): its points then go through in chunks that fit.  Below one chunk of 256 points it takes its per-point route, whose scratch
 * (about 161 bytes per point plus the scalar multiplication's window tables) the limit does NOT bound.  Results are identical for every
 * limit.  0 restores the default.
 * Process-wide; takes effect at the next call. */
int32_t sylow_hip_set_scratch_limit(size_t bytes);
/* Route selectors and thresholds (A/B measurements, crossover runs, forcing a route in a test).  Process-wide, read at every call; a value
 * < 0 restores the default.  The LIBRARY reads no environment variable (rounds 1-5 did: eight getenv switches behind this ABI); a host
 * that wants SYLOW_HIP_* variables reads them itself and calls this (sylow_amd/_lib.py does).  Results are identical
 * under every setting.
 *   STAGGER          1 (default) skewed launches of pairing_batch / bls_verify_batch at >= 2 rounds, 0 plain launches, 2 the skew with the
 *                    parking blocks' flags muted (every finishing block takes its recompute fallback)
 *   MULTI_TABLES     default: jobs of >= 2 pairs on average go through line tables in HBM; 0 never, 1 always
 *   WIDE_TAIL        1 (default) one-wavefront-per-element kernels for small batches and single tails, 0 never
 *   WIDE_PACK        two elements per wavefront in those kernels above this many elements (default: the CU count; 0 never, 1 always)
 *   AGG_FORK         1 (default) the aggregate verifiers fork the signature half onto a side stream, 0 one stream
 *   SIGN_WIDE_MAX    largest batch signed / hashed / multiplied on eight lanes per element (default 16384)
 *   WIDE_MAX         largest batch of pairings on the one-wavefront route (default 6144)
 *   WIDE_VERIFY_MAX  largest batch of verifications on it (default 4096)
 *   QUAD_MAX         largest batch of pairings / Miller loops / final exponentiations / verifications on one lane QUAD per element
 *                    (plk_quad.hip; default: 64 x the CU count = 16384, one wavefront per SIMD; 0 never)
 *   TAIL_SPLIT       1 (default) a batch of one or two whole rounds of one wavefront per SIMD (128 x the CU count = 32768 elements each) plus a
 *                    tail that fits the quad route runs the tail on quads on a side stream beside the rounds, 0 one launch */
#define SYLOW_HIP_OPT_STAGGER 0
#define SYLOW_HIP_OPT_MULTI_TABLES 1
#define SYLOW_HIP_OPT_WIDE_TAIL 2
#define SYLOW_HIP_OPT_WIDE_PACK 3
#define SYLOW_HIP_OPT_AGG_FORK 4
#define SYLOW_HIP_OPT_SIGN_WIDE_MAX 5
#define SYLOW_HIP_OPT_WIDE_MAX 6
#define SYLOW_HIP_OPT_WIDE_VERIFY_MAX 7
#define SYLOW_HIP_OPT_QUAD_MAX 8
#define SYLOW_HIP_OPT_TAIL_SPLIT 9
#define SYLOW_HIP_OPT_COUNT 10
int32_t sylow_hip_set_option(int32_t option, int64_t value);
/* @shape value_host=i64[1] */
int32_t sylow_hip_get_option(int32_t option, int64_t* value_host);      /* HOST pointer; -1 = the default is in force */
/* Live clock probe of the metric's kernels (plk::k_pairing, plk::k_bls_verify_fused, and their lane-quad forms for mid-size batches).  `acc` = 256 uint64 words of DEVICE memory, zeroed
 * by the caller (NULL switches the probe off; the default).  While set, every wavefront of those kernels reads the shader-clock counter
 * (s_memtime) and the constant-rate counter (s_memrealtime) when it starts and when it ends and adds, with relaxed device-scope atomics, into
 * slot s = blockIdx % 64:  acc[4 s] += shader-clock ticks, acc[4 s + 1] += constant-rate ticks, acc[4 s + 2] += 1 (wavefronts),
 * acc[4 s + 3] = max(constant-rate ticks of one wavefront).  sum(acc[4 s]) / sum(acc[4 s + 1]) x the constant rate
 * (sylow_hip_wall_clock_khz) is the engine clock those wavefronts ran at, weighted by residency: what bench.py reports as
 * roofline.sustained_mhz.  Process-wide: one accumulator for whichever launches follow, so it must be memory of the device those launches run
 * on (a host that drives several GPUs from one process probes one device at a time); the pointer must stay valid until the probe is switched off
 * and the stream is drained. */
/* @shape acc=u64[256]? */
int32_t sylow_hip_clock_probe(uint64_t* acc);
/* @shape khz_host=i32[1] */
int32_t sylow_hip_wall_clock_khz(int32_t* khz_host);                    /* HOST pointer: rate of s_memrealtime on the current device */
const char* sylow_hip_last_error(void);
int32_t sylow_hip_device_count(void);
int32_t sylow_hip_malloc(void** dptr, size_t bytes);
int32_t sylow_hip_free(void* dptr);
int32_t sylow_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int32_t sylow_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int32_t sylow_hip_stream_sync(void* stream);
/* Synthetic inputs: n draws of the SplitMix64-seeded xoshiro256** stream, each 256 bits (four outputs, least-significant
 * word first) masked to 254 bits and rejection-sampled to < p (Fp::rand's role for benches and tests).
 * HOST function: out_host is a HOST array in the SoA layout [4][stride] (stride >= n). */
/* @shape out_host=u64[3*stride+n] */
int32_t sylow_hip_host_xoshiro_fp(uint64_t seed, uint64_t* out_host, size_t n, size_t stride);
/* layout helpers for hosts that hold array-of-structs ([n][W], e.g. a Rust Vec<[u64; 4]>) */
/* @shape aos=u64[words*n] soa=u64[words*n] */
int32_t sylow_hip_aos_to_soa(const uint64_t* aos, uint64_t* soa, size_t words, size_t n, void* stream);
/* @shape soa=u64[words*n] aos=u64[words*n] */
int32_t sylow_hip_soa_to_aos(const uint64_t* soa, uint64_t* aos, size_t words, size_t n, void* stream);

/* ---- Fp: src/fields/fp.rs ----------------------------------------------------------------- */
/* Add / Sub / Mul / Neg / square / Inv for &Fp (fp.rs:304-310, 340-347, 387-393, 442-449,
 * 620-622, 418-433).  inv(0) = 0, no error (fp.rs:1126-1132). */
/* @shape a=u64[4*n] b=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fp_add_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] b=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fp_sub_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] b=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fp_mul_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fp_sqr_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fp_neg_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fp_inv_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* Fp::pow(U256) (fp.rs:451-457), per-element exponents e [4][n] */
/* @shape a=u64[4*n] e=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fp_pow_batch(const uint64_t* a, const uint64_t* e, uint64_t* out, size_t n, void* stream);
/* Fp::sqrt (fp.rs:611-616): out = a^((p+1)/4), is_some[i] = (out_i^2 == a_i), i.e. the CtOption's value and flag */
/* @shape a=u64[4*n] out=u64[4*n] is_some=u8[n] */
int32_t sylow_hip_fp_sqrt_batch(const uint64_t* a, uint64_t* out, uint8_t* is_some, size_t n, void* stream);
/* Fp::is_square (fp.rs:625-631): 1 for squares and for 0 */
/* @shape a=u64[4*n] flags=u8[n] */
int32_t sylow_hip_fp_is_square_batch(const uint64_t* a, uint8_t* flags, size_t n, void* stream);
/* Fp::from_be_bytes / Fr::from_be_bytes (fp.rs:686-719, 746-778) = CtOption::new(Self::new(v), v < modulus) on 32 big-endian
 * bytes per element, in [n][32]: out [4][n] receives the value (v mod modulus, like Self::new) and status[i] the flag --
 * OK, or DECODE_ERROR where the reference's CtOption is none (v >= p resp. v >= r).  to_be_bytes (fp.rs:727-737) writes the
 * canonical value, out [n][32]. */
/* @shape in=u8[32*n] out=u64[4*n] status=u8[n] */
int32_t sylow_hip_fp_from_be_bytes_batch(const uint8_t* in, uint64_t* out, uint8_t* status, size_t n, void* stream);
/* @shape in=u8[32*n] out=u64[4*n] status=u8[n] */
int32_t sylow_hip_fr_from_be_bytes_batch(const uint8_t* in, uint64_t* out, uint8_t* status, size_t n, void* stream);
/* @shape a=u64[4*n] out=u8[32*n] */
int32_t sylow_hip_fp_to_be_bytes_batch(const uint64_t* a, uint8_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] out=u8[32*n] */
int32_t sylow_hip_fr_to_be_bytes_batch(const uint64_t* a, uint8_t* out, size_t n, void* stream);

/* ---- Fr, the r-torsion scalar field (fields/fp.rs:556-565: the same macro-generated API as Fp, modulus r) -----------
 * Same contract as the Fp calls: [4][n] canonical limbs in and out, any 256-bit input accepted like Fr::new,
 * inv(0) = 0.  Used by Lagrange interpolation / polynomial evaluation (examples/threshold_signing.rs:64-70,146-155). */
/* @shape a=u64[4*n] b=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fr_add_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] b=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fr_sub_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] b=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fr_mul_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fr_sqr_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fr_neg_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fr_inv_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);

/* ---- Fr: inverses that share one inversion (kzg_evals.hip; geometry in kzg_evals_plan.hpp) ------------------------------------------------
 * out_i = a_i^-1 mod r by Montgomery's trick: a [4][n] and out [4][n] as above, any 256-bit words taken mod r, canonical words out,
 * inv(0) = 0 -- an element = 0 mod r yields 0 and does not disturb its neighbours (it enters the product chain as 1).  The words are
 * bit-equal to what sylow_hip_fr_inv_batch writes (the inverse is unique); that call pays a power a^(r-2), about 380 products, per element,
 * this one about 5 products per element and ONE inversion per chunk of 2048 elements: a lane owns 8 consecutive elements, a block a chunk,
 * prefix and suffix products inside the lane and through LDS, and the chunk's product is inverted on one lane by the binary extended
 * Euclidean algorithm.  ONE launch, no scratch, stream-ordered, no host synchronisation.  n = 0: OK, nothing launched, nothing written.
 * SYLOW_HIP_E_ARG, no launch, nothing written, for: NULL a or out; out overlapping a (the two byte ranges of 32 n bytes are compared: the
 * elements are read twice). */
/* @shape a=u64[4*n] out=u64[4*n] */
int32_t sylow_hip_fr_batch_inv(const uint64_t* a, uint64_t* out, size_t n, void* stream);

/* ---- Fr: transforms on radix-2 domains (ntt.hip; geometry, ping-pong and scratch in ntt_plan.hpp) ---------------------------------------
 * r - 1 = 2^28 * odd, so Fr holds the domains of n = 2^log_n points for 0 <= log_n <= 28, generated by w_n = W^(2^(28 - log_n)) with
 * W = 5^((r - 1) / 2^28) = 0x2a3c09f0a58a7e8500e0a7eb8ef62abc402d111e41112ed49bd61b6e725b19f0 (the root arkworks, gnark and snarkjs use).
 * Natural order in, natural order out; the optional coset shift is g (shift = NULL: g = 1):
 *   forward (inverse = 0):  out_i = sum_k a_k (g w_n^i)^k         -- the values of the polynomial a on the coset g <w_n>
 *   inverse (inverse = 1):  out_k = n^-1 g^-k sum_i a_i w_n^(-ik)  -- the coefficients from those values
 * Conventions (those of the KZG prover block below):
 *   arrays:    in and out are [m][4][n]: m Fr SoA arrays one after another, word w of element k of array j at (j * 4 + w) * n + k -- the layout of
 *              `coeffs`.  shift is [4] device words.
 *   scalars:   inputs and shift are ANY 256-bit words, taken mod r; outputs are canonical words below r.
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call (the table w_n^e, e < n/2, is built per call: 16 n bytes; a
 *              transform of more than one step also leases one buffer of the size of `out`).  m = 0: OK, nothing launched, nothing written.
 *   errors:    SYLOW_HIP_E_ARG, no launch, nothing written, for: NULL in or out; log_n < 0 or > 28; inverse not 0 or 1; out overlapping in
 *              (the two byte ranges of 32 n m bytes are compared); for the _tuned form stages == 0 or stages > 10.
 *   inverse with shift = 0 mod r: g^-1 is the library's inv(0) = 0, so out_0 = n^-1 sum_i a_i and every other out_k = 0.
 * One launch builds the table, one more per pass, and one element-wise launch (c s^k a_k) carries the forward shift or the inverse's scale:
 * a pass is a radix-2^s step (Stockham autosort, s <= 10 stages in LDS, 5 by default), so a transform of log_n <= 5 has ONE pass and a
 * longer one ceil(log_n / 5); no bit-reversal launch.  log_n is an int32_t like every other small integer of this header. */
/* @shape in=u64[4*2**log_n*m] shift=u64[4]? out=u64[4*2**log_n*m] */
int32_t sylow_hip_fr_ntt_batch(const uint64_t* in, int32_t log_n, size_t m, int32_t inverse, const uint64_t* shift, uint64_t* out, void* stream);
/* The same with the stages of a pass pinned: 1 .. 10 (NTT_STAGES_MAX of ntt_plan.hpp), < 0 = the default (5).  The last pass takes what is left
 * of log_n.  The values do not depend on it. */
/* @shape in=u64[4*2**log_n*m] shift=u64[4]? out=u64[4*2**log_n*m] */
int32_t sylow_hip_fr_ntt_batch_tuned(const uint64_t* in, int32_t log_n, size_t m, int32_t inverse, const uint64_t* shift, int32_t stages,
                                     uint64_t* out, void* stream);

/* ---- G1: transforms on radix-2 domains (g1_ntt.hip; butterflies, grids, ping-pong and scratch in g1_ntt_plan.hpp) ----------------------------
 * The discrete Fourier transform of the block above with G1 POINTS as elements and the same roots w_n as twiddles, natural order in and out:
 *   forward (inverse = 0):  out_i = sum_k w_n^(ik) P_k
 *   inverse (inverse = 1):  out_k = n^-1 sum_i w_n^(-ik) P_i
 * so for P_k = s_k G the output is NTT(s)_i G.  There is NO coset shift: transforms on a coset g <w_n> are out of scope.
 *   arrays:    p_xy and out_xy are [m][8][n], n = 2^log_n, 0 <= log_n <= 28: m affine SoA arrays one after another, word w of point k of
 *              array j at (j * 8 + w) * n + k.  p_inf is [m][n] bytes, optional (NULL = nothing flagged); out_inf is [m][n], required.
 *   points:    taken as given, no on-curve check.  A flagged input is the identity whatever its words hold, and so is the pair (0, 1) that
 *              every call writes for the identity, with or without its flag ((0, 1) is no point of the curve).  Outputs are the canonical
 *              affine words of a group element, the identity as (0, 1) + its flag: they do NOT depend on the plan (max_blocks below).
 *              At log_n = 0 the output is the input point made canonical, in both directions.
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call: two projective buffers of 96 n m bytes (one at log_n = 1,
 *              none at 0), the twiddle table of 16 n bytes, and window tables of 1 KB per RESIDENT lane (at most 512 blocks of 256 lanes
 *              by default: 128 MB, whatever n is).  A lease that does not fit returns SYLOW_HIP_E_HIP.  m = 0: OK, nothing launched,
 *              nothing written.
 *   errors:    SYLOW_HIP_E_ARG, no launch, nothing written, for: NULL p_xy, out_xy or out_inf; log_n < 0 or > 28; inverse not 0 or 1;
 *              out_xy overlapping p_xy (the two byte ranges of 64 n m bytes are compared); out_inf overlapping p_inf (n m bytes);
 *              max_blocks == 0.
 * One launch builds the twiddle table (log_n >= 2), one per radix-2 Stockham stage (log_n of them; a butterfly (U, V) -> (U + kV, U - kV) is
 * one scalar multiplication, skipped where k = 1: all of the first stage, one butterfly in 2^p of stage p), and ONE closing launch scales
 * by n^-1 (inverse) and converts to affine, one Fp inversion per point. */
/* @shape p_xy=u64[8*2**log_n*m] p_inf=u8[2**log_n*m]? out_xy=u64[8*2**log_n*m] out_inf=u8[2**log_n*m] */
int32_t sylow_hip_g1_ntt_batch(const uint64_t* p_xy, const uint8_t* p_inf, int32_t log_n, size_t m, int32_t inverse,
                               uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* The same with the blocks of a stage launch capped: max_blocks >= 1 (at most 4096; more is 4096), < 0 = the default (512).  Lanes walk the
 * butterflies beyond the grid with a grid stride, and the window tables are max_blocks * 256 KB.  The values do not depend on it. */
/* @shape p_xy=u64[8*2**log_n*m] p_inf=u8[2**log_n*m]? out_xy=u64[8*2**log_n*m] out_inf=u8[2**log_n*m] */
int32_t sylow_hip_g1_ntt_batch_tuned(const uint64_t* p_xy, const uint8_t* p_inf, int32_t log_n, size_t m, int32_t inverse, int64_t max_blocks,
                                     uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* The Lagrange-basis KZG SRS from the monomial one: srs_g1_xy [8][n] = tau^k G1gen, no flag array; out_xy [8][n] and out_inf [n] (required)
 * = L_i(tau) G1gen = n^-1 sum_k w_n^(-ik) tau^k G1gen -- the inverse transform above with m = 1, and its errors.  A SET FLAG means that tau
 * lies in the domain (some L_i(tau) = 0): such an SRS is unusable.  The output, fed to sylow_hip_kzg_commit_batch or
 * sylow_hip_kzg_open_evals_batch, gives word for word what the monomial SRS gives through sylow_hip_kzg_commit_evals_batch or
 * sylow_hip_kzg_open_batch on the interpolated coefficients; the forward transform takes it back to the monomial SRS. */
/* @shape srs_g1_xy=u64[8*2**log_n] out_xy=u64[8*2**log_n] out_inf=u8[2**log_n] */
int32_t sylow_hip_kzg_srs_lagrange(const uint64_t* srs_g1_xy, int32_t log_n, uint64_t* out_xy, uint8_t* out_inf, void* stream);

/* ---- extension tower (test hooks): fields/fp2.rs:285-306,164-171,355-360; fp6.rs:283-367,
 * 415-423; fp12.rs:229-238,536-550,281-286,515-522,426-503 ------------------------------------ */
/* FieldExtension<D, N, F> component-wise operators (fields/extensions.rs:67-238): Add / Sub / Neg and scale by a base-field
 * element, for Fp2 / Fp6 / Fp12 batches: degree = 2, 6 or 12 Fp coefficients, arrays [4 * degree][n]; the scale factor k is one Fp
 * per element, [4][n]. */
/* @shape a=u64[4*degree*n] b=u64[4*degree*n] out=u64[4*degree*n] */
int32_t sylow_hip_fext_add_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, int32_t degree, size_t n, void* stream);
/* @shape a=u64[4*degree*n] b=u64[4*degree*n] out=u64[4*degree*n] */
int32_t sylow_hip_fext_sub_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, int32_t degree, size_t n, void* stream);
/* @shape a=u64[4*degree*n] out=u64[4*degree*n] */
int32_t sylow_hip_fext_neg_batch(const uint64_t* a, uint64_t* out, int32_t degree, size_t n, void* stream);
/* @shape a=u64[4*degree*n] k=u64[4*n] out=u64[4*degree*n] */
int32_t sylow_hip_fext_scale_batch(const uint64_t* a, const uint64_t* k, uint64_t* out, int32_t degree, size_t n, void* stream);
/* @shape a=u64[8*n] b=u64[8*n] out=u64[8*n] */
int32_t sylow_hip_fp2_mul_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[8*n] out=u64[8*n] */
int32_t sylow_hip_fp2_sqr_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[8*n] out=u64[8*n] */
int32_t sylow_hip_fp2_inv_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[24*n] b=u64[24*n] out=u64[24*n] */
int32_t sylow_hip_fp6_mul_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[24*n] out=u64[24*n] */
int32_t sylow_hip_fp6_inv_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* The small tower items the pairing composes, as entry points of their own: Fp2::residue_mul (x (9 + u), fp2.rs:99-107),
 * Fp2::frobenius(exponent) (fp2.rs:119-133: conjugation for odd exponents), Fp6::square (fp6.rs:213-236), Fp6::residue_mul
 * (x v, fp6.rs:189-192), Fp6::frobenius(exponent) (fp6.rs:205-211: any exponent, tables indexed mod 6) */
/* @shape a=u64[8*n] out=u64[8*n] */
int32_t sylow_hip_fp2_residue_mul_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[8*n] out=u64[8*n] */
int32_t sylow_hip_fp2_frobenius_batch(const uint64_t* a, uint64_t exponent, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[24*n] out=u64[24*n] */
int32_t sylow_hip_fp6_sqr_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[24*n] out=u64[24*n] */
int32_t sylow_hip_fp6_residue_mul_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[24*n] out=u64[24*n] */
int32_t sylow_hip_fp6_frobenius_batch(const uint64_t* a, uint64_t exponent, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[48*n] b=u64[48*n] out=u64[48*n] */
int32_t sylow_hip_fp12_mul_batch(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[48*n] out=u64[48*n] */
int32_t sylow_hip_fp12_sqr_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[48*n] out=u64[48*n] */
int32_t sylow_hip_fp12_inv_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* Fp12::frobenius(exponent), exponent in {1,2,3} (the ones the pairing uses) */
/* @shape a=u64[48*n] out=u64[48*n] */
int32_t sylow_hip_fp12_frobenius_batch(const uint64_t* a, int32_t exponent, uint64_t* out, size_t n, void* stream);
/* Fp12::sparse_mul(ell_0, ell_vw, ell_vv): ell is [24][n] = (ell_0, ell_vw, ell_vv) as Fp2 each */
/* @shape f=u64[48*n] ell=u64[24*n] out=u64[48*n] */
int32_t sylow_hip_fp12_sparse_mul_batch(const uint64_t* f, const uint64_t* ell, uint64_t* out, size_t n, void* stream);

/* test hook for the carry-free 9 x 29-bit core used inside the final exponentiation (csrc/bn254_f29.hpp):
 * op 0: round trip; 1: a*b; 2: 2ab via the fused two-product pass; 3: 2a(b-a) through lazy add/sub + normalise */
/* @shape a=u64[*] b=u64[*]? out=u64[*] */
int32_t sylow_hip_f29_hook_batch(int32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);
/* test hook for the same core on RAW limbs: operands are [9][n] int32 limb planes, applied exactly as given (no conversion).
 * op 0: norm(a); 1: norm_x8(a); 2: norm_sub3(a, b); 3: mul(a, b) inlined; 4: mul(a, b) through the out-of-line leaf; 5: sqr(a);
 * 6: dot2(a, b, c, d); 7: dot2_ilp(a, b, c, d); 8: reduce_from(limb(i) = k0 a[i] + k1 b[i]); 9: reduce_terms(a, b; k0, k1);
 * 10: reduce_terms(a, b, c, d; four 16-bit coefficients, k0 = k[0] | k[1] << 16, k1 = k[2] | k[3] << 16); 11: norm_terms(a, b; k0, k1);
 * 12: norm_terms as op 10; 13: u2_xi_lin(x = (a, b), k0, y = (c, d), k1), out [18][n]; 14: to_fp(a), out = 8 u32 words and a zero
 * word; 15: from_fp(a[0..7] as u32 words).  Out [9][n] except op 13. */
/* @shape a=i32[9*n] b=i32[9*n]? c=i32[9*n]? d=i32[9*n]? out=i32[*] */
int32_t sylow_hip_f29_raw_hook_batch(int32_t op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t k0,
                                     int32_t k1, int32_t* out, size_t n, void* stream);

/* ---- groups: src/groups/group.rs, g1.rs, g2.rs ----------------------------------------------- */
/* Mul<&Fp> for &G1Projective / &G2Projective (group.rs:639-667): out_i = k_i * P_i.
 * Points affine in (+ optional infinity flags), affine out + infinity flags (comparison is by
 * affine normalisation).  Scalars are Fp VALUES (k < p, not reduced mod r, N4). */
/* @shape p_xy=u64[8*n] p_inf=u8[n]? k=u64[4*n] out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_g1_scalar_mul_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k,
                                      uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* @shape p_xy=u64[16*n] p_inf=u8[n]? k=u64[4*n] out_xy=u64[16*n] out_inf=u8[n] */
int32_t sylow_hip_g2_scalar_mul_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k,
                                      uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* The same product for points of G2 proper (the r-torsion) -- every G2Projective the reference lets a caller build
 * (G2Projective::new checks membership, g2.rs:460-525; from_be_bytes, generator multiples, sums): the scalar is split
 * four ways along the endomorphism psi (g2.rs:140-152), ~1.8x faster, same affine result.  PRECONDITION: p_i in the r-torsion
 * (sylow_hip_g2_subgroup_check_batch / g2_from_be_bytes_batch establish it); for other points of the twist use
 * sylow_hip_g2_scalar_mul_batch, which is exact on the whole curve. */
/* @shape p_xy=u64[16*n] p_inf=u8[n]? k=u64[4*n] out_xy=u64[16*n] out_inf=u8[n] */
int32_t sylow_hip_g2_scalar_mul_subgroup_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k,
                                               uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* G2Projective::generator() * k_i for a batch of scalars -- the public half of KeyPair::generate (lib.rs:131-137): a fixed-base
 * table of the generator (built once per device, 590 KB) turns the product into 32 additions, no doublings; same affine result
 * as sylow_hip_g2_scalar_mul_batch on the generator. */
/* @shape k=u64[4*n] out_xy=u64[16*n] out_inf=u8[n] */
int32_t sylow_hip_g2_generator_mul_batch(const uint64_t* k, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* The same for G1Projective::generator() * k_i (GroupTrait::rand, test data): 295 KB table, 32 additions. */
/* @shape k=u64[4*n] out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_g1_generator_mul_batch(const uint64_t* k, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* Add for &G1Projective (group.rs:528-599) on affine inputs, affine output */
/* @shape a_xy=u64[8*n] a_inf=u8[n]? b_xy=u64[8*n] b_inf=u8[n]? out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_g1_add_batch(const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                               uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* Add for &G2Projective, GroupProjective::double for G1 / G2 (group.rs:528-599, 339-386), affine in / out */
/* @shape a_xy=u64[16*n] a_inf=u8[n]? b_xy=u64[16*n] b_inf=u8[n]? out_xy=u64[16*n] out_inf=u8[n] */
int32_t sylow_hip_g2_add_batch(const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                               uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* Sub for &G1Projective / &G2Projective (group.rs:614-624: self + (-other)), affine in / out */
/* @shape a_xy=u64[8*n] a_inf=u8[n]? b_xy=u64[8*n] b_inf=u8[n]? out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_g1_sub_batch(const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                               uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* @shape a_xy=u64[16*n] a_inf=u8[n]? b_xy=u64[16*n] b_inf=u8[n]? out_xy=u64[16*n] out_inf=u8[n] */
int32_t sylow_hip_g2_sub_batch(const uint64_t* a_xy, const uint8_t* a_inf, const uint64_t* b_xy, const uint8_t* b_inf,
                               uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* G1Projective::new([x, y, z]) (g1.rs:383-402) and G2Projective::new([x, y, z]) (g2.rs:460-525) on projective SoA input
 * ([12][n] / [24][n]): status OK / NOT_ON_CURVE / NOT_IN_SUBGROUP (G2 only); Z = 0 is accepted as the reference does.  Where the
 * reference panics (an off-curve G2 input reaches endomorphism(), g2.rs:151) the status is NOT_ON_CURVE. */
/* @shape p_xyz=u64[12*n] status=u8[n] */
int32_t sylow_hip_g1_projective_new_batch(const uint64_t* p_xyz, uint8_t* status, size_t n, void* stream);
/* @shape p_xyz=u64[24*n] status=u8[n] */
int32_t sylow_hip_g2_projective_new_batch(const uint64_t* p_xyz, uint8_t* status, size_t n, void* stream);
/* ConstantTimeEq / PartialEq for projective points (group.rs:426-447): eq[i] = 1 iff both are the identity, or neither is and
 * the cross-multiplied coordinates agree.  a, b projective SoA [12][n] / [24][n]. */
/* @shape a_xyz=u64[12*n] b_xyz=u64[12*n] eq=u8[n] */
int32_t sylow_hip_g1_ct_eq_batch(const uint64_t* a_xyz, const uint64_t* b_xyz, uint8_t* eq, size_t n, void* stream);
/* @shape a_xyz=u64[24*n] b_xyz=u64[24*n] eq=u8[n] */
int32_t sylow_hip_g2_ct_eq_batch(const uint64_t* a_xyz, const uint64_t* b_xyz, uint8_t* eq, size_t n, void* stream);
/* @shape a_xy=u64[8*n] a_inf=u8[n]? out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_g1_double_batch(const uint64_t* a_xy, const uint8_t* a_inf, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* @shape a_xy=u64[16*n] a_inf=u8[n]? out_xy=u64[16*n] out_inf=u8[n] */
int32_t sylow_hip_g2_double_batch(const uint64_t* a_xy, const uint8_t* a_inf, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* Weighted aggregation sum_i k_{j,i} * P_{j,i} (examples/threshold_signing.rs:124-143: partial signatures times
 * Lagrange coefficients), n_jobs independent sums of n_terms terms each.  p_xy [8][n_jobs*n_terms], k [4][n_jobs*n_terms]
 * (Fr / Fp values), term-major: element (job j, term i) is at index i*n_jobs + j.  out [8][n_jobs] affine + flags.
 * n_terms = 0 yields the identity, like G1Projective::default(). */
/* @shape p_xy=u64[8*n_jobs*n_terms] p_inf=u8[n_jobs*n_terms]? k=u64[4*n_jobs*n_terms] out_xy=u64[8*n_jobs] out_inf=u8[n_jobs] */
int32_t sylow_hip_g1_lincomb_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, uint64_t* out_xy, uint8_t* out_inf,
                                   size_t n_jobs, size_t n_terms, void* stream);
/* sum_i k_i * P_i as ONE G1 point (bucket method).  p_xy [8][n] affine + optional flags, k [4][n] scalars with the
 * same contract as sylow_hip_g1_lincomb_batch (Fp values: k >= p is reduced like Fp::new, i.e. the reference's
 * Mul<&Fp>), out [8][1] affine + out_inf [1].  n = 0 gives the identity.  Stream-ordered, no host synchronisation.
 * Output bit-identical to sylow_hip_g1_lincomb_batch(..., n_jobs = 1, n_terms = n).  Points are taken as given (no on-curve
 * check).  Scratch: about 80 + 7.4 W bytes per point and 232 bytes per bucket (W windows of 2^(c-1) buckets); under
 * sylow_hip_set_scratch_limit the points go through in chunks that fit. */
/* @shape p_xy=u64[8*n] p_inf=u8[n]? k=u64[4*n] out_xy=u64[8] out_inf=u8[1] */
int32_t sylow_hip_g1_msm(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n,
                         uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* The same with the plan given explicitly (A/B runs, crossover measurements, forcing a route in a test); a value < 0 is the default
 * sylow_hip_g1_msm uses.  window: the width c (4..16, else SYLOW_HIP_E_ARG) of the bucket route, default c0 = floor(log2 n) - 4 clamped
 * to 8..16, or c0 +- 1 where that leaves the top window more bits.  min_n: the smallest n sent to the bucket route, default 2^18 = 262144 (measured); below it a scalar multiplication per point and the batch sum
 * (0: the bucket route for every n >= 1).  The output does not depend on either. */
/* @shape p_xy=u64[8*n] p_inf=u8[n]? k=u64[4*n] out_xy=u64[8] out_inf=u8[1] */
int32_t sylow_hip_g1_msm_tuned(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, int32_t window, int64_t min_n,
                               uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* Mul<&Fr> for &Gt (groups/gt.rs:161-187): out_i = gt_i "times" k_i, i.e. gt_i^k_i in Fp12, by the reference's own
 * 256-step signed-digit square-and-multiply (negative digits multiply by the conjugate).  k: Fr values, [4][n]. */
/* @shape gt=u64[48*n] k=u64[4*n] out=u64[48*n] */
int32_t sylow_hip_gt_pow_batch(const uint64_t* gt, const uint64_t* k, uint64_t* out, size_t n, void* stream);
/* GroupAffine::from(&GroupProjective) (group.rs:475-495) */
/* @shape p_xyz=u64[12*n] out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_g1_normalize_batch(const uint64_t* p_xyz, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* @shape p_xyz=u64[24*n] out_xy=u64[16*n] out_inf=u8[n] */
int32_t sylow_hip_g2_normalize_batch(const uint64_t* p_xyz, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* sum_i P_i of a batch of G1 points as ONE point (the `+` fold over signatures / hashes of
 * examples/verify_multiple_messages_same_signer.rs:41-60, Add for G1Projective, group.rs:528-599): p_xy [8][n] affine + flags in,
 * out_xy [8][1] + out_inf [1] out; n = 0 gives the identity.  Serial per-lane accumulation in stages (g1.hip), complete formulas. */
/* @shape p_xy=u64[8*n] p_inf=u8[n]? out_xy=u64[8] out_inf=u8[1] */
int32_t sylow_hip_g1_sum_batch(const uint64_t* p_xy, const uint8_t* p_inf, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* ---- G2: many points into one (g2_msm.hpp, compiled with plk_group.hip).  Public keys are G2 points (lib.rs, examples/dkg.rs:37-49): dkg.rs:309-314 folds keys with `+`,
 * a threshold group key is sum_i lambda_i pk_i, a rogue-key-safe aggregate key is sum_i t_i pk_i, and the G2 half of a KZG or Groth16 verifier
 * is a G2 multi-scalar multiplication.  All four calls are stream-ordered with no host synchronisation, and points are taken as given: no
 * on-curve check, no subgroup check.
 * THE SCALAR RULE is that of sylow_hip_g2_scalar_mul_batch, not that of the G1 calls above: k is an Fp value, k >= p is reduced like Fp::new,
 * and the product is EXACT ON THE WHOLE TWIST -- there is no reduction mod r anywhere (a twist point need not have order r), and there is no
 * "subgroup" variant. */
/* sum_i Q_i as ONE G2 point: q_xy [16][n] affine + optional flags in, out_xy [16][1] + out_inf [1] out; n = 0 gives the identity (0, 1, inf).
 * The segmented lane-pair sum of the committee verifier with one segment, complete formulas. */
/* @shape q_xy=u64[16*n] q_inf=u8[n]? out_xy=u64[16] out_inf=u8[1] */
int32_t sylow_hip_g2_sum_batch(const uint64_t* q_xy, const uint8_t* q_inf, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* n_jobs independent sums sum_i k_{j,i} * Q_{j,i} of n_terms terms each, term-major exactly like sylow_hip_g1_lincomb_batch (element (job j,
 * term i) at index i*n_jobs + j): p_xy [16][n_jobs*n_terms], k [4][n_jobs*n_terms], out [16][n_jobs] affine + flags.  n_terms = 0 yields
 * identities.  A scalar multiplication per lane pair, then the segmented sum. */
/* @shape p_xy=u64[16*n_jobs*n_terms] p_inf=u8[n_jobs*n_terms]? k=u64[4*n_jobs*n_terms] out_xy=u64[16*n_jobs] out_inf=u8[n_jobs] */
int32_t sylow_hip_g2_lincomb_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, uint64_t* out_xy, uint8_t* out_inf,
                                   size_t n_jobs, size_t n_terms, void* stream);
/* sum_i k_i * Q_i as ONE G2 point, bucket method on lane pairs: p_xy [16][n] affine + optional flags, k [4][n], out [16][1] affine +
 * out_inf [1].  n = 0 gives the identity.  Output bit-identical to sylow_hip_g2_lincomb_batch(..., n_jobs = 1, n_terms = n) on every route
 * (both are the canonical affine words of the same group element).  Scratch: about 160 + 14.8 W bytes per point and 448 bytes per bucket
 * (W windows of 2^(c-1) buckets); under sylow_hip_set_scratch_limit the points go through in chunks that fit, every chunk adding into the
 * same buckets. */
/* @shape p_xy=u64[16*n] p_inf=u8[n]? k=u64[4*n] out_xy=u64[16] out_inf=u8[1] */
int32_t sylow_hip_g2_msm(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n,
                         uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* The same with the plan given explicitly; a value < 0 is the default sylow_hip_g2_msm uses.  window: the width c (4..16, else
 * SYLOW_HIP_E_ARG), default as for sylow_hip_g1_msm_tuned below n = 2^16 and 15 from there on (measured).  min_n: the smallest n sent to the
 * bucket route, default 2^16 = 65536 (measured);
 * below it, or under a scratch limit too small for one chunk, sylow_hip_g2_scalar_mul_batch and the segmented sum (0: the bucket route for
 * every n >= 1).  The output does not depend on either. */
/* @shape p_xy=u64[16*n] p_inf=u8[n]? k=u64[4*n] out_xy=u64[16] out_inf=u8[1] */
int32_t sylow_hip_g2_msm_tuned(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, int32_t window, int64_t min_n,
                               uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* G1Affine::new (g1.rs:111-132): status[i] = OK when y^2 == x^3 + 3 (or the identity flag is set), NOT_ON_CURVE otherwise */
/* @shape p_xy=u64[8*n] p_inf=u8[n]? status=u8[n] */
int32_t sylow_hip_g1_on_curve_batch(const uint64_t* p_xy, const uint8_t* p_inf, uint8_t* status, size_t n, void* stream);
/* G2Affine::endomorphism (g2.rs:140-152): psi(x, y) = (xi^((p-1)/3) conj x, xi^((p-1)/2) conj y), identity -> identity.
 * status (may be NULL): NOT_ON_CURVE where the reference's on-curve re-check of the image would panic. */
/* @shape q_xy=u64[16*n] q_inf=u8[n]? out_xy=u64[16*n] out_inf=u8[n] status=u8[n] */
int32_t sylow_hip_g2_psi_batch(const uint64_t* q_xy, const uint8_t* q_inf, uint64_t* out_xy, uint8_t* out_inf, uint8_t* status, size_t n, void* stream);
/* G2Projective::new on affine input (g2.rs:460-525): status = OK / NOT_ON_CURVE / NOT_IN_SUBGROUP.
 * (The reference panics for off-curve input, g2.rs:151; this returns NOT_ON_CURVE instead.) */
/* @shape q_xy=u64[16*n] q_inf=u8[n]? status=u8[n] */
int32_t sylow_hip_g2_subgroup_check_batch(const uint64_t* q_xy, const uint8_t* q_inf, uint8_t* status, size_t n, void* stream);

/* ---- pairing: src/pairing.rs ------------------------------------------------------------------- */
/* G2Affine::precompute().miller_loop(&G1Affine) (pairing.rs:590-619, 676-708): raw Miller value,
 * strict replay of the reference's line formulas and digit schedule.  No infinity handling. */
/* @shape p_xy=u64[8*n] q_xy=u64[16*n] f_out=u64[48*n] */
int32_t sylow_hip_miller_loop_batch(const uint64_t* p_xy, const uint64_t* q_xy, uint64_t* f_out, size_t n, void* stream);
/* MillerLoopResult::final_exponentiation (pairing.rs:245-492) */
/* @shape f=u64[48*n] gt_out=u64[48*n] */
int32_t sylow_hip_final_exp_batch(const uint64_t* f, uint64_t* gt_out, size_t n, void* stream);
/* pairing(&G1, &G2) (pairing.rs:870-893): n independent Gt values; either input at infinity ->
 * Gt identity.  p_inf / q_inf may be NULL. */
/* @shape p_xy=u64[8*n] p_inf=u8[n]? q_xy=u64[16*n] q_inf=u8[n]? gt_out=u64[48*n] */
int32_t sylow_hip_pairing_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf,
                                uint64_t* gt_out, size_t n, void* stream);
/* glued_pairing (pairing.rs:970-1037), one product per job: job j multiplies the pairs
 * [pair_offsets[j], pair_offsets[j+1]) (uint64 device array of n_jobs+1 entries; n_pairs =
 * pair_offsets[n_jobs] is the SoA stride of p_xy / q_xy) with shared
 * squarings and ONE final exponentiation.  skip_infinity = 0 replays the reference (infinity flags
 * ignored: a G2 identity zeroes the product); skip_infinity = 1 drops pairs with an
 * identity on either side (EIP-197 semantics).  gt_out [48][n_jobs] may be NULL;
 * is_one [n_jobs] (may be NULL) receives product == Gt::identity(). */
/* @shape p_xy=u64[8*n_pairs]? p_inf=u8[n_pairs]? q_xy=u64[16*n_pairs]? q_inf=u8[n_pairs]? pair_offsets=u64[n_jobs+1] gt_out=u64[48*n_jobs]? is_one=u8[n_jobs]? */
int32_t sylow_hip_multi_pairing_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf,
                                      const uint64_t* pair_offsets, size_t n_jobs, size_t n_pairs, int32_t skip_infinity,
                                      uint64_t* gt_out, uint8_t* is_one, void* stream);
/* glued_miller_loop(&[G2PreComputed], &[G1Affine]) -> MillerLoopResult (pairing.rs:970-1022), one raw value per job (same job
 * layout as multi_pairing_batch, no final exponentiation, no identity handling -- exactly like the reference's loop).  The value
 * is the product of the per-pair Miller values, which is what the shared-squaring loop computes. */
/* @shape p_xy=u64[8*n_pairs]? q_xy=u64[16*n_pairs]? pair_offsets=u64[n_jobs+1] f_out=u64[48*n_jobs] */
int32_t sylow_hip_glued_miller_loop_batch(const uint64_t* p_xy, const uint64_t* q_xy, const uint64_t* pair_offsets, size_t n_jobs, size_t n_pairs,
                                          uint64_t* f_out, void* stream);
/* glued_pairing over the WHOLE batch as one product (pairing.rs:1029-1037 applied to n_pairs pairs; the batch-verification
 * shape of examples/verify_multiple_messages_same_signer.rs:41-60 and threshold_signing.rs:92-121): gt_out [48][1] =
 * final_exponentiation(prod_i miller(P_i, Q_i)), is_one[0] = (that == Gt::identity()).  The pairs are spread over the whole
 * GPU (chunks with shared squarings, a product tree, one final exponentiation); the value is the one the reference's
 * sequential glued loop yields.  skip_infinity as for multi_pairing_batch.  n_pairs = 0 gives the identity. */
/* @shape p_xy=u64[8*n_pairs]? p_inf=u8[n_pairs]? q_xy=u64[16*n_pairs]? q_inf=u8[n_pairs]? gt_out=u64[48]? is_one=u8[1]? */
int32_t sylow_hip_pairing_product_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf,
                                        size_t n_pairs, int32_t skip_infinity, uint64_t* gt_out, uint8_t* is_one, void* stream);

/* The same loops against line tables a host CACHED from sylow_hip_g2_precompute_batch (`G2PreComputed`, pairing.rs:556):
 * G2PreComputed::miller_loop(&G1Affine) (pairing.rs:590-619) and glued_miller_loop(&[G2PreComputed], &[G1Affine])
 * (pairing.rs:970-1022).  coeffs is the canonical SoA array [87*24][n_tables] exactly as g2_precompute_batch wrote it; pair i
 * uses table table_idx[i] (uint64 device array, every entry < n_tables -- NOT checked on the device: an out-of-range index
 * reads outside coeffs), or table i when table_idx is NULL (then n_tables must equal the number of
 * pairs) -- so one cached key serves any number of G1 points.  Raw MillerLoopResult out, no identity handling (as the
 * reference).  The glued form takes the job layout of multi_pairing_batch; an empty job yields 1. */
/* @shape coeffs=u64[87*24*n_tables] table_idx=u64[n]? p_xy=u64[8*n] f_out=u64[48*n] */
int32_t sylow_hip_miller_loop_precomputed_batch(const uint64_t* coeffs, size_t n_tables, const uint64_t* table_idx, const uint64_t* p_xy,
                                                uint64_t* f_out, size_t n, void* stream);
/* @shape coeffs=u64[87*24*n_tables]? table_idx=u64[n_pairs]? p_xy=u64[8*n_pairs]? pair_offsets=u64[n_jobs+1] f_out=u64[48*n_jobs] */
int32_t sylow_hip_glued_miller_loop_precomputed_batch(const uint64_t* coeffs, size_t n_tables, const uint64_t* table_idx, const uint64_t* p_xy,
                                                      const uint64_t* pair_offsets, size_t n_jobs, size_t n_pairs, uint64_t* f_out, void* stream);
/* The two halves of pairing_product_batch, for hosts that split one product over several GPUs:
 * partial: f_out [48][1] = c * prod_i miller(P_i, Q_i) of this shard (no final exponentiation; n_pairs = 0 gives 1) with some c in Fp* that
 *          depends on the route taken -- an intermediate for _final_ only, where c disappears (c^(p^6 - 1) = 1): the Miller loops of a value
 *          that ends in a final exponentiation may run on isomorphic curves.  The reference's raw MillerLoopResult
 *          itself comes from sylow_hip_miller_loop_batch / sylow_hip_glued_miller_loop_batch;
 * final:   gt_out [48][1] = final_exponentiation(prod_{j<k} parts_j), parts SoA [48][k]; is_one[0] = (== Gt::identity()).
 * glued_pairing over all shards == fp12_product_final_exp over the shards' partials (Fp12 products commute). */
/* @shape p_xy=u64[8*n_pairs]? p_inf=u8[n_pairs]? q_xy=u64[16*n_pairs]? q_inf=u8[n_pairs]? f_out=u64[48] */
int32_t sylow_hip_pairing_product_partial_batch(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf,
                                                size_t n_pairs, int32_t skip_infinity, uint64_t* f_out, void* stream);
/* @shape parts=u64[48*k] gt_out=u64[48]? is_one=u8[1]? */
int32_t sylow_hip_fp12_product_final_exp(const uint64_t* parts, size_t k, uint64_t* gt_out, uint8_t* is_one, void* stream);

/* ---- hash-to-curve and BLS: src/hasher.rs, src/svdw.rs, src/groups/g1.rs:307-331, src/lib.rs --- */
/* Expander::hash_to_field(msg, 2, 48) with XMDExpander<Keccak256>(dst, 128) (hasher.rs:84-128, 157-250): out_u [8][n] = (u0, u1),
 * each the 48-byte big-endian slice of expand_message_xmd(msg, DST', 96) reduced mod p.  dst_host NULL = the library DST. */
/* @shape msgs=u8[*] msg_offsets=u64[n+1] dst_host=u8[dst_len]? out_u=u64[8*n] */
int32_t sylow_hip_hash_to_field_batch(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* dst_host, size_t dst_len,
                                      uint64_t* out_u, size_t n, void* stream);
/* G1Projective::hash_to_curve with XMDExpander<Keccak256>(dst, 128), COUNT=2, L=48.
 * msgs: concatenated message bytes; msg_offsets: n+1 uint64 byte offsets.  dst/dst_len: HOST
 * pointer to the domain separation tag (NULL -> sylow's DST, lib.rs:90). */
/* @shape msgs=u8[*] msg_offsets=u64[n+1] dst_host=u8[dst_len]? out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_hash_to_g1_batch(const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* dst_host, size_t dst_len,
                                   uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* SvdW::unchecked_map_to_point (svdw.rs:180-262, RFC 9380 6.6.1 straight line, Z = 1) by itself: u [4][n] -> (x, y) [8][n] on the
 * curve; status (may be NULL) = CANNOT_HASH where the reference returns MapError. */
/* @shape u=u64[4*n] out_xy=u64[8*n] status=u8[n] */
int32_t sylow_hip_svdw_map_batch(const uint64_t* u, uint64_t* out_xy, uint8_t* status, size_t n, void* stream);
/* Fp::compute_naf (fp.rs:653-662) on the raw 256-bit words k [4][n]: out_np / out_nm [4][n] = the masks of the +1 / -1 digits
 * (digit_i = np_i - nm_i; x + (x >> 1) is taken modulo 2^256 exactly as the reference's 256-bit arithmetic does). */
/* @shape k=u64[4*n] out_np=u64[4*n] out_nm=u64[4*n] */
int32_t sylow_hip_fp_compute_naf_batch(const uint64_t* k, uint64_t* out_np, uint64_t* out_nm, size_t n, void* stream);
/* sign(&Fp, &[u8]) (lib.rs:179-187): sig_i = sk_i * H(msg_i), affine out */
/* @shape sk=u64[4*n] msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n] */
int32_t sylow_hip_bls_sign_batch(const uint64_t* sk, const uint8_t* msgs, const uint64_t* msg_offsets,
                                 uint64_t* sig_xy, uint8_t* sig_inf, size_t n, void* stream);
/* verify(&G2Projective, &[u8], &G1Projective) (lib.rs:223-236): ok_i = [ e(sig_i, G2gen) == e(H(msg_i), pk_i) ]; identity inputs
 * as pairing() treats them (that pairing is Gt::identity()).  Evaluated as e(sig_i, G2gen) * e(-H(msg_i), pk_i) == 1 with one
 * shared-squaring 2-pair Miller loop and ONE final exponentiation per element (the shape of
 * examples/verify_multiple_messages_same_signer.rs:41-60, threshold_signing.rs:92-121): FE(a) == FE(b) <=> FE(a conj(b)) == 1 and
 * conj(miller(H, pk)) = miller(-H, pk) exactly, so the boolean is the reference's for EVERY input.  _fused_ is the same
 * kernel under its round-1 name. */
/* @shape pk_xy=u64[16*n] pk_inf=u8[n]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_bls_verify_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint8_t* msgs, const uint64_t* msg_offsets,
                                   const uint64_t* sig_xy, const uint8_t* sig_inf, uint8_t* ok, size_t n, void* stream);
/* @shape pk_xy=u64[16*n] pk_inf=u8[n]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_bls_verify_fused_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint8_t* msgs, const uint64_t* msg_offsets,
                                         const uint64_t* sig_xy, const uint8_t* sig_inf, uint8_t* ok, size_t n, void* stream);
/* The same boolean evaluated literally as lib.rs:223-236 writes it: two Miller loops, two final exponentiations, compare
 * (~1.5x the time; kept as the second implementation the first is tested against, and to price the reference's shape). */
/* @shape pk_xy=u64[16*n] pk_inf=u8[n]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_bls_verify_two_pairings_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint8_t* msgs, const uint64_t* msg_offsets,
                                                const uint64_t* sig_xy, const uint8_t* sig_inf, uint8_t* ok, size_t n, void* stream);
/* ---- a caller-chosen RFC 9380 expander and tag: Expander, XMDExpander<D>, XOFExpander<D> (src/lib.rs:71-84, src/hasher.rs) ---------
 * expander: XMDExpander<Keccak256> (the suite of every entry point above), XMDExpander<Sha256> or XOFExpander<Shake128>, the two the
 * reference pins with RFC 9380 literals (hasher.rs:345-472).  dst_host / dst_len: HOST pointer to the tag, NULL = the library tag
 * (lib.rs:90); a tag longer than 255 bytes is shortened once per call as XMDExpander::new / XOFExpander::new do (hasher.rs:157-173,
 * 274-290: H("H2C-OVERSIZE-DST-" || DST), for the XOF ceil(2 security_bits / 8) bytes of it).  security_bits: the expanders' k
 * (128 for BN254).  Expander 0 with the same tag gives the bytes, field elements, points and flags of the entry points above, bit for
 * bit.  The new expanders hash one message per lane at every batch size.
 * Whole-call errors, the conditions of HashError::ExpandMessage (hasher.rs:211-216) and of i2osp's ranges: an unknown expander,
 * len_in_bytes > 65535, XMD with ceil(len_in_bytes / 32) > 255 or 2 security_bits > 256, security_bits < 1, XOF with
 * ceil(2 security_bits / 8) > 255, and len_in_bytes == 0 (there the reference's XMD indexes an empty vector and panics, its XOF returns
 * no bytes: a divergence) return SYLOW_HIP_E_ARG, launch nothing and name the reason in sylow_hip_last_error(). */
#define SYLOW_HIP_EXPANDER_XMD_KECCAK256 0
#define SYLOW_HIP_EXPANDER_XMD_SHA256 1
#define SYLOW_HIP_EXPANDER_XOF_SHAKE128 2
/* Expander::expand_message(msg, len_in_bytes) (hasher.rs:201-250 XMD, 315-329 XOF): raw bytes, row i at out + i * len_in_bytes. */
/* @shape msgs=u8[*] msg_offsets=u64[n+1] dst_host=u8[dst_len]? out=u8[len_in_bytes*n] */
int32_t sylow_hip_expand_message_batch(int32_t expander, const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* dst_host, size_t dst_len,
                                       int32_t security_bits, size_t len_in_bytes, uint8_t* out, size_t n, void* stream);
/* Expander::hash_to_field(msg, 2, 48) (hasher.rs:84-128) under the expander: out_u [8][n] = (u0, u1). */
/* @shape msgs=u8[*] msg_offsets=u64[n+1] dst_host=u8[dst_len]? out_u=u64[8*n] */
int32_t sylow_hip_hash_to_field_expander_batch(int32_t expander, const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* dst_host, size_t dst_len,
                                               int32_t security_bits, uint64_t* out_u, size_t n, void* stream);
/* G1Projective::hash_to_curve(&expander, msg) (g1.rs:307-331), affine out. */
/* @shape msgs=u8[*] msg_offsets=u64[n+1] dst_host=u8[dst_len]? out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_hash_to_g1_expander_batch(int32_t expander, const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* dst_host, size_t dst_len,
                                            int32_t security_bits, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* sign_message(&expander, msg, sk) (g1.rs:355): sig_i = sk_i * H(msg_i) with H from the expander. */
/* @shape dst_host=u8[dst_len]? sk=u64[4*n] msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n] */
int32_t sylow_hip_bls_sign_expander_batch(int32_t expander, const uint8_t* dst_host, size_t dst_len, int32_t security_bits, const uint64_t* sk,
                                          const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t* sig_xy, uint8_t* sig_inf, size_t n, void* stream);
/* The boolean of verify (lib.rs:223-236) with H from the expander: sylow_hip_bls_verify_batch's evaluation, reading of identities and
 * routes by batch size behind another hashing launch. */
/* @shape dst_host=u8[dst_len]? pk_xy=u64[16*n] pk_inf=u8[n]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_bls_verify_expander_batch(int32_t expander, const uint8_t* dst_host, size_t dst_len, int32_t security_bits,
                                            const uint64_t* pk_xy, const uint8_t* pk_inf, const uint8_t* msgs, const uint64_t* msg_offsets,
                                            const uint64_t* sig_xy, const uint8_t* sig_inf, uint8_t* ok, size_t n, void* stream);
/* The same boolean on points H_i the caller hashed -- another hash-to-curve, or one hash checked against many signatures:
 * ok_i = [ e(sig_i, G2gen) == e(H_i, pk_i) ], h_xy [8][n] affine (reduced like Fp::new), identity inputs as pairing() treats them:
 * h_inf[i] = 1 (h_inf may be NULL) makes the right-hand pairing Gt::identity(), as an identity hash does above. */
/* @shape pk_xy=u64[16*n] pk_inf=u8[n]? h_xy=u64[8*n] h_inf=u8[n]? sig_xy=u64[8*n] sig_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_bls_verify_hashed_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint64_t* h_xy, const uint8_t* h_inf,
                                          const uint64_t* sig_xy, const uint8_t* sig_inf, uint8_t* ok, size_t n, void* stream);
/* ---- wire formats: G1Affine/G2Affine::{to,from}_be_bytes (g1.rs:151-280, g2.rs:319-433) -------------- */
/* G1: 64 bytes x | y big-endian; G2: 128 bytes x.c1 | x.c0 | y.c1 | y.c0; bit 7 of byte 0 is the infinity flag and
 * the identity is written as (0, 1) + flag.  from_be_bytes masks the flag, then: a coordinate >= p, or a set flag
 * with coordinates other than (0, 1) -> DECODE_ERROR (the reference's CtOption is none); off the curve ->
 * NOT_ON_CURVE; G2 outside the r-torsion -> NOT_IN_SUBGROUP.  Failed elements decode to the identity. */
/* @shape p_xy=u64[8*n] p_inf=u8[n]? out=u8[64*n] */
int32_t sylow_hip_g1_to_be_bytes_batch(const uint64_t* p_xy, const uint8_t* p_inf, uint8_t* out /*[n][64]*/, size_t n, void* stream);
/* @shape in=u8[64*n] out_xy=u64[8*n] out_inf=u8[n] status=u8[n] */
int32_t sylow_hip_g1_from_be_bytes_batch(const uint8_t* in /*[n][64]*/, uint64_t* out_xy, uint8_t* out_inf, uint8_t* status, size_t n, void* stream);
/* @shape p_xy=u64[16*n] p_inf=u8[n]? out=u8[128*n] */
int32_t sylow_hip_g2_to_be_bytes_batch(const uint64_t* p_xy, const uint8_t* p_inf, uint8_t* out /*[n][128]*/, size_t n, void* stream);
/* @shape in=u8[128*n] out_xy=u64[16*n] out_inf=u8[n] status=u8[n] */
int32_t sylow_hip_g2_from_be_bytes_batch(const uint8_t* in /*[n][128]*/, uint64_t* out_xy, uint8_t* out_inf, uint8_t* status, size_t n, void* stream);

/* ---- EVM alt_bn128 precompile shapes: examples/reth_bn128.rs:99-217 (EIP-196 / EIP-197) --------- */
/* Byte-level batches.  Field elements are 32-byte big-endian and must be < p (else DECODE_ERROR =
 * Bn128FieldPointNotAMember); (0,0) is the identity; G1 points must be on the curve, G2 points on the twist
 * and in the r-torsion (else NOT_ON_CURVE / NOT_IN_SUBGROUP = Bn128AffineGFailedToCreate).
 * ecadd: in [n][128] = two points, out [n][64] (identity -> 64 zero bytes, to_be_bytes_scrubbed g1.rs:182-192).
 * ecmul: in [n][96] = point | 32-byte scalar (any 256-bit value, reduced mod r), out [n][64].
 * ecpairing: `in` = n_pairs 192-byte elements (G1 x|y, G2 x.c1|x.c0|y.c1|y.c0), job j owns elements
 * [pair_offsets[j], pair_offsets[j+1]); result[j] = 1 iff the product of pairings is one (empty job -> 1).
 * Identity pairs are skipped as EIP-197 requires (the reference adapter inherits glued_pairing's Q = identity
 * defect and answers false there).  Padding, length % 192 and gas rules are host-side (sylow_amd/evm.py). */
/* @shape in=u8[128*n] out=u8[64*n] status=u8[n] */
int32_t sylow_hip_evm_ecadd_batch(const uint8_t* in, uint8_t* out, uint8_t* status, size_t n, void* stream);
/* @shape in=u8[96*n] out=u8[64*n] status=u8[n] */
int32_t sylow_hip_evm_ecmul_batch(const uint8_t* in, uint8_t* out, uint8_t* status, size_t n, void* stream);
/* @shape in=u8[192*n_pairs]? pair_offsets=u64[n_jobs+1] result=u8[n_jobs] status=u8[n_jobs] */
int32_t sylow_hip_evm_ecpairing_batch(const uint8_t* in, const uint64_t* pair_offsets, size_t n_jobs, size_t n_pairs,
                                      uint8_t* result, uint8_t* status, void* stream);
/* Same-signer batch (examples/verify_multiple_messages_same_signer.rs:41-60): ONE public key (pk_xy is a
 * 1-element SoA array, pk_inf one byte or NULL) against n (message, signature) pairs.  The key's G2PreComputed
 * line table is built once per call and both pairs of every element read wave-uniform tables, so the Miller
 * loops contain no G2 arithmetic. */
/* @shape pk_xy=u64[16] pk_inf=u8[1]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_bls_verify_same_signer_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, const uint8_t* msgs, const uint64_t* msg_offsets,
                                               const uint64_t* sig_xy, const uint8_t* sig_inf, uint8_t* ok, size_t n, void* stream);
/* The same check against a key table the host keeps across calls ("G2PreComputed cached per pk"): sylow_hip_g2_line_table
 * writes the line table of element idx of an SoA G2 array (n = its stride) into `table`, a device buffer of
 * sylow_hip_g2_line_table_words() int32 words (opaque, device-internal digit layout); bls_verify_line_table_batch then runs
 * the same-signer check with no G2 arithmetic and nothing rebuilt per call.  pk_inf: one device byte or NULL. */
int32_t sylow_hip_g2_line_table_words(void);
/* @shape q_xy=u64[16*n]? table=i32[*] */
int32_t sylow_hip_g2_line_table(const uint64_t* q_xy, size_t n, size_t idx, int32_t* table, void* stream);
/* @shape pk_table=i32[*] pk_inf=u8[1]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_bls_verify_line_table_batch(const int32_t* pk_table, const uint8_t* pk_inf, const uint8_t* msgs, const uint64_t* msg_offsets,
                                              const uint64_t* sig_xy, const uint8_t* sig_inf, uint8_t* ok, size_t n, void* stream);
/* G2Affine::precompute (pairing.rs:676-708): the 87 line-coefficient triples [Ell; 87] of each point, canonical
 * words, SoA [87*24][n] (triple t = words 24t..24t+23 = ell.0, ell.1, ell.2 as Fp2).  Strict replay. */
/* @shape q_xy=u64[16*n] coeffs=u64[87*24*n] */
int32_t sylow_hip_g2_precompute_batch(const uint64_t* q_xy, uint64_t* coeffs, size_t n, void* stream);
/* AND of a flag array -> one int32 on the device (1 = all set); the multi-GPU aggregate then
 * MIN-reduces that word over ranks (RCCL has no bit-AND; min over {0,1} is AND). */
/* @shape flags=u8[n] out_dev=i32[1] */
int32_t sylow_hip_flags_all(const uint8_t* flags, size_t n, int32_t* out_dev, void* stream);


/* ---- multi-GPU aggregates (one process per GPU): the only exchange steps of the path --------------------------------------
 * `comm` is the caller's RCCL communicator (ncclComm_t) passed as void*; NULL means a single rank.  RCCL is bound at run time
 * (dlopen of librccl.so.1), so single-GPU hosts never load it.  Both calls are asynchronous on `stream` and must be issued by
 * every rank of the communicator, like any collective.
 * all_valid: out_dev[0] (device int32) = 1 iff every flag on EVERY rank is set -- flags_all + a 4-byte MIN all-reduce
 *            (verify(...) over a sharded batch -> one boolean, lib.rs:223-236).
 * pairing_product_all: glued_pairing (pairing.rs:1029-1037) over the union of all ranks' pairs: every rank computes its
 *            partial Miller product, the 384-byte partials are all-gathered and each rank finishes product + final
 *            exponentiation, so every rank ends with the same gt_out [48][1] / is_one[0]. */
/* @shape flags=u8[n] comm=void[*]? out_dev=i32[1] */
int32_t sylow_hip_all_valid(const uint8_t* flags, size_t n, void* comm, int32_t* out_dev, void* stream);
/* @shape p_xy=u64[8*n_pairs]? p_inf=u8[n_pairs]? q_xy=u64[16*n_pairs]? q_inf=u8[n_pairs]? comm=void[*]? gt_out=u64[48]? is_one=u8[1]? */
int32_t sylow_hip_pairing_product_all(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf, size_t n_pairs,
                                      int32_t skip_infinity, void* comm, uint64_t* gt_out, uint8_t* is_one, void* stream);

/* Aggregate verification -- "are ALL n signatures valid?" as ONE Gt comparison, the batch shape of
 * examples/verify_multiple_messages_same_signer.rs:41-60 and threshold_signing.rs:92-121, where the reference glues the 2n pairs
 * (sig_i, G2gen), (-H(msg_i), pk_i) into one product:  gt_out [48][1] = that product after the final exponentiation,
 * is_one[0] = (gt_out == Gt::identity()).  Evaluated through bilinearity: prod_i e(sig_i, G2gen) = e(sum_i sig_i, G2gen), so the
 * G2gen half costs n G1 additions and ONE Miller loop; with one key for the whole batch (n_pk = 1) the other half collapses the
 * same way, prod_i e(-H(msg_i), pk) = e(-sum_i H(msg_i), pk), and the check is n hashes + two sums + a two-pair product.  The Gt
 * value is the same group element as the reference's 2n-pair product, hence the same words.  n_pk = n: pk_xy [16][n] one key per
 * message; n_pk = 1: pk_xy [16][1].  Identity signatures / keys contribute 1 (pairing() semantics).  n = 0 gives the identity.
 * (As in the reference's example there are no random weights: it answers "is the PRODUCT the identity" -- the product sees the
 * signatures only through their sum, so signatures permuted among the messages still pass; per-element flags: bls_verify_batch.)
 * Two more shapes of the key array fold the OTHER half the same way; both use the term-major index rule of sylow_hip_g1_lincomb_batch
 * (element t of job i at t * n_jobs + i), so one huge group and many small ones are both coalesced reads:
 *   n_pk = c n, c >= 2, n >= 1 -- COMMITTEES: key j belongs to message j mod n and sig_i is committee i's aggregate signature (the
 *     shape of batch_verify_partial in threshold_signing.rs / dkg.rs and of every validator-set check; n = 1 is "one message, one
 *     aggregate signature, a list of keys").  prod_t e(-H(msg_i), pk[t n + i]) = e(-H(msg_i), apk_i), apk_i = sum_t pk[t n + i]: a
 *     segmented G2 sum and n + 1 Miller loops whatever c is.  A caller who holds individual signatures sums them first with
 *     sylow_hip_g1_sum_batch.
 *   n = c n_pk, c >= 2, n_pk >= 2 -- KEY REUSE: signature i is under key i mod n_pk.  prod_t e(-H(msg[t n_pk + j]), pk_j) =
 *     e(-sum_t H(msg[t n_pk + j]), pk_j): a segmented G1 sum and n_pk + 1 Miller loops.
 *   Any other (n, n_pk) with n > 0, n_pk = 0 included, is SYLOW_HIP_E_ARG.  n_pk = 1 and n_pk = n run exactly as before.
 * gt_out is the Gt element, hence the words, of the reference's glued_pairing over the n + max(n, n_pk) literal pairs (sig_i, G2gen),
 * (-H(msg[j mod n]), pk[j mod n_pk]).  A flagged key adds nothing to its sum, whatever its coordinate words hold; a committee whose keys
 * cancel has apk_i = identity and its pair contributes 1, like pairing().  Key words >= p are reduced like Fp::new.  Precondition, as for
 * the two older shapes: keys in G2 proper; and summing keys presumes PROOFS OF POSSESSION -- without them a signer can publish a key that
 * cancels the others' (rogue-key attack).  With comm != NULL every rank passes WHOLE committees / whole periods of keys (shards are cut by
 * message row); one committee split across ranks is not supported.
 *   _partial_: f_out [48][1] = this shard's Miller product up to a factor in Fp* (see sylow_hip_pairing_product_partial_batch; for hosts
 *              that combine shards themselves, with sylow_hip_fp12_product_final_exp);
 *   _verify_:  the whole check; comm = the host's ncclComm_t for a batch sharded over the GPUs of a node (every rank passes its
 *              shard and receives the same answer; 384 bytes per rank are all-gathered), NULL = this process alone. */
/* @shape pk_xy=u64[16*n_pk] pk_inf=u8[n_pk]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? f_out=u64[48] */
int32_t sylow_hip_bls_aggregate_partial_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n_pk, const uint8_t* msgs, const uint64_t* msg_offsets,
                                              const uint64_t* sig_xy, const uint8_t* sig_inf, size_t n, uint64_t* f_out, void* stream);
/* @shape pk_xy=u64[16*n_pk] pk_inf=u8[n_pk]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? comm=void[*]? gt_out=u64[48]? is_one=u8[1]? */
int32_t sylow_hip_bls_aggregate_verify_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n_pk, const uint8_t* msgs, const uint64_t* msg_offsets,
                                             const uint64_t* sig_xy, const uint8_t* sig_inf, size_t n, void* comm, uint64_t* gt_out, uint8_t* is_one, void* stream);
/* The SOUND one-boolean form ("random-linear-combination multi-pairing"): the small-exponent batch test
 *   prod_i [ e(sig_i, G2gen) e(-H(msg_i), pk_i) ]^(w_i) == identity,   evaluated as e(sum_i w_i sig_i, G2gen) prod_i e(-w_i H(msg_i), pk_i).
 * weights [4][n]: w_i as Fp values (the caller draws them AFTER the signatures are fixed, e.g. 64 or 128 random bits each; 0 removes an
 * element from the test).  If every signature is valid the result is the identity; if any is not, the test passes with probability at most
 * 2^-(bits of the weights) over the caller's randomness (keys in G2 proper, as G2Projective::new guarantees).  No counterpart exists upstream --
 * the reference's examples multiply unweighted (the two entry points above); the Gt value equals the reference's glued_pairing over the 2n
 * pairs (w_i sig_i, G2gen), (-w_i H(msg_i), pk_i), which is how it is tested.  Shapes, n_pk (committees and key reuse included: weights
 * stay [4][n], one per message row, and multiply sig_i and H(msg_i); the key sums are never weighted), comm and the _partial_ form as above. */
/* @shape pk_xy=u64[16*n_pk] pk_inf=u8[n_pk]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? weights=u64[4*n] f_out=u64[48] */
int32_t sylow_hip_bls_weighted_partial_batch(const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n_pk, const uint8_t* msgs, const uint64_t* msg_offsets,
                                             const uint64_t* sig_xy, const uint8_t* sig_inf, const uint64_t* weights, size_t n, uint64_t* f_out, void* stream);
/* @shape pk_xy=u64[16*n_pk] pk_inf=u8[n_pk]? msgs=u8[*] msg_offsets=u64[n+1] sig_xy=u64[8*n] sig_inf=u8[n]? weights=u64[4*n] comm=void[*]? gt_out=u64[48]? is_one=u8[1]? */
int32_t sylow_hip_bls_batch_verify_weighted(const uint64_t* pk_xy, const uint8_t* pk_inf, size_t n_pk, const uint8_t* msgs, const uint64_t* msg_offsets,
                                            const uint64_t* sig_xy, const uint8_t* sig_inf, const uint64_t* weights, size_t n, void* comm,
                                            uint64_t* gt_out, uint8_t* is_one, void* stream);

/* ---- Groth16 on BN254 under ONE verifying key (groth16.hip, groth16_pair.hpp compiled with plk_multi.hip) -------------------------
 * vk = (alpha in G1; beta, gamma, delta in G2; IC_0 .. IC_l in G1), a proof is (A in G1, B in G2, C in G1) with l = n_inputs public
 * inputs x_1 .. x_l.  In the EVM / snarkjs form
 *     vk_x = IC_0 + sum_j x_j IC_j,     ok = [ e(-A, B) e(alpha, beta) e(vk_x, gamma) e(C, delta) == 1 ].
 * Conventions of the three calls:
 *   vk arrays: device SoA arrays WITHOUT flag arrays -- vk_alpha [8][1], vk_beta / vk_gamma / vk_delta [16][1], vk_ic [8][n_inputs + 1].
 *   proofs:    a_xy [8][n], b_xy [16][n], c_xy [8][n], each with an optional identity-flag array; inputs [4][n_inputs * n], INPUT-MAJOR:
 *              input j of proof i at index j*n + i (the term-major rule of sylow_hip_g1_lincomb_batch).
 *   words:     field words >= p are reduced like Fp::new, as everywhere.
 *   scalars:   inputs and weights follow sylow_hip_evm_ecmul_batch -- ANY 256-bit word, taken mod r (every G1 point has order r, so for a
 *              word < p this is also what sylow_hip_g1_lincomb_batch computes).  Solidity verifiers REJECT an input >= r: a host that wants
 *              that rule checks the inputs with sylow_hip_fr_from_be_bytes_batch first.
 *   identity:  EIP-197, as sylow_hip_evm_ecpairing_batch and skip_infinity = 1: a pair with a flagged identity on either side contributes 1,
 *              and so does a vk_x that sums to the identity.
 *   points:    taken as given, as in the MSM calls: no on-curve check, no subgroup check.  PRECONDITION: B, beta, gamma, delta in G2
 *              proper (sylow_hip_g2_subgroup_check_batch / sylow_hip_g2_from_be_bytes_batch establish that).
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call.  n = 0 launches nothing that reads the arrays;
 *              n_inputs = 0 is legal (vk_x = IC_0).  NULL where a pointer is required: SYLOW_HIP_E_ARG and no launch. */
/* vk_x of every proof: out [8][n] affine + flags (the identity as (0, 1) + flag), bit-identical to sylow_hip_g1_lincomb_batch with
 * n_jobs = n, n_terms = n_inputs + 1 on the bases replicated n times, scalar 1 for IC_0 and the inputs taken mod r.  The bases are shared:
 * one small kernel builds a 16-entry window table per base per call, then one lane per proof runs Straus interleaving -- ONE chain of 252
 * doublings and one complete addition per input and 4-bit window.  Equal bases and partial sums that hit the identity are legal. */
/* @shape vk_ic=u64[8*(n_inputs+1)] inputs=u64[4*n_inputs*n]? out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_groth16_vk_x_batch(const uint64_t* vk_ic, size_t n_inputs, const uint64_t* inputs, size_t n,
                                     uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* ok [n]: the boolean above for every proof.  Routes: n <= 1024 with 4 n <= SYLOW_HIP_OPT_WIDE_MAX (default 6144), and any batch whose
 * scratch limit is below 1024 proofs' line tables (19.5 KB each) or with SYLOW_HIP_OPT_MULTI_TABLES = 0, take the COMPOSED route: vk_x
 * by the kernel above, then the four literal pairs per proof through sylow_hip_multi_pairing_batch.  Every other batch takes the TABLE route:
 * per call the lines of gamma and delta are formed once and e(-alpha, beta) is ONE Miller loop whose value is multiplied into every
 * job before its final exponentiation; per proof vk_x, the lines of B_i (in HBM, in slices under sylow_hip_set_scratch_limit exactly as
 * sylow_hip_multi_pairing_batch slices), one shared-squaring loop over three lines per step, one final exponentiation, a compare.  The flags
 * are the same on every route and under every limit. */
/* @shape vk_alpha=u64[8] vk_beta=u64[16] vk_gamma=u64[16] vk_delta=u64[16] vk_ic=u64[8*(n_inputs+1)] a_xy=u64[8*n] a_inf=u8[n]? b_xy=u64[16*n] b_inf=u8[n]? c_xy=u64[8*n] c_inf=u8[n]? inputs=u64[4*n_inputs*n]? ok=u8[n] */
int32_t sylow_hip_groth16_verify_batch(const uint64_t* vk_alpha, const uint64_t* vk_beta, const uint64_t* vk_gamma, const uint64_t* vk_delta,
                                       const uint64_t* vk_ic, size_t n_inputs, const uint64_t* a_xy, const uint8_t* a_inf,
                                       const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy, const uint8_t* c_inf,
                                       const uint64_t* inputs, size_t n, uint8_t* ok, void* stream);
/* The SOUND one-boolean form, the move of sylow_hip_bls_batch_verify_weighted: with weights r_i [4][n]
 *     prod_i e(r_i A_i, B_i) e(-s alpha, beta) e(-sum_i r_i vk_x_i, gamma) e(-sum_i r_i C_i, delta) == 1,      s = sum_i r_i mod r,
 *     sum_i r_i vk_x_i = s IC_0 + sum_j (sum_i r_i x_ij mod r) IC_j
 * -- n scalar multiplications in G1, one n-pair Miller product, one multi-scalar multiplication over the C_i (sylow_hip_g1_msm, whatever
 * route it picks), the Fr column sums s, s_j in one two-level reduction, n_inputs + 2 more scalar multiplications, three more pairs and ONE
 * final exponentiation.  gt_out [48][1] is the Gt element, hence the words, of the reference's glued_pairing over the n + 3 literal pairs
 * written above; is_one [1] its comparison with the identity; either may be NULL (not both).  A weight of 0 removes a proof from the test;
 * n = 0 gives the identity.  The caller draws the weights AFTER the proofs are fixed (e.g. 64 or 128 random bits each): if every proof is
 * valid the result is the identity; if any is not, the test passes with probability at most 2^-(bits of the weights) over the caller's
 * randomness, provided every G2 input is in the r-torsion (the precondition above). */
/* @shape vk_alpha=u64[8] vk_beta=u64[16] vk_gamma=u64[16] vk_delta=u64[16] vk_ic=u64[8*(n_inputs+1)] a_xy=u64[8*n] a_inf=u8[n]? b_xy=u64[16*n] b_inf=u8[n]? c_xy=u64[8*n] c_inf=u8[n]? inputs=u64[4*n_inputs*n]? weights=u64[4*n] gt_out=u64[48]? is_one=u8[1]? */
int32_t sylow_hip_groth16_batch_verify_weighted(const uint64_t* vk_alpha, const uint64_t* vk_beta, const uint64_t* vk_gamma, const uint64_t* vk_delta,
                                                const uint64_t* vk_ic, size_t n_inputs, const uint64_t* a_xy, const uint8_t* a_inf,
                                                const uint64_t* b_xy, const uint8_t* b_inf, const uint64_t* c_xy, const uint8_t* c_inf,
                                                const uint64_t* inputs, const uint64_t* weights, size_t n, uint64_t* gt_out, uint8_t* is_one, void* stream);

/* ---- KZG openings on BN254 under ONE SRS (kzg.hip; the per-opening check runs plk_verify.hip's same-signer kernels) -------------------
 * The SRS as the caller holds it: the G1 generator (1, 2), the library's G2 generator, and tau_g2 = tau G2gen.  An opening is
 * (C, z, y, pi) and claims f(z) = y for the polynomial committed in C:
 *     F = C - y G1gen + z pi,     ok = [ e(F, G2gen) e(-pi, tau_g2) == 1 ].
 * Conventions of the four calls (those of the Groth16 block above):
 *   arrays:    device SoA arrays -- c_xy [8][n], pi_xy [8][n], z [4][n], y [4][n]; c_inf / pi_inf are optional identity-flag arrays.
 *   tau_g2:    tau_g2_xy [16][1], WITHOUT a flag array.
 *   words:     field words >= p are reduced like Fp::new, as everywhere.
 *   scalars:   z, y and weights follow sylow_hip_evm_ecmul_batch and the Groth16 inputs -- ANY 256-bit word, taken mod r.
 *   identity:  pairing() / EIP-197: a pair with an identity on either side contributes 1.  A flagged C is the commitment to the zero
 *              polynomial and is legal; a flagged pi is the proof for a constant polynomial, and the row is then valid iff C = y G1gen; an F
 *              that sums to the identity while pi is not the identity is an INVALID row.  A flagged point adds nothing, whatever its
 *              coordinate words hold.
 *   points:    taken as given: no on-curve check, no subgroup check.  PRECONDITION: tau_g2 in G2 proper, and not the identity.
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call.  n = 0 launches nothing that reads the arrays.  NULL
 *              where a pointer is required: SYLOW_HIP_E_ARG, no launch, nothing written. */
/* F_i for every opening: out [8][n] affine + flags (the identity as (0, 1) + flag), bit-identical to the composition
 * sylow_hip_g1_generator_mul_batch(y mod r), sylow_hip_g1_scalar_mul_batch(pi, z mod r), sylow_hip_g1_add_batch, sylow_hip_g1_sub_batch -- both
 * are the canonical affine words of one group element.  ONE launch, one opening per lane, one accumulator: the GLV window walk of z pi, then
 * 32 complete additions against the per-device fixed-base table of the G1 generator for y, then C; one normalisation.  Every addition is
 * complete: C = +-z pi, C = y G1gen, pi = +-G1gen and scalars = 0 mod r are legal. */
/* @shape c_xy=u64[8*n] c_inf=u8[n]? z=u64[4*n] y=u64[4*n] pi_xy=u64[8*n] pi_inf=u8[n]? out_xy=u64[8*n] out_inf=u8[n] */
int32_t sylow_hip_kzg_fold_batch(const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z, const uint64_t* y,
                                 const uint64_t* pi_xy, const uint8_t* pi_inf, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream);
/* ok [n]: the boolean above for every opening, evaluated as the fold and then the same-signer BLS check with sig := F, -H := -pi and
 * tau_g2 as the key: its line table is built once per call, no G2 arithmetic runs per opening.  Routes by batch size exactly as
 * sylow_hip_bls_verify_same_signer_batch (one wavefront per Miller loop up to SYLOW_HIP_OPT_WIDE_VERIFY_MAX, lane quads up to
 * SYLOW_HIP_OPT_QUAD_MAX, lane pairs above); the flags are the same on every route and equal sylow_hip_kzg_fold_batch +
 * sylow_hip_bls_verify_hashed_batch with tau_g2 replicated n times. */
/* @shape tau_g2_xy=u64[16] c_xy=u64[8*n] c_inf=u8[n]? z=u64[4*n] y=u64[4*n] pi_xy=u64[8*n] pi_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_kzg_verify_batch(const uint64_t* tau_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z, const uint64_t* y,
                                   const uint64_t* pi_xy, const uint8_t* pi_inf, uint8_t* ok, size_t n, void* stream);
/* The same against a line table of tau_g2 the host cached with sylow_hip_g2_line_table (sylow_hip_g2_line_table_words() int32 words):
 * nothing is rebuilt per call.  Like sylow_hip_bls_verify_line_table_batch it has no one-wavefront route (that route walks the point). */
/* @shape tau_table=i32[*] c_xy=u64[8*n] c_inf=u8[n]? z=u64[4*n] y=u64[4*n] pi_xy=u64[8*n] pi_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_kzg_verify_line_table_batch(const int32_t* tau_table, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z, const uint64_t* y,
                                              const uint64_t* pi_xy, const uint8_t* pi_inf, uint8_t* ok, size_t n, void* stream);
/* The SOUND one-boolean form, the move of sylow_hip_groth16_batch_verify_weighted: with weights r_i [4][n]
 *     e( sum_i r_i C_i + sum_i (r_i z_i) pi_i - (sum_i r_i y_i) G1gen , G2gen ) e( -sum_i r_i pi_i , tau_g2 ) == 1
 * -- one small kernel reduces r_i, r_i z_i and s = sum_i r_i y_i mod r (two levels) and concatenates the 2n bases and scalars; then one
 * sylow_hip_g1_msm over the 2n terms and one over the pi_i (whatever route it picks), one generator product, and
 * sylow_hip_pairing_product_batch over the two pairs with skip_infinity = 1: two Miller loops and ONE final exponentiation whatever n is.
 * gt_out [48][1] is the Gt element, hence the words, of the reference's glued_pairing over the two literal pairs written above, identity
 * pairs left out; is_one [1] its comparison with the identity; either may be NULL (not both).  A weight of 0 removes an opening from the
 * test; n = 0 gives the identity.  The caller draws the weights AFTER the openings are fixed (e.g. 64 or 128 random bits each): if every
 * opening is valid the result is the identity; if any is not, the test passes with probability at most 2^-(bits of the weights) over the
 * caller's randomness, provided tau_g2 is in the r-torsion (the precondition above). */
/* @shape tau_g2_xy=u64[16] c_xy=u64[8*n] c_inf=u8[n]? z=u64[4*n] y=u64[4*n] pi_xy=u64[8*n] pi_inf=u8[n]? weights=u64[4*n] gt_out=u64[48]? is_one=u8[1]? */
int32_t sylow_hip_kzg_batch_verify_weighted(const uint64_t* tau_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* z, const uint64_t* y,
                                            const uint64_t* pi_xy, const uint8_t* pi_inf, const uint64_t* weights, size_t n,
                                            uint64_t* gt_out, uint8_t* is_one, void* stream);

/* ---- KZG, the prover's side: commit to and open polynomials under ONE SRS (kzg_prove.hip; geometry and routes in kzg_prove_plan.hpp) ----
 * The G1 half of the SRS as the prover holds it: srs_g1_xy [8][len], the affine points tau^k G1gen for k = 0 .. len - 1, WITHOUT a flag array.
 * Conventions of the four calls (those of the KZG block above):
 *   polynomials: m polynomials of len coefficients each (len >= 1), lowest degree first.  Each is an ordinary Fr SoA array [4][len] and the m
 *              arrays lie one after another -- coeffs [m][4][len], word w of coefficient k of polynomial j at (j * 4 + w) * len + k -- so that
 *              polynomial j is, as it lies, an array of len scalars of stride len.  A shorter polynomial is padded with zeros by the caller; a
 *              host with a longer SRS passes a packed prefix of it (the SoA stride is len).
 *   scalars:   coefficients and z are ANY 256-bit words, taken mod r (NOT like Fp::new first: a coefficient word >= p is its residue mod r).
 *   words:     coordinate words >= p are reduced like Fp::new, as everywhere.
 *   points:    taken as given: no on-curve check, no subgroup check.
 *   outputs:   q_out [m][4][len] in the layout of coeffs, canonical words below r, q_{len - 1} = 0 written; y [4][m]; points as [8][m] affine +
 *              [m] flags, the identity as (0, 1) + its flag.
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call.  len = 0: SYLOW_HIP_E_ARG.  m = 0: OK, nothing launched,
 *              nothing written.  NULL where a pointer is required: SYLOW_HIP_E_ARG, no launch, nothing written. */
/* q_j(X) = (f_j(X) - f_j(z_j)) / (X - z_j) and y_j = f_j(z_j): the recurrence h_len = 0, h_k = f_k + z h_{k+1}; y = h_0, q_k = h_{k+1} for
 * k < len - 1, q_{len-1} = 0.  Exact in Fr.  Either output may be NULL, not both; q_out = NULL is plain polynomial evaluation.  q_out must
 * NOT overlap coeffs.  A lane owns 8 consecutive coefficients, a block a chunk of 2048; a polynomial of at most one chunk is ONE launch,
 * a longer one three (chunk totals, one carry level, the chunks again). */
/* @shape coeffs=u64[4*len*m] z=u64[4*m] q_out=u64[4*len*m]? y_out=u64[4*m]? */
int32_t sylow_hip_kzg_quotient_batch(const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z,
                                     uint64_t* q_out, uint64_t* y_out, void* stream);
/* out_j = sum_k f_jk srs_k: the canonical affine words of one group element, hence identical on every route and for every chunking.
 * len >= the bucket route's crossover (that of sylow_hip_g1_msm): the coefficients mod r, then one sylow_hip_g1_msm_tuned per polynomial and
 * one gather.  Shorter: all m len (polynomial, term) pairs through ONE sylow_hip_g1_scalar_mul_batch and a segmented sum, in chunks of
 * whole polynomials that fit sylow_hip_set_scratch_limit (default 1 GB) at about 1.3 KB per pair; if not even one polynomial fits, each
 * goes through sylow_hip_g1_msm.  A zero polynomial (coefficients 0 mod r) and a sum that lands on the identity give (0, 1) + the flag. */
/* @shape srs_g1_xy=u64[8*len] coeffs=u64[4*len*m] out_xy=u64[8*m] out_inf=u8[m] */
int32_t sylow_hip_kzg_commit_batch(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m,
                                   uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* The same with the plan pinned, as sylow_hip_g1_msm_tuned: window (4..16, < 0 = the default) is passed to the bucket route; min_len is the
 * smallest len that takes it (< 0 = the default, 0 = always).  The points do not depend on either. */
/* @shape srs_g1_xy=u64[8*len] coeffs=u64[4*len*m] out_xy=u64[8*m] out_inf=u8[m] */
int32_t sylow_hip_kzg_commit_batch_tuned(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m,
                                         int32_t window, int64_t min_len, uint64_t* out_xy, uint8_t* out_inf, void* stream);
/* The opening of f_j at z_j: y_j = f_j(z_j) and pi_j = commit(q_j) -- the quotient into leased scratch, then the commitment of the quotients
 * over the same SRS.  pi_j is flagged as the identity exactly when q_j = 0 (f_j constant), the case sylow_hip_kzg_verify_batch reads as
 * "valid iff C = y G1gen".  (C, z, y, pi) with C from sylow_hip_kzg_commit_batch is a valid row of the verifiers above under tau_g2. */
/* @shape srs_g1_xy=u64[8*len] coeffs=u64[4*len*m] z=u64[4*m] y_out=u64[4*m] pi_xy=u64[8*m] pi_inf=u8[m] */
int32_t sylow_hip_kzg_open_batch(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, const uint64_t* z,
                                 uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream);
/* The commitment of m polynomials given by their VALUES on the domain of n = 2^log_n points (evals [m][4][n], evals_ji = f_j(w_n^i), any words,
 * taken mod r): sylow_hip_fr_ntt_batch(inverse = 1, no shift) into leased scratch, then sylow_hip_kzg_commit_batch over len = n -- the same
 * canonical words as committing the interpolated coefficients.  srs_g1_xy is [8][n].  log_n < 0 or > 28: SYLOW_HIP_E_ARG. */
/* @shape srs_g1_xy=u64[8*2**log_n] evals=u64[4*2**log_n*m] out_xy=u64[8*m] out_inf=u8[m] */
int32_t sylow_hip_kzg_commit_evals_batch(const uint64_t* srs_g1_xy, const uint64_t* evals, int32_t log_n, size_t m,
                                         uint64_t* out_xy, uint8_t* out_inf, void* stream);

/* ---- KZG, the prover's side, from evaluations: open polynomials held by their VALUES on a radix-2 domain, without leaving that form
 * (kzg_evals.hip; geometry and scratch in kzg_evals_plan.hpp) -----------------------------------------------------------------------------
 * Conventions (those of the transform block and of the KZG prover block above):
 *   polynomials: evals [m][4][n], n = 2^log_n, 0 <= log_n <= 28: evals_ji = f_j(w_n^i) with w_n the root of the transform block, natural
 *              order; f_j is THE polynomial of degree < n through those values.  z is [4][m].  Every word is taken mod r.
 *   the SRS:   srs_lagrange_xy [8][n], the affine points L_i(tau) G1gen with L_i the Lagrange basis of the same domain,
 *              L_i(tau) = (tau^n - 1) w^i / (n (tau - w^i)); supplied by the caller (ceremony files ship it), taken as given, no flag array.
 *   outputs:   y_out [4][m]; q_out [m][4][n] in the layout of evals; canonical words below r; points as [8][m] affine + [m] flags.
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call.  m = 0: OK, nothing launched, nothing written.
 *   errors:    SYLOW_HIP_E_ARG, no launch, nothing written, for: log_n < 0 or > 28; a required pointer NULL; q_out overlapping evals (the two
 *              byte ranges of 32 n m bytes are compared).
 * A COMMITMENT from evaluations under a Lagrange-basis SRS needs no entry point of its own: sum_i f_j(w^i) L_i(tau) G1gen = f_j(tau) G1gen is
 * sylow_hip_kzg_commit_batch(srs_lagrange_xy, evals, n, m, ...) as it stands -- the same point sylow_hip_kzg_commit_evals_batch yields under
 * the monomial SRS of the same tau. */
/* y_j = f_j(z_j) and the values on the domain of q_j(X) = (f_j(X) - y_j) / (X - z_j), exact in Fr.  With d_i = z - w^i:
 *   z outside the domain:   y = (z^n - 1) n^-1 sum_i f_i w^i d_i^-1 (the barycentric formula),   q_i = (y - f_i) d_i^-1;
 *   z = w^k mod r (however the word was written):   y = f_k,   q_i = (y - f_i) d_i^-1 for i != k,   q_k = -w^-k sum_(i != k) q_i w^i = f_j'(w^k).
 * A batch may mix rows of both kinds; at log_n = 0, y = f_0 and q_0 = 0 for every z.  Either output may be NULL, not both; q_out = NULL is
 * barycentric evaluation alone.  The d_i^-1 share one inversion per chunk of 2048 points (the mechanism of sylow_hip_fr_batch_inv; inv(0) = 0
 * marks the hit, whose q_k one lane repairs after the second sum).  Five launches with q_out (the powers of w_n once per call; d_i^-1 and
 * the first sum per chunk; y per polynomial; q per chunk; the repair), three without.  Scratch: 32 bytes per (polynomial, chunk) and 8 (40
 * without y_out) per polynomial, plus 928. */
/* @shape evals=u64[4*2**log_n*m] z=u64[4*m] q_out=u64[4*2**log_n*m]? y_out=u64[4*m]? */
int32_t sylow_hip_kzg_quotient_evals_batch(const uint64_t* evals, int32_t log_n, size_t m, const uint64_t* z,
                                           uint64_t* q_out, uint64_t* y_out, void* stream);
/* The opening of f_j at z_j from its values: y_j as above and pi_j = sum_i q_j(w^i) srs_lagrange_i = q_j(tau) G1gen -- the quotient's values
 * into leased scratch (32 n m bytes), then the commitment code of sylow_hip_kzg_commit_batch over them, entered past its mod-r pass since the
 * words are canonical.  pi_j is flagged as the identity exactly when q_j = 0 (f_j constant).  (C, z, y, pi) with C from
 * sylow_hip_kzg_commit_batch(srs_lagrange_xy, evals, ...) is a valid row of the verifiers above under tau_g2; the words are those
 * sylow_hip_kzg_open_batch yields for the interpolated coefficients under the monomial SRS of the same tau. */
/* @shape srs_lagrange_xy=u64[8*2**log_n] evals=u64[4*2**log_n*m] z=u64[4*m] y_out=u64[4*m] pi_xy=u64[8*m] pi_inf=u8[m] */
int32_t sylow_hip_kzg_open_evals_batch(const uint64_t* srs_lagrange_xy, const uint64_t* evals, int32_t log_n, size_t m, const uint64_t* z,
                                       uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream);

/* ---- KZG, the prover's side: every point of the domain at once (kzg_open_all.hip; geometry, ping-pong and scratch in kzg_open_all_plan.hpp) ----
 * The n proofs of ONE polynomial of n = 2^log_n coefficients at all n points w_n^i of its domain, in n log n instead of n^2 (Feist-Khovratovich):
 *   pi_i = q_i(tau) G1gen,  q_i = (f - f(w^i)) / (X - w^i)   =   sum_b w^(ib) h_b,   h_b = sum_(t = 0 .. n-2-b) f_(b+1+t) s_t,   h_(n-1) = identity,
 * a forward transform (that of sylow_hip_g1_ntt_batch) of a Toeplitz product, and the Toeplitz product a cyclic convolution of 2n points:
 * h = the first n points of G1-INTT_2n(F_i T_i) with F = the Fr transform of (f, then n zeros) and T the transform of x, x_(2n-1-t) = s_t
 * for t = 0 .. n-2 and the identity elsewhere (s_(n-1) is not used).  T depends on the SRS alone and serves every polynomial.
 * Conventions (those of the transform blocks and of the KZG prover block above):
 *   the SRS:   srs_g1_xy [8][n], the affine points s_t = tau^t G1gen, taken as given, no flag array.
 *   the table: table_xy [8][2n] + table_inf [2n], canonical affine words, the identity as (0, 1) + its flag.  Read back, a flagged entry is the
 *              identity whatever its words hold, and so is (0, 1) without a flag; table_inf may then be NULL.
 *   polynomials: coeffs [m][4][n], 0 <= log_n <= 27 (the transform of 2n points must fit the 2^28 roots); ANY 256-bit words, taken mod r.
 *   outputs:   y_out [m][4][n] in the layout of coeffs, y_ji = f_j(w^i), canonical words below r (the forward Fr transform; may be NULL);
 *              pi_xy [m][8][n] + pi_inf [m][n] (required): the proofs as canonical affine words, the identity as (0, 1) + its flag, in the
 *              layout of sylow_hip_g1_ntt_batch.  They do NOT depend on the plan (max_blocks below).  Row (C_j, w^i, y_ji, pi_ji) with C_j from
 *              sylow_hip_kzg_commit_batch is a valid row of the verifiers above under tau_g2, and pi_ji is word for word what
 *              sylow_hip_kzg_open_batch yields for f_j at z = w^i.
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call, summed in saturating arithmetic and refused before the lease.
 *              m = 0: OK, nothing launched, nothing written.
 *   errors:    SYLOW_HIP_E_ARG, no launch, nothing written, for: log_n < 0 or > 27; a required pointer NULL; max_blocks == 0; y_out
 *              overlapping coeffs; pi_xy overlapping coeffs or table_xy. */
/* T of the block above from the monomial SRS: x into leased scratch (130 n bytes), then sylow_hip_g1_ntt_batch over 2n points, forward, m = 1
 * -- word for word what that call returns for x.  Once per SRS.  A SET FLAG IS AN OUTPUT, NOT AN ERROR: at log_n = 0 both entries are the
 * identity, and a special tau gives others (T_0 = (1 + tau + .. + tau^(n-2)) G1gen is the identity for log_n = 2 and 4 when tau^3 = 1). */
/* @shape srs_g1_xy=u64[8*2**log_n] table_xy=u64[16*2**log_n] table_inf=u8[2*2**log_n] */
int32_t sylow_hip_kzg_open_all_prepare(const uint64_t* srs_g1_xy, int32_t log_n, uint64_t* table_xy, uint8_t* table_inf, void* stream);
/* The proofs of m polynomials at every point of the domain, and their values there.  Per call: the forward Fr transform into y_out; (2n)^-1 f
 * padded to 2n and its Fr transform F into scratch (the scale of the inverse transform as ONE Fr PRODUCT per coefficient, not a scalar
 * multiplication per point); one launch for the pointwise products fused with stage 0 of the inverse transform (two scalar multiplications
 * from the affine table per butterfly); log_n launches of the stage kernel of sylow_hip_g1_ntt_batch for the rest of it; one launch for
 * stage 0 of the forward transform of n points, which reads h where the inverse left it and takes h_(n-1) as the identity; log_n - 1 stage
 * launches and the closing launch without a scale: one Fp inversion per proof.  Nothing between F and the affine proofs leaves the device or
 * projective form.  About 1.5 n log_n scalar multiplications per polynomial: 2n + (n (log_n - 1) + 1) + ((n / 2)(log_n - 2) + 1).
 * Scratch: two projective buffers of 192 n m bytes each (F lies in one of them), twiddle tables of 48 n bytes, window tables of 1 KB per
 * RESIDENT lane (128 MB by default).  log_n = 0: the one proof is the identity, y_j0 = f_j0 mod r.  A zero or constant polynomial has every
 * proof flagged. */
/* @shape table_xy=u64[16*2**log_n] table_inf=u8[2*2**log_n]? coeffs=u64[4*2**log_n*m] y_out=u64[4*2**log_n*m]? pi_xy=u64[8*2**log_n*m] pi_inf=u8[2**log_n*m] */
int32_t sylow_hip_kzg_open_all_batch(const uint64_t* table_xy, const uint8_t* table_inf, const uint64_t* coeffs, int32_t log_n, size_t m,
                                     uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream);
/* The same with the blocks of a multiplying launch capped, as sylow_hip_g1_ntt_batch_tuned: max_blocks >= 1 (at most 4096; more is 4096),
 * < 0 = the default (512).  The values do not depend on it. */
/* @shape table_xy=u64[16*2**log_n] table_inf=u8[2*2**log_n]? coeffs=u64[4*2**log_n*m] y_out=u64[4*2**log_n*m]? pi_xy=u64[8*2**log_n*m] pi_inf=u8[2**log_n*m] */
int32_t sylow_hip_kzg_open_all_batch_tuned(const uint64_t* table_xy, const uint8_t* table_inf, const uint64_t* coeffs, int32_t log_n, size_t m,
                                           int64_t max_blocks, uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream);

/* ---- KZG, folded openings: many polynomials opened at one point under ONE proof (kzg_multi.hip; tiles, grids, the flush length, scratch and
 * the chunks of the combined commitments in kzg_multi_plan.hpp) ---------------------------------------------------------------------------
 * What a PLONK-style prover sends: at the evaluation challenge it opens a dozen polynomials, at a shifted point one or two more, and it sends
 * ONE proof per point, formed from the polynomials folded under a challenge gamma.  The m polynomials fall into G GROUPS of consecutive
 * polynomials; group g holds the polynomials group_start[g] .. group_start[g + 1] - 1, is opened at z_g and folded under gamma_g.  With
 * i = j - group_start[g] the index of polynomial j inside its group, and 0^0 = 1:
 *     F_g = sum_j gamma_g^i f_j        y_j = f_j(z_g)        pi_g = commit((F_g - F_g(z_g)) / (X - z_g))
 *     C_F,g = sum_j gamma_g^i C_j      y_F,g = sum_j gamma_g^i y_j
 * and (C_F,g, z_g, y_F,g, pi_g) is a row of the verifiers of the KZG block above.  An empty group gives F = 0, y_F = 0, C_F = the identity
 * ((0, 1) + its flag) and pi = the identity.
 * Conventions (those of the KZG prover blocks above):
 *   polynomials: coeffs [m][4][len], or evals [m][4][n] with n = 2^log_n, as in those blocks.
 *   group_start: a HOST array of G + 1 uint64_t -- the host plans scratch, padded layouts and per-group routes from it, and no call of this
 *              library synchronises a stream to read an argument.  Non-decreasing, group_start[0] = 0, group_start[G] = m; anything else is
 *              SYLOW_HIP_E_ARG before anything is enqueued.  An empty group is legal.  IT IS READ BEFORE THE CALL RETURNS and may be freed or
 *              overwritten then: its values reach the device inside kernel arguments (256 offsets per launch of a one-block kernel that
 *              stores them to leased scratch), and a launch copies its arguments before it returns -- no copy engine, no pinned staging
 *              buffer, no synchronisation.
 *   scalars:   z [4][G], gamma [4][G], weights [4][m] and y [4][m] are DEVICE arrays; ANY 256-bit words, taken mod r.  Outputs are canonical
 *              words below r.
 *   points:    [8][.] affine SoA words + flags, the identity as (0, 1) + its flag; taken as given; coordinate words >= p are reduced like
 *              Fp::new, as everywhere.
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call.  G = 0 or m = 0 is the EMPTY BATCH: OK, nothing launched,
 *              nothing written (not even the zeros of empty groups).  NULL where an array is required, or len = 0: SYLOW_HIP_E_ARG, no
 *              launch, nothing written.
 *   soundness: THE LIBRARY DRAWS NO CHALLENGE.  gamma_g must be drawn AFTER the commitments C_j and the claimed values y_j are fixed (a
 *              transcript hash of them); the weights of sylow_hip_kzg_batch_verify_weighted over the folded rows must be drawn AFTER the
 *              proofs pi_g are fixed.  A gamma known before the y_j are chosen lets a prover cancel a wrong value against another. */
/* out [G][4][len], out_g[k] = sum_{j in group g} weights_j a_j[k] mod r for a [m][4][len]; an empty group gives zeros.  The linear
 * combination of polynomials over Fr: the fold above with weights = the powers of gamma, a prover's linearisation polynomial with arbitrary
 * weights.  out must NOT overlap a (the byte ranges are compared: SYLOW_HIP_E_ARG).  ONE launch over (group, tile of 256 columns) work
 * items: a lane owns one coefficient column and walks the polynomials of its group, the four limb planes are read coalesced along k, the
 * weight of a polynomial is fetched once per block (16 at a time through LDS), and a lane adds up to 16 products UNREDUCED in 16 limbs per
 * Barrett reduction (the multiply-accumulate of sylow_hip_fr_spmv_batch; both factors are brought to canonical form at the load).  Group and
 * tile counts past the grid's caps are walked with a stride. */
/* @shape a=u64[4*len*m] weights=u64[4*m] group_start=u64[G+1] out=u64[4*len*G] */
int32_t sylow_hip_fr_lincomb_batch(const uint64_t* a, size_t len, size_t m, const uint64_t* weights, const uint64_t* group_start, size_t G,
                                   uint64_t* out, void* stream);
/* out [4][m], out_j = gamma_g^i for polynomial j of group g, i = j - group_start[g]; gamma = 0 gives 1, 0, 0, ...  One lane per polynomial,
 * square-and-multiply on i: the lanes stay independent and a lane runs at most 2 log2(i) products, where a walk along the group is serial
 * in its length. */
/* @shape gamma=u64[4*G] group_start=u64[G+1] out=u64[4*m] */
int32_t sylow_hip_fr_group_powers_batch(const uint64_t* gamma, const uint64_t* group_start, size_t G, size_t m, uint64_t* out, void* stream);
/* y_out [4][m] and pi [8][G] + flags [G] of the block above, from coefficients under the monomial SRS srs_g1_xy [8][len].  The powers and z_g
 * spread to its polynomials (one small launch); y through sylow_hip_kzg_quotient_batch with q_out = NULL; the linear combination into leased
 * scratch (32 G len bytes); then sylow_hip_kzg_open_batch over the G folded polynomials: pi_g is word for word what that call yields for
 * F_g.  A group whose F_g is constant -- an empty group and a fold that cancels to zero included -- gives the flagged identity. */
/* @shape srs_g1_xy=u64[8*len] coeffs=u64[4*len*m] group_start=u64[G+1] z=u64[4*G] gamma=u64[4*G] y_out=u64[4*m] pi_xy=u64[8*G] pi_inf=u8[G] */
int32_t sylow_hip_kzg_open_multi_batch(const uint64_t* srs_g1_xy, const uint64_t* coeffs, size_t len, size_t m, const uint64_t* group_start, size_t G,
                                       const uint64_t* z, const uint64_t* gamma, uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf, void* stream);
/* The same from evaluation form under the Lagrange-basis SRS srs_lagrange_xy [8][n]: y through sylow_hip_kzg_quotient_evals_batch with
 * q_out = NULL (points inside the domain included), the same linear combination over the VALUES (the fold is linear), then
 * sylow_hip_kzg_open_evals_batch over the G folded rows.  The words are those sylow_hip_kzg_open_multi_batch yields for the interpolated
 * coefficients under the monomial SRS of the same tau.  log_n < 0 or > 28: SYLOW_HIP_E_ARG. */
/* @shape srs_lagrange_xy=u64[8*2**log_n] evals=u64[4*2**log_n*m] group_start=u64[G+1] z=u64[4*G] gamma=u64[4*G] y_out=u64[4*m] pi_xy=u64[8*G] pi_inf=u8[G] */
int32_t sylow_hip_kzg_open_multi_evals_batch(const uint64_t* srs_lagrange_xy, const uint64_t* evals, int32_t log_n, size_t m, const uint64_t* group_start,
                                             size_t G, const uint64_t* z, const uint64_t* gamma, uint64_t* y_out, uint64_t* pi_xy, uint8_t* pi_inf,
                                             void* stream);
/* The verifier's half: cf_xy [8][G] + cf_inf [G] = C_F and yf [4][G] = y_F from the commitments c_xy [8][m] (+ optional flags) and the claimed
 * values y [4][m].  The powers; the m terms laid out term-major, every group padded to the longest with (identity, scalar 0), through ONE
 * sylow_hip_g1_scalar_mul_batch and a segmented sum, in chunks of whole groups that fit sylow_hip_set_scratch_limit at about 1.3 KB per
 * padded slot; a group at or above sylow_hip_g1_msm's crossover (or too long for the limit on its own) goes through sylow_hip_g1_msm.  The
 * words are the canonical affine words of one group element: the same on every route and for every chunking.  y_F is a modular sum from one
 * small launch (a block per group). */
/* @shape c_xy=u64[8*m] c_inf=u8[m]? y=u64[4*m] group_start=u64[G+1] gamma=u64[4*G] cf_xy=u64[8*G] cf_inf=u8[G] yf=u64[4*G] */
int32_t sylow_hip_kzg_combine_openings_batch(const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* y, size_t m, const uint64_t* group_start, size_t G,
                                             const uint64_t* gamma, uint64_t* cf_xy, uint8_t* cf_inf, uint64_t* yf, void* stream);
/* ok [G]: sylow_hip_kzg_combine_openings_batch into leased scratch, then sylow_hip_kzg_verify_batch over the G rows (C_F,g, z_g, y_F,g, pi_g).
 * The one-boolean form needs no call of its own: combine, then sylow_hip_kzg_batch_verify_weighted over the G rows. */
/* @shape tau_g2_xy=u64[16] c_xy=u64[8*m] c_inf=u8[m]? y=u64[4*m] group_start=u64[G+1] z=u64[4*G] gamma=u64[4*G] pi_xy=u64[8*G] pi_inf=u8[G]? ok=u8[G] */
int32_t sylow_hip_kzg_verify_multi_batch(const uint64_t* tau_g2_xy, const uint64_t* c_xy, const uint8_t* c_inf, const uint64_t* y, size_t m,
                                         const uint64_t* group_start, size_t G, const uint64_t* z, const uint64_t* gamma, const uint64_t* pi_xy,
                                         const uint8_t* pi_inf, uint8_t* ok, void* stream);

/* ---- Groth16, the prover's side: R1CS products, the quotient and the proof under ONE proving key (groth16_prove.hip; lanes per row, grids,
 * scratch and chunks in groth16_prove_plan.hpp) ------------------------------------------------------------------------------------------
 * Conventions of the calls below (those of the transforms and of the KZG prover block):
 *   Fr arrays: [4][n] SoA words; batches are [m][4][n], m arrays one after another.  ANY 256-bit word is taken mod r on input (not like
 *              Fp::new first); outputs are canonical words below r.
 *   points:    G1 [8][n] / G2 [16][n] affine SoA words with an optional identity-flag array ([n] bytes, NULL = none flagged); outputs carry
 *              their flags, the identity as (0, 1) + its flag.  Taken as given: no on-curve check, no subgroup check.
 *   calls:     stream-ordered, no host synchronisation; scratch leased per call.  m = 0: OK, nothing launched, nothing written.  NULL where
 *              a pointer is required: SYLOW_HIP_E_ARG, no launch, nothing written. */
/* out_j = M w_j over Fr for a sparse matrix M in CSR and m vectors: row_ptr [rows + 1] (non-decreasing, row_ptr[rows] = nnz), col [nnz],
 * val [4][nnz]; w [m][4][n_cols]; out [m][4][n_out] with n_out >= rows:
 *     out_j[i] = sum over the entries e of row i of val_e w_j[col_e] mod r,     out_j[i] = 0 for rows <= i < n_out (the padding to a domain).
 * THE KERNEL NEVER READS OUTSIDE ITS ARRAYS, whatever the index arrays hold: an entry with col >= n_cols contributes zero, and a row's ends are
 * clamped to nnz (an end before its start is an empty row) -- a malformed matrix gives a wrong number, never a fault.  Column indices are
 * uint64_t because this header has no other unsigned integer array type.  n_out < rows, or a size whose byte count overflows:
 * SYLOW_HIP_E_ARG.  m = 0 or n_out = 0: OK, nothing launched.  2^k lanes share a row (k = 0 .. 6, from nnz / rows alone: a lane gets at least 8
 * entries of an average row); a lane adds up to 16 products UNREDUCED in 16 limbs per Barrett reduction; the vectors are brought to canonical
 * form once per call into leased scratch (32 n_cols m bytes, SoA as they came). */
/* @shape row_ptr=u64[rows+1] col=u64[nnz]? val=u64[4*nnz]? w=u64[4*n_cols*m]? out=u64[4*n_out*m] */
int32_t sylow_hip_fr_spmv_batch(const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t rows, size_t nnz, const uint64_t* w,
                                size_t n_cols, size_t m, size_t n_out, uint64_t* out, void* stream);
/* The same with the lanes per row pinned: 2^lanes_log, lanes_log = 0 .. 6, < 0 = the default; more than 6: SYLOW_HIP_E_ARG.  The values do not
 * depend on it. */
/* @shape row_ptr=u64[rows+1] col=u64[nnz]? val=u64[4*nnz]? w=u64[4*n_cols*m]? out=u64[4*n_out*m] */
int32_t sylow_hip_fr_spmv_batch_tuned(const uint64_t* row_ptr, const uint64_t* col, const uint64_t* val, size_t rows, size_t nnz, const uint64_t* w,
                                      size_t n_cols, size_t m, size_t n_out, int32_t lanes_log, uint64_t* out, void* stream);
/* a, b, c [m][4][n], n = 2^log_n, 0 <= log_n <= 28: the values of three polynomials of degree < n on the domain <w_n> of the transforms above.
 * h_out [m][4][n]: the coefficients of THE polynomial of degree < n that equals (a b - c) / (X^n - 1) on the coset 5 <w_n>.  Where
 * a_i b_i = c_i on the whole domain that is the exact quotient, of degree <= n - 2, and h[n - 1] = 0 is written; otherwise it is what the
 * definition says, and no error is raised.  Three inverse transforms, three forward ones onto the coset, ONE element-wise kernel
 * (a b - c) zinv -- X^n - 1 is the constant 5^n - 1 there, its inverse a table of 29 constants -- and one inverse transform from the coset:
 * the 3 m arrays lie in one leased buffer, so it is three sylow_hip_fr_ntt_batch calls.  Scratch: 192 n m bytes and what those calls lease.
 * h_out may be a, b or c.  log_n < 0 or > 28: SYLOW_HIP_E_ARG. */
/* @shape a=u64[4*2**log_n*m] b=u64[4*2**log_n*m] c=u64[4*2**log_n*m] h_out=u64[4*2**log_n*m] */
int32_t sylow_hip_groth16_quotient_batch(const uint64_t* a, const uint64_t* b, const uint64_t* c, int32_t log_n, size_t m, uint64_t* h_out, void* stream);
/* m proofs for m witnesses of ONE circuit under ONE proving key, with the caller's randomness.
 *   circuit:   three CSR matrices A, B, C (a_*, b_*, c_* as in sylow_hip_fr_spmv_batch) of n_cons rows and n_vars columns; the domain has
 *              n = 2^log_n >= n_cons points; variable 0 is the constant 1, variables 1 .. n_inputs are public, n_inputs < n_vars.
 *   key:       arkworks' names.  alpha_g1, beta_g1, delta_g1 [8][1] and beta_g2, delta_g2 [16][1] WITHOUT flag arrays; a_query [8][n_vars],
 *              b_g1_query [8][n_vars], b_g2_query [16][n_vars], h_query [8][n - 1], l_query [8][n_vars - n_inputs - 1], each with its optional
 *              flag array (a variable absent from A or B has the identity there).  h_query and l_query may be NULL when they hold no point.
 *   witnesses: z [m][4][n_vars]; randomness r, s [4][m].  Any words, taken mod r.
 *   proofs:    A [8][m], B [16][m], C [8][m] with their flags -- what sylow_hip_groth16_verify_batch takes.
 * With h = the quotient above of (A z, B z, C z) padded to the domain:
 *     A  = alpha_g1 + sum_i z_i a_query_i + r delta_g1          B  = beta_g2 + sum_i z_i b_g2_query_i + s delta_g2
 *     B1 = beta_g1 + sum_i z_i b_g1_query_i + s delta_g1
 *     C  = sum_{i > n_inputs} z_i l_query_{i - n_inputs - 1} + sum_{k < n - 1} h_k h_query_k + s A + r B1 - (r s mod r) delta_g1
 * Per witness four sylow_hip_g1_msm and one sylow_hip_g2_msm (whatever route they pick) on canonical scalars; the closing sums run through
 * sylow_hip_g1_scalar_mul_batch / sylow_hip_g2_scalar_mul_batch / the add calls, one lane per witness.
 * THE LIBRARY CHECKS NEITHER z_0 = 1 NOR THAT THE CONSTRAINTS HOLD: an unsatisfied witness yields a proof the verifier rejects.
 * Witnesses go through in chunks of whole witnesses under sylow_hip_set_scratch_limit (default 1 GB; about 320 n + 64 n_vars bytes each and 16 n once); if
 * not even one fits: SYLOW_HIP_E_HIP, the code of a failed scratch allocation, with the bytes needed in sylow_hip_last_error.
 * log_n < 0 or > 28, n_cons > 2^log_n, n_inputs >= n_vars: SYLOW_HIP_E_ARG. */
/* @shape a_row_ptr=u64[n_cons+1] a_col=u64[a_nnz]? a_val=u64[4*a_nnz]? b_row_ptr=u64[n_cons+1] b_col=u64[b_nnz]? b_val=u64[4*b_nnz]? c_row_ptr=u64[n_cons+1] c_col=u64[c_nnz]? c_val=u64[4*c_nnz]? alpha_g1=u64[8] beta_g1=u64[8] delta_g1=u64[8] beta_g2=u64[16] delta_g2=u64[16] a_query=u64[8*n_vars] a_query_inf=u8[n_vars]? b_g1_query=u64[8*n_vars] b_g1_query_inf=u8[n_vars]? b_g2_query=u64[16*n_vars] b_g2_query_inf=u8[n_vars]? h_query=u64[*]? h_query_inf=u8[*]? l_query=u64[*]? l_query_inf=u8[*]? z=u64[4*n_vars*m] r=u64[4*m] s=u64[4*m] a_xy=u64[8*m] a_inf=u8[m] b_xy=u64[16*m] b_inf=u8[m] c_xy=u64[8*m] c_inf=u8[m] */
int32_t sylow_hip_groth16_prove_batch(const uint64_t* a_row_ptr, const uint64_t* a_col, const uint64_t* a_val, size_t a_nnz,
                                      const uint64_t* b_row_ptr, const uint64_t* b_col, const uint64_t* b_val, size_t b_nnz,
                                      const uint64_t* c_row_ptr, const uint64_t* c_col, const uint64_t* c_val, size_t c_nnz,
                                      size_t n_cons, size_t n_vars, size_t n_inputs, int32_t log_n,
                                      const uint64_t* alpha_g1, const uint64_t* beta_g1, const uint64_t* delta_g1,
                                      const uint64_t* beta_g2, const uint64_t* delta_g2,
                                      const uint64_t* a_query, const uint8_t* a_query_inf, const uint64_t* b_g1_query, const uint8_t* b_g1_query_inf,
                                      const uint64_t* b_g2_query, const uint8_t* b_g2_query_inf, const uint64_t* h_query, const uint8_t* h_query_inf,
                                      const uint64_t* l_query, const uint8_t* l_query_inf,
                                      const uint64_t* z, const uint64_t* r, const uint64_t* s, size_t m,
                                      uint64_t* a_xy, uint8_t* a_inf, uint64_t* b_xy, uint8_t* b_inf, uint64_t* c_xy, uint8_t* c_inf, void* stream);

/* ---- test hooks (stable enough for the repo's own tests; not part of the drop-in surface) ------------------------------------
 * Granger-Scott cyclotomic square (pairing.rs:309-350) and the raw Fp12 selector: 0..7 one-element-per-lane tower ops (tower.hip), 8 / 9 product /
 * cyclotomic square on the carry-free core, 10 / 11 exp_by_neg_z (carry-free / saturated), 16..31 the lane-pair Fp12 layer: 16 product,
 * 17 square, 18 sparse product (b = ell_0, ell_vw, ell_vv), 19 cyclotomic square, 20..22 Frobenius 1..3, 23 exp_by_neg_z, 24..27 product,
 * square, inverse, cyclotomic square on the saturated core, 28 conjugate, 29 sparse product with ell_0 = (element index & 1), 30 / 31 the
 * Miller loop's doubling / addition step (a = R (X, Y, Z) then Q (x, y); b = P (x, y); out = the new R then ell_0, ell_vw P.y, ell_vv P.x).
 * The same routines at the same offset on the other layouts: 32..47 lane quads (offsets 0..7, 13..15), 48..63 / 64..79 one wavefront per
 * one / two elements (offsets 0..7, 14, 15; 2 is the product by the line (ell_0, 0, ell_vv; 0, ell_vw, 0), 8 the final exponentiation,
 * 10 the inverse).  Another op, or a missing b where the op reads one, is SYLOW_HIP_E_ARG. */
/* @shape a=u64[48*n] out=u64[48*n] */
int32_t sylow_hip_fp12_cyclotomic_sqr_batch(const uint64_t* a, uint64_t* out, size_t n, void* stream);
/* @shape a=u64[48*n] b=u64[*]? out=u64[48*n] */
int32_t sylow_hip_fp12_hook_batch(int32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);

/* ---- value-typed forms: HOST arrays in, HOST results out (pipeline.hip) ------------------------------------------------------
 * The reference's API takes and returns values (pairing(&G1Projective, &G2Projective) -> Gt, pairing.rs:870-893;
 * verify(&G2Projective, &[u8], &G1Projective) -> bool, lib.rs:223-236): a host that switches holds arrays of structs in HOST memory.
 * These two calls are the batched forms on such arrays -- EVERY pointer is a HOST pointer, element-major ("array of structs", what a
 * Rust Vec<[u64; W]> is): p_aos [n][8] (x, y), q_aos / pk_aos [n][16], sig_aos [n][8], gt_aos [n][48], flags [n] (NULL = none), msgs +
 * msg_offsets [n + 1] as in sylow_hip_bls_verify_batch, ok [n].  The batch is cut into chunks -- `chunk` elements (0 = 2^16: one resident
 * set of lane pairs) first and last, up to four times that in between -- that alternate between two internal streams, each chunk H2D -> AoS->SoA -> the same kernels as the device-pointer
 * entry points -> D2H, issued so that the copy engines move chunk k - 1 out and chunk k + 1 in while chunk k computes.  Synchronous:
 * the results are in host memory when the call returns.  Bit-identical to upload + sylow_hip_pairing_batch /
 * sylow_hip_bls_verify_batch + download.  Pageable memory works; pinned memory (sylow_hip_host_malloc) makes every copy asynchronous. */
/* @shape p_aos=u64[8*n] p_inf=u8[n]? q_aos=u64[16*n] q_inf=u8[n]? gt_aos=u64[48*n] */
int32_t sylow_hip_pairing_host(const uint64_t* p_aos, const uint8_t* p_inf, const uint64_t* q_aos, const uint8_t* q_inf,
                               uint64_t* gt_aos, size_t n, size_t chunk);
/* @shape pk_aos=u64[16*n] pk_inf=u8[n]? msgs=u8[*]? msg_offsets=u64[n+1] sig_aos=u64[8*n] sig_inf=u8[n]? ok=u8[n] */
int32_t sylow_hip_bls_verify_host(const uint64_t* pk_aos, const uint8_t* pk_inf, const uint8_t* msgs, const uint64_t* msg_offsets,
                                  const uint64_t* sig_aos, const uint8_t* sig_inf, uint8_t* ok, size_t n, size_t chunk);
/* The same two pipelines fed with the reference's WIRE format, which is how a Rust host gets points across without relying on sylow's
 * (non-repr(C)) memory layout: p_be / sig_be [n][64] = G1Affine::to_be_bytes (g1.rs:151-180), q_be / pk_be [n][128] =
 * G2Affine::to_be_bytes (g2.rs:319-359).  Decoding and validation run on the device inside the pipeline (from_be_bytes + curve check;
 * G2 also the r-torsion check of G2Projective::new, g2.rs:460-525); status_* [n] (HOST) receive SYLOW_HIP_ST_* per element, and an
 * element that failed enters the computation as the identity: its Gt is one, and its `ok` is forced to ZERO -- the reference returns Err
 * from from_be_bytes / G2Projective::new and never reaches verify, and identity inputs can satisfy the pairing equation (a rejected key
 * with an all-zero signature), so a caller that reads only `ok` must not see 1 for a rejected blob.  msg_offsets must be non-decreasing
 * over the whole batch (checked on the host: SYLOW_HIP_E_ARG otherwise). */
/* @shape p_be=u8[64*n] q_be=u8[128*n] gt_aos=u64[48*n] status_p=u8[n] status_q=u8[n] */
int32_t sylow_hip_pairing_host_bytes(const uint8_t* p_be, const uint8_t* q_be, uint64_t* gt_aos, uint8_t* status_p, uint8_t* status_q,
                                     size_t n, size_t chunk);
/* @shape pk_be=u8[128*n] msgs=u8[*]? msg_offsets=u64[n+1] sig_be=u8[64*n] ok=u8[n] status_pk=u8[n] status_sig=u8[n] */
int32_t sylow_hip_bls_verify_host_bytes(const uint8_t* pk_be, const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* sig_be,
                                        uint8_t* ok, uint8_t* status_pk, uint8_t* status_sig, size_t n, size_t chunk);
/* page-locked host memory for the staging side of the calls above (hipHostMalloc / hipHostFree) */
int32_t sylow_hip_host_malloc(void** hptr, size_t bytes);
int32_t sylow_hip_host_free(void* hptr);

#ifdef __cplusplus
}
#endif
#endif /* SYLOW_HIP_H */
