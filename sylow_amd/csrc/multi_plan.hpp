// multi_plan.hpp -- which schedule runs a multi-pair call (plk_multi.hip, groth16_pair.hpp), and how its line tables are sliced: every
// decision between an entry point and its kernels, plain C++ so that tests/cpp/multi_plan_test.cpp can compile it with g++ on a box
// without a GPU.  The launch code reads the knobs once per entry-point call and asks these functions; it decides nothing itself.
#pragma once
#include <cstddef>

namespace multi_plan {
// line-table geometry (k_pair_lines' layout): 87 lines per pair, each 7 chunks of 16 bytes per lane, two lanes per pair
constexpr int LT_CHUNKS = 7;
constexpr int LT_LINES = 87;
constexpr size_t CHUNK_PAIR_BYTES = 32;
constexpr size_t ROUND = 65536;          // the lane pairs one GPU round holds
constexpr size_t JOB_BLOCK = 1024;       // the table route slices a batch into blocks of at least this many jobs
constexpr int KMAXW = 4;                 // ecPairing / glued jobs (a few pairs each)
constexpr int KPROD = 8;                 // batch-wide product: more pairs per shared squaring

// bytes of line tables one job of kt slots takes
constexpr size_t table_bytes_per_job(size_t kt) { return (size_t)LT_LINES * kt * LT_CHUNKS * CHUNK_PAIR_BYTES; }
// slots per job: the batch average, rounded up, 1..8; longer jobs take the in-register tail
inline size_t table_slots(size_t n_jobs, size_t n_pairs) {
  const size_t kt = n_jobs ? (n_pairs + n_jobs - 1) / n_jobs : 1;
  return kt < 1 ? 1 : kt > 8 ? 8 : kt;
}

// The knobs in force for one entry-point call.
struct Knobs {
  int tables_mode;       // SYLOW_HIP_OPT_MULTI_TABLES: 0 never tables, 1 tables whatever the job size (A/B runs), anything else the default
  size_t budget;         // bytes the line tables of the call may take (sylow_hip_set_scratch_limit, or the default)
  size_t wide_cap;       // the one-wavefront routes' cap in Miller loops; 0 when the small-batch routes are off
  bool small_routes;     // SYLOW_HIP_OPT_WIDE_TAIL != 0
};

enum class Route {
  ONE_WAVE_JOBS,         // a wavefront per Miller loop, then a wavefront per job (single_job_product)
  TABLES,                // line tables in HBM (multi_pairing_tables)
  SLOTS_2,               // k_multi_pairing<2>
  SLOTS_KMAXW,           // k_multi_pairing<KMAXW>
  SLOTS_KPROD,           // k_multi_pairing<KPROD>
  SINGLE_WIDE,           // the batch-wide product of ONE pair: k_miller_single_wide
  WIDE_BATCH,            // the batch-wide product of few pairs: k_miller_wide_batch, a value per pair
};

// FEW jobs with few pairs.  EIP-197 reading of identities only (skip_infinity): the one-wavefront kernels have no replay mode.
inline bool single_job_route(const Knobs& k, size_t n_jobs, size_t n_pairs, bool skip_infinity) {
  return k.wide_cap != 0 && n_pairs >= 1 && n_pairs <= k.wide_cap && n_jobs <= JOB_BLOCK && skip_infinity;
}
// The table route slices a batch into blocks of at least 1024 jobs: a budget below 1024 jobs' tables (20 - 160 MB by the job size) cannot be
// honoured by it, so such a batch takes the in-register schedule (no table at all) -- the bound a host sets is never silently exceeded.
inline bool use_tables(const Knobs& k, size_t n_jobs, size_t n_pairs) {
  if (k.tables_mode == 0) return false;
  if (k.tables_mode != 1 && n_pairs < 2 * n_jobs) return false;     // below two pairs per job on average the in-register loops win
  if (!n_pairs) return false;                                       // mode 1 included: nothing to tabulate
  const size_t need = table_bytes_per_job(table_slots(n_jobs, n_pairs)) * (n_jobs < JOB_BLOCK ? n_jobs : JOB_BLOCK);
  return need <= k.budget;
}
// Jobs (n_jobs > 0): sylow_hip_multi_pairing_batch and sylow_hip_evm_ecpairing_batch (raw_glued = false), and the raw glued Miller loop.
//   raw_glued: never ONE_WAVE_JOBS (its kernels work on the isomorphic curves: not the reference's raw value) and never SLOTS_2 --
//              a batch of one-pair jobs runs <KMAXW> there, as it always has.
//   n_pairs == 0: no route above SLOTS_2 takes it (SLOTS_KMAXW for raw_glued); the kernel runs over jobs that hold nothing.
//   n_pairs == 2 n_jobs exactly: tables if the budget allows, else SLOTS_2 (`<=`), not SLOTS_KMAXW.
//   TABLES may still end on SLOTS_KMAXW, whatever the average job size: table_fallback().
inline Route job_route(const Knobs& k, size_t n_jobs, size_t n_pairs, bool skip_infinity, bool raw_glued) {
  if (!raw_glued && single_job_route(k, n_jobs, n_pairs, skip_infinity)) return Route::ONE_WAVE_JOBS;
  if (use_tables(k, n_jobs, n_pairs)) return Route::TABLES;
  if (!raw_glued && n_pairs <= 2 * n_jobs) return Route::SLOTS_2;
  return Route::SLOTS_KMAXW;
}
// a table lease that fails even at one round: the in-register schedule needs no workspace
constexpr Route table_fallback() { return Route::SLOTS_KMAXW; }

// The batch-wide product (n_pairs > 0).  Pairs per lane pair: as few as keep the whole product inside ONE round of the GPU, at most KPROD --
// a small product is latency-bound (one Miller loop deep), a large one throughput-bound (shared squarings).
inline size_t product_chunk(size_t n_pairs) {
  const size_t chunk = (n_pairs + ROUND - 1) / ROUND;
  return chunk > (size_t)KPROD ? (size_t)KPROD : chunk;
}
//   SINGLE_WIDE asks for small_routes, WIDE_BATCH only for n_pairs <= wide_cap (which is 0 when they are off).
//   `range` (one job of a multi-pairing batch) rules WIDE_BATCH out, not SINGLE_WIDE: that kernel reads the range itself.
//   TABLES: the budget test is ONE ROUND of chunk-slot jobs (not use_tables' 1024), and mode 1 waives it -- the slicer then takes
//           blocks of 1024 jobs whatever the budget.  No `average of two pairs` test: chunk >= 2 is that test.
//   chunk == 2 without tables runs <KMAXW>, three and more <KPROD>; chunk == 1 beyond the wide cap <KMAXW> (its one-pair loop).
inline Route chunk_route(const Knobs& k, size_t n_pairs, bool has_range, bool skip_infinity) {
  const size_t chunk = product_chunk(n_pairs);
  if (n_pairs == 1 && skip_infinity && k.small_routes) return Route::SINGLE_WIDE;
  if (chunk == 1 && !has_range && skip_infinity && n_pairs <= k.wide_cap) return Route::WIDE_BATCH;
  if (chunk >= 2 && k.tables_mode != 0 && (table_bytes_per_job(chunk) * ROUND <= k.budget || k.tables_mode == 1)) return Route::TABLES;
  return chunk <= 2 ? Route::SLOTS_KMAXW : Route::SLOTS_KPROD;
}

// Groth16: the per-proof table route (one slot per proof), or the COMPOSED route through sylow_hip_multi_pairing_batch.  Composed
// whenever that entry would take its one-wavefront route for the 4 n literal pairs; mode 1 forces nothing here (any mode but 0 is "on").
inline bool groth16_tables(const Knobs& k, size_t n) {
  return !single_job_route(k, n, 4 * n, true) && k.tables_mode != 0 && table_bytes_per_job(1) * (n < JOB_BLOCK ? n : JOB_BLOCK) <= k.budget;
}

// Jobs per slice of a table route: whole rounds of the GPU's 2^16 resident lane pairs while the budget allows; under a budget below one
// round as many jobs as fit, in blocks of 1024 -- phase B / C then run under-filled, the price of the bound -- and never fewer than 1024
// (the floor exceeds a budget below 1024 jobs' tables: the predicates above decline before that case is reached, mode 1 of the chunk
// route excepted).
inline size_t slice_jobs(size_t budget, size_t per_job, size_t n_jobs) {
  const size_t rounds = budget / (per_job * ROUND);
  size_t slice = rounds >= 1 ? rounds * ROUND : (budget / per_job) & ~(JOB_BLOCK - 1);
  if (slice < JOB_BLOCK) slice = JOB_BLOCK;
  return n_jobs < slice ? n_jobs : slice;
}
// a device short of memory (the lease of jb_max jobs failed): one round per slice, or 0 = nothing smaller to try
inline size_t slice_retry(size_t jb_max) { return jb_max > ROUND ? ROUND : 0; }
}  // namespace multi_plan
