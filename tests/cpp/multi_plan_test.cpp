// CPU-only check of the multi-pair planner (sylow_amd/csrc/multi_plan.hpp): table geometry, the slice rule, and the three route
// functions on grids.  Every expected value below is written by hand from the rules the launch code followed before the planner
// existed (quirks included); nothing is derived from the header: no constant, no helper of it appears on the expected side.
#include "../../sylow_amd/csrc/multi_plan.hpp"

#include <cstdio>
#include <initializer_list>

using namespace multi_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const char* name(Route r) {
  switch (r) {
    case Route::ONE_WAVE_JOBS: return "ONE_WAVE_JOBS";
    case Route::TABLES: return "TABLES";
    case Route::SLOTS_2: return "SLOTS_2";
    case Route::SLOTS_KMAXW: return "SLOTS_KMAXW";
    case Route::SLOTS_KPROD: return "SLOTS_KPROD";
    case Route::SINGLE_WIDE: return "SINGLE_WIDE";
    case Route::WIDE_BATCH: return "WIDE_BATCH";
  }
  return "?";
}
static const size_t GB12 = (size_t)12 << 30, MB64 = (size_t)64 << 20;
static const int MODES[3] = {-1, 0, 1};      // the default, never tables, tables whatever the job size

static void geometry_and_slices() {
  EXPECT(table_bytes_per_job(1) == 19488, "%zu", table_bytes_per_job(1));      // 87 lines x 7 chunks x 32 bytes
  EXPECT(table_bytes_per_job(2) == 38976, "%zu", table_bytes_per_job(2));
  EXPECT(table_bytes_per_job(8) == 155904, "%zu", table_bytes_per_job(8));
  EXPECT(LT_LINES == 87 && LT_CHUNKS == 7 && ROUND == 65536 && JOB_BLOCK == 1024 && KMAXW == 4 && KPROD == 8, "constants");
  // the batch average, rounded up, within 1..8
  const size_t slots[][3] = {{0, 0, 1}, {0, 7, 1}, {4, 0, 1}, {4, 1, 1}, {4, 4, 1}, {4, 5, 2}, {4, 8, 2}, {4, 9, 3}, {1, 8, 8}, {1, 9, 8}, {4, 32, 8}, {4, 33, 8}, {1025, 2050, 2}, {1025, 2051, 3}};
  for (const auto& s : slots) EXPECT(table_slots(s[0], s[1]) == s[2], "table_slots(%zu, %zu) = %zu", s[0], s[1], table_slots(s[0], s[1]));
  // whole rounds under the budget; below a round a multiple of 1024; never fewer than 1024; never more than the batch
  EXPECT(slice_jobs(GB12, 19488, 1u << 20) == 655360, "%zu", slice_jobs(GB12, 19488, 1u << 20));       // 10 rounds of 1 277 165 568 bytes
  EXPECT(slice_jobs(MB64, 19488, 1u << 20) == 3072, "%zu", slice_jobs(MB64, 19488, 1u << 20));         // 3443 jobs fit
  EXPECT(slice_jobs((size_t)1024 * 19488, 19488, 1u << 20) == 1024, "exactly 1024 jobs' tables");
  EXPECT(slice_jobs((size_t)1024 * 19488 - 1, 19488, 1u << 20) == 1024, "the floor (the predicates decline before this is reached)");
  EXPECT(slice_jobs((size_t)65536 * 19488, 19488, 1u << 20) == 65536, "one round exactly");
  EXPECT(slice_jobs((size_t)65536 * 19488 - 1, 19488, 1u << 20) == 64512, "one byte below a round: 65535 fit, 63 blocks of 1024");
  EXPECT(slice_jobs(GB12, 38976, 1u << 20) == 327680, "two slots: 5 rounds");
  EXPECT(slice_jobs(GB12, 19488, 70000) == 70000 && slice_jobs(MB64, 19488, 3071) == 3071 && slice_jobs(MB64, 19488, 1) == 1, "n_jobs below the slice");
  EXPECT(slice_retry(655360) == 65536 && slice_retry(65537) == 65536, "retry at one round");
  EXPECT(slice_retry(65536) == 0 && slice_retry(3072) == 0 && slice_retry(1) == 0, "nothing smaller to try");
}

// n_jobs in {1, 1024, 1025} x average pairs per job in {0, 1, 2, 3, 9} x skip_infinity x mode x wide cap {0, 6144} x three budgets, for
// sylow_hip_multi_pairing_batch / ecPairing (raw = 0) and the raw glued loop (raw = 1).  The expectation, cell by cell:
//   slots per job: 1, 1, 2, 3, 8 for the five averages, so per_job = 19488, 19488, 38976, 58464, 155904 bytes
//   the budgets: 12 GB holds 1024 jobs of any of these; 1024 * per_job holds exactly min(n_jobs, 1024) jobs; one byte less holds
//     them only for n_jobs = 1
//   the one-wavefront job route needs the cap (6144), skip_infinity, n_jobs <= 1024 and 1 <= n_pairs <= 6144: at n_jobs = 1 the
//     averages 1, 2, 3, 9; at n_jobs = 1024 the averages 1, 2, 3 (9216 pairs are too many); never at 1025; never for the raw loop
//   tables need a mode other than 0, at least one pair, the budget, and an average >= 2 unless the mode is 1
//   otherwise <2> for an average <= 2 (the empty batch included), else <KMAXW>; the raw loop runs <KMAXW> in both cases
static void job_grid() {
  const size_t n_jobs_v[3] = {1, 1024, 1025}, avg_v[5] = {0, 1, 2, 3, 9}, per_job_v[5] = {19488, 19488, 38976, 58464, 155904};
  for (int raw = 0; raw < 2; ++raw) for (size_t n_jobs : n_jobs_v) for (int a = 0; a < 5; ++a) for (int skip = 0; skip < 2; ++skip)
    for (int mode : MODES) for (size_t cap : {(size_t)0, (size_t)6144}) for (int bl = 0; bl < 3; ++bl) {
      const size_t avg = avg_v[a], n_pairs = avg * n_jobs;
      const size_t budget = bl == 0 ? GB12 : bl == 1 ? 1024 * per_job_v[a] : 1024 * per_job_v[a] - 1;
      const bool few = cap == 6144 && skip && ((n_jobs == 1 && avg >= 1) || (n_jobs == 1024 && avg >= 1 && avg <= 3));
      const bool one_wave = !raw && few;
      const bool fits = bl != 2 || n_jobs == 1;
      const bool tables = mode != 0 && avg >= 1 && (mode == 1 || avg >= 2) && fits;
      const Route want = one_wave ? Route::ONE_WAVE_JOBS : tables ? Route::TABLES : (!raw && avg <= 2) ? Route::SLOTS_2 : Route::SLOTS_KMAXW;
      const Knobs k{mode, budget, cap, cap != 0};
      const Route got = job_route(k, n_jobs, n_pairs, skip != 0, raw != 0);
      EXPECT(got == want, "job_route raw=%d n_jobs=%zu avg=%zu skip=%d mode=%d cap=%zu budget#%d: %s, expected %s", raw, n_jobs, avg, skip, mode, cap, bl, name(got), name(want));
      // the two predicates keep their names: what tests/test_gpu_evm_batches.py's docstrings refer to
      EXPECT(use_tables(k, n_jobs, n_pairs) == tables, "use_tables n_jobs=%zu avg=%zu mode=%d budget#%d", n_jobs, avg, mode, bl);
      EXPECT(single_job_route(k, n_jobs, n_pairs, skip != 0) == few, "single_job_route n_jobs=%zu avg=%zu skip=%d cap=%zu", n_jobs, avg, skip, cap);
    }
  // the documented batches of tests/test_gpu_evm_batches.py, default knobs of an empty MI355X (12 GB, cap 6144, skip_infinity)
  const Knobs dflt{-1, GB12, 6144, true};
  EXPECT(job_route(dflt, 368, 2256, true, false) == Route::ONE_WAVE_JOBS, "the pool as it is (368 jobs, 2256 pairs): n_jobs <= 1024, 1 <= n_pairs <= 6144");
  EXPECT(job_route(dflt, 1024, 6144, true, false) == Route::ONE_WAVE_JOBS && job_route(dflt, 1024, 6145, true, false) == Route::TABLES, "the cap, inclusive");
  EXPECT(job_route(dflt, 1104, 6768, true, false) == Route::TABLES, "the pool three times (1104 jobs, 6768 pairs): more than 1024 jobs, two pairs or more on average");
  EXPECT(job_route(dflt, 4959, 9852, true, false) == Route::SLOTS_2, "short jobs mixed in until n_pairs < 2 n_jobs (4959 jobs, 9852 pairs)");
  EXPECT(job_route(dflt, 1, 0, true, false) == Route::SLOTS_2 && job_route(dflt, 1500, 0, true, false) == Route::SLOTS_2, "n_pairs = 0");
  EXPECT(job_route(Knobs{0, GB12, 6144, true}, 1104, 6768, true, false) == Route::SLOTS_KMAXW, "MULTI_TABLES = 0: the four-slot schedule");
  EXPECT(job_route(Knobs{1, GB12, 6144, true}, 4959, 9852, true, false) == Route::TABLES, "MULTI_TABLES = 1: tables below two pairs per job");
  EXPECT(job_route(dflt, 1200, 2400, true, false) == Route::TABLES && job_route(Knobs{0, GB12, 6144, true}, 1200, 2400, true, false) == Route::SLOTS_2, "exactly two per job");
  EXPECT(job_route(dflt, 2048, 6144, false, true) == Route::TABLES && job_route(dflt, 2048, 2048, false, true) == Route::SLOTS_KMAXW, "the raw glued loop");
  EXPECT(table_fallback() == Route::SLOTS_KMAXW, "a table lease that fails: <KMAXW>, whatever the average job size");
}

// The batch-wide product: pairs per lane pair 1 up to 65536 pairs, 2 at 65537, 3 at 140000, 8 (the cap; 10 by the division) at 600000.
// One round of chunk-slot tables is 2.55 GB, 3.83 GB and 10.2 GB for chunks of 2, 3 and 8: inside 12 GB, outside 64 MB.
static void chunk_grid() {
  const size_t n_v[9] = {1, 2, 256, 6144, 6145, 65536, 65537, 140000, 600000}, chunk_v[9] = {1, 1, 1, 1, 1, 1, 2, 3, 8};
  for (int i = 0; i < 9; ++i) {
    EXPECT(product_chunk(n_v[i]) == chunk_v[i], "product_chunk(%zu) = %zu", n_v[i], product_chunk(n_v[i]));
    for (int range = 0; range < 2; ++range) for (int skip = 0; skip < 2; ++skip) for (int mode : MODES) for (size_t budget : {GB12, MB64}) {
      const size_t n = n_v[i];
      const bool tables = mode != 0 && (budget == GB12 || mode == 1);
      Route want;
      if (n == 1) want = skip ? Route::SINGLE_WIDE : Route::SLOTS_KMAXW;                               // the range does not matter
      else if (n <= 6144) want = (skip && !range) ? Route::WIDE_BATCH : Route::SLOTS_KMAXW;
      else if (n <= 65536) want = Route::SLOTS_KMAXW;                                                  // one pair per lane pair, in register
      else if (n == 65537) want = tables ? Route::TABLES : Route::SLOTS_KMAXW;                         // chunks of two without tables: <KMAXW>
      else want = tables ? Route::TABLES : Route::SLOTS_KPROD;
      const Route got = chunk_route(Knobs{mode, budget, 6144, true}, n, range != 0, skip != 0);
      EXPECT(got == want, "chunk_route n=%zu range=%d skip=%d mode=%d budget=%zu: %s, expected %s", n, range, skip, mode, budget, name(got), name(want));
    }
  }
  // the case tests/test_gpu_runtime.py (scratch limit bounds the line tables) relies on
  EXPECT(chunk_route(Knobs{-1, MB64, 6144, true}, 140000, false, true) == Route::SLOTS_KPROD, "140000 pairs under 64 MB: in register, <KPROD>");
  // small routes off (the cap is then 0): neither one-wavefront kernel
  const Knobs off{-1, GB12, 0, false};
  EXPECT(chunk_route(off, 1, false, true) == Route::SLOTS_KMAXW && chunk_route(off, 256, false, true) == Route::SLOTS_KMAXW, "WIDE_TAIL = 0");
  // a moved cap (SYLOW_HIP_OPT_WIDE_MAX) moves the wide batch only
  EXPECT(chunk_route(Knobs{-1, GB12, 100, true}, 101, false, true) == Route::SLOTS_KMAXW && chunk_route(Knobs{-1, GB12, 100, true}, 100, false, true) == Route::WIDE_BATCH, "cap 100");
  // one round exactly fits; one byte less does not (chunks of two: 2 x 19488 x 65536 bytes)
  EXPECT(chunk_route(Knobs{-1, (size_t)2554331136, 6144, true}, 65537, false, true) == Route::TABLES, "one round of two-slot jobs");
  EXPECT(chunk_route(Knobs{-1, (size_t)2554331135, 6144, true}, 65537, false, true) == Route::SLOTS_KMAXW, "one byte below a round");
}

static void groth16() {
  const size_t lim = (size_t)1024 * 19488;                                  // tests/test_gpu_groth16.py: 1024 * TABLE_BYTES_PER_PROOF
  EXPECT(groth16_tables(Knobs{-1, lim, 6144, true}, 1025), "the smallest limit the table route honours");
  EXPECT(!groth16_tables(Knobs{-1, lim - 1, 6144, true}, 1025), "one byte below: composed");
  // n <= 1024 with 4 n <= cap: multi_pairing_batch would take its one-wavefront route, so composed, whatever the budget
  EXPECT(!groth16_tables(Knobs{-1, GB12, 6144, true}, 8) && !groth16_tables(Knobs{-1, GB12, 6144, true}, 1024), "composed below the cap");
  EXPECT(groth16_tables(Knobs{-1, GB12, 4095, true}, 1024) && groth16_tables(Knobs{-1, GB12, 0, false}, 8), "4 n beyond the cap, or no cap");
  EXPECT(groth16_tables(Knobs{-1, GB12, 6144, true}, 2048) && groth16_tables(Knobs{1, GB12, 6144, true}, 2048), "tables");
  EXPECT(!groth16_tables(Knobs{0, GB12, 6144, true}, 2048), "MULTI_TABLES = 0: composed");
  EXPECT(groth16_tables(Knobs{-1, (size_t)8 * 19488, 0, false}, 8) && !groth16_tables(Knobs{-1, (size_t)8 * 19488 - 1, 0, false}, 8), "fewer than 1024 proofs: their own tables");
  EXPECT(!groth16_tables(Knobs{1, lim - 1, 6144, true}, 1025), "mode 1 does not waive the budget here");
}

int main() {
  geometry_and_slices();
  job_grid();
  chunk_grid();
  groth16();
  if (fails) { printf("%d of %zu checks failed\n", fails, checked); return 1; }
  printf("OK %zu checks\n", checked);
  return 0;
}
