// CPU-only check of the planner of the batched PLONK verifier (sylow_amd/csrc/plonk_verify_plan.hpp).  Every expected value is written out by
// hand from the rules in the header's comments (2 W + 2 key points and W + E + 3 proof points; T = 3 W + E + 5 terms, the key's first; the
// denominators and their inverses, 8 words a public input and proof; a chunk of the fold leases the denominators, 4 + 8 words a term, 40
// words a proof for pi's terms and the two results, and a flag byte per term and four per proof; the weighted form's columns are the key's,
// then s, then the count).  Built with -fsanitize=address,undefined by tests/test_plonk_verify_plan.py: host code only.
#include "../../sylow_amd/csrc/plonk_verify_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <set>

using namespace plonk_verify_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void constants_and_pins() {
  EXPECT(PV_BLOCK == 256 && FR_WORDS == 4 && G1_WORDS == 8 && G2_WORDS == 16 && PI_TERMS == 2 && STATUS_ZETA_IN_DOMAIN == 2 && WEIGHTED_POINTS == 5, "constants");
  EXPECT(dims_ok(0, 0, 2) && dims_ok(26, 2, 32) && dims_ok(0, 28, 3) && !dims_ok(27, 2, 3) && !dims_ok(-1, 2, 3) && !dims_ok(3, -1, 3) && !dims_ok(3, 2, 1) &&
             !dims_ok(3, 2, 33),
         "the dimensions are the prover's");
  EXPECT(pub_ok(3, 0) && pub_ok(3, 8) && !pub_ok(3, 9) && pub_ok(0, 1) && !pub_ok(0, 2), "0 <= n_pub <= n");
  EXPECT(!max_blocks_ok(0) && max_blocks_ok(-1) && max_blocks_ok(1), "max_blocks");
  EXPECT(tau_bytes() == 128 && gt_bytes() == 384 && points_bytes(2) == 128 && points_bytes(SIZE_MAX / 8) == SIZE_MAX, "bytes");
}

static void terms_and_offsets() {
  EXPECT(key_points(2) == 6 && key_points(3) == 8 && key_points(32) == 66, "2 W + 2");
  EXPECT(proof_points(2, 3) == 10 && proof_points(0, 2) == 6 && proof_points(5, 32) == 67, "W + E + 3");
  EXPECT(terms(2, 3) == 18 && terms(0, 2) == 12 && terms(0, 3) == 15 && terms(2, 32) == 105 && terms(5, 17) == 88, "T = 3 W + E + 5");
  // W = 3, E = 4, in the header's order
  EXPECT(term_selector(0) == 0 && term_selector(2) == 2 && term_qm(3) == 3 && term_qc(3) == 4 && term_sigma(3, 0) == 5 && term_sigma(3, 1) == 6 && term_sigma(3, 2) == 7, "the key");
  EXPECT(term_wire(3, 0) == 8 && term_wire(3, 2) == 10 && term_z(3) == 11 && term_chunk(3, 0) == 12 && term_chunk(3, 3) == 15 && term_wzeta(2, 3) == 16 &&
             term_womega(2, 3) == 17,
         "the proof");
  EXPECT(pslot_wire(2) == 2 && pslot_z(3) == 3 && pslot_chunk(3, 0) == 4 && pslot_chunk(3, 3) == 7 && pslot_wzeta(2, 3) == 8 && pslot_womega(2, 3) == 9, "the slots of a proof");
  EXPECT(pslot_wzeta(0, 2) == 4 && pslot_womega(0, 2) == 5 && term_womega(0, 2) == 11, "E = 1");
  // every term once, for several shapes
  for (const int W : {2, 3, 17, 32})
    for (const int log_e : {0, 2, 5}) {
      std::set<size_t> seen;
      for (int j = 0; j < W; ++j) { seen.insert(term_selector(j)); seen.insert(term_sigma(W, j)); seen.insert(term_wire(W, j)); }
      seen.insert(term_qm(W)); seen.insert(term_qc(W)); seen.insert(term_z(W)); seen.insert(term_wzeta(log_e, W)); seen.insert(term_womega(log_e, W));
      for (size_t e = 0; e < elems(log_e); ++e) seen.insert(term_chunk(W, e));
      EXPECT(seen.size() == terms(log_e, W) && *seen.rbegin() == terms(log_e, W) - 1 && term_own(W, 0) == key_points(W), "W = %d, log_e = %d", W, log_e);
    }
  EXPECT(key_bytes(3) == 512 && proof_count(2, 3, 2) == 20 && proof_bytes(2, 3, 2) == 1280 && term_count(2, 3, 2) == 36 && pub_count(3, 2) == 6, "W = 3, E = 4, m = 2");
  EXPECT(proof_bytes(2, 3, SIZE_MAX / 16) == SIZE_MAX && term_count(2, 3, SIZE_MAX / 4) == SIZE_MAX && pub_count(SIZE_MAX / 2, 3) == SIZE_MAX, "saturate");
}

static void scratch_sums() {
  EXPECT(den_words(3, 2) == 48 && den_words(0, 5) == 0 && scalars_scratch_words(8, 1) == 64 && den_words(SIZE_MAX / 4, 2) == SIZE_MAX, "the denominators and their inverses");
  EXPECT(flag_words(0) == 0 && flag_words(1) == 1 && flag_words(8) == 1 && flag_words(9) == 2, "flags round up to words");
  // W = 3, E = 4, n_pub = 3: 24 + 12 * 18 + 40 + ceil(22 / 8) words a proof
  EXPECT(fold_flags(2, 3, 1) == 22 && fold_chunk_words(2, 3, 3, 1) == 24 + 216 + 40 + 3 && fold_chunk_bytes(2, 3, 3, 1) == 2264, "one proof: %zu", fold_chunk_bytes(2, 3, 3, 1));
  EXPECT(fold_chunk_words(2, 3, 3, 2) == 48 + 432 + 80 + 6 && fold_chunk_bytes(2, 3, 3, 2) == 4528, "two proofs: %zu", fold_chunk_bytes(2, 3, 3, 2));
  EXPECT(fold_chunk_words(2, 3, 0, 1) == 216 + 40 + 3, "no public inputs");
  EXPECT(fold_chunk_words(2, 3, 3, SIZE_MAX / 8) == SIZE_MAX && fold_chunk_bytes(2, 3, 3, SIZE_MAX / 8) == SIZE_MAX && fold_chunk_bytes(2, 3, SIZE_MAX / 2, 1) == SIZE_MAX &&
             fold_chunk_bytes(2, 3, 3, SIZE_MAX / 2200) == SIZE_MAX,
         "saturates at the top");
  EXPECT(verify_words(2) == 48 + 1 && verify_words(9) == 216 + 3 && verify_words(SIZE_MAX / 8) == SIZE_MAX, "C, pi, y, zeros and two flag arrays");
  EXPECT(weighted_columns(3) == 10 && column_s(3) == 8 && column_bad(3) == 9 && weighted_parts(1) == 1 && weighted_parts(256) == 1 && weighted_parts(257) == 2, "columns and parts");
  EXPECT(weighted_words(2, 3, 3, 2) == 48 + 152 + 80 + 48 + 80 + 88 + 2, "m = 2: %zu", weighted_words(2, 3, 3, 2));
  EXPECT(weighted_words(2, 3, 3, SIZE_MAX / 8) == SIZE_MAX && !scratch_ok(SIZE_MAX) && scratch_ok(1000), "saturates, and is refused");
}

static void chunks() {
  EXPECT(proofs_per_chunk(2, 3, 3, 5, 2263) == 0, "below one proof: refused");
  EXPECT(proofs_per_chunk(2, 3, 3, 5, 2264) == 1 && proofs_per_chunk(2, 3, 3, 5, 4527) == 1 && proofs_per_chunk(2, 3, 3, 5, 4528) == 2, "holds one, then two");
  EXPECT(proofs_per_chunk(2, 3, 3, 5, (size_t)1 << 30) == 5 && proofs_per_chunk(2, 3, 3, 0, (size_t)1 << 30) == 0 && proofs_per_chunk(2, 3, 3, 1, 2264) == 1, "m caps it");
  // the flags' rounding: whatever the budget, the chunk fits and one more proof does not
  for (size_t budget = 2264; budget < 40000; budget += 97) {
    const size_t mc = proofs_per_chunk(2, 3, 3, 1000, budget);
    EXPECT(mc >= 1 && fold_chunk_bytes(2, 3, 3, mc) <= budget && fold_chunk_bytes(2, 3, 3, mc + 1) > budget, "budget %zu: %zu", budget, mc);
  }
  EXPECT(chunk_count(5, 2) == 3 && chunk_size(5, 2, 4) == 1 && chunk_size(5, 2, 2) == 2 && chunk_count(5, 0) == 0, "whole proofs");
  EXPECT(proofs_per_chunk(2, 3, SIZE_MAX / 2, 4, (size_t)1 << 30) == 0, "a size that saturates is refused");
}

int main() {
  constants_and_pins();
  terms_and_offsets();
  scratch_sums();
  chunks();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
