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
#include "layout_check.hpp"

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

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // W = 3, E = 4: 18 terms; 3 public inputs; ONE proof: 22 flag bytes, padded to 24
    const FoldLayout l = fold_layout(2, 3, 3, 1);
    const Region r[] = {WORDS(l, den, 24), WORDS(l, k, 72), WORDS(l, bases, 144), WORDS(l, pbases, 16), WORDS(l, psc, 8), WORDS(l, C, 8), WORDS(l, PI, 8), BYTES(l, binf, 18),
                        BYTES(l, pbinf, 2), BYTES(l, cinf, 1), BYTES(l, pinf, 1)};
    EXPECT(layout_ok("fold", r, l.bytes) && l.k == 192 && l.bases == 768 && l.pbases == 1920 && l.psc == 2048 && l.C == 2112 && l.PI == 2176 && l.binf == 2240 && l.pbinf == 2258 &&
               l.cinf == 2260 && l.pinf == 2261 && l.bytes == 2264, "one proof: %zu", l.bytes);
  }
  {
    const FoldLayout l = fold_layout(2, 3, 3, 2);
    const Region r[] = {WORDS(l, den, 48), WORDS(l, k, 144), WORDS(l, bases, 288), WORDS(l, pbases, 32), WORDS(l, psc, 16), WORDS(l, C, 16), WORDS(l, PI, 16), BYTES(l, binf, 36),
                        BYTES(l, pbinf, 4), BYTES(l, cinf, 2), BYTES(l, pinf, 2)};
    EXPECT(layout_ok("fold 2", r, l.bytes) && l.k == 384 && l.bases == 1536 && l.pbases == 3840 && l.C == 4224 && l.binf == 4480 && l.cinf == 4520 && l.pinf == 4522 && l.bytes == 4528,
           "two proofs: %zu", l.bytes);
  }
  {  // no public inputs: no denominators
    const FoldLayout l = fold_layout(2, 3, 0, 1);
    const Region r[] = {WORDS(l, den, 0), WORDS(l, k, 72), WORDS(l, bases, 144), WORDS(l, pbases, 16), WORDS(l, psc, 8), WORDS(l, C, 8), WORDS(l, PI, 8), BYTES(l, binf, 18),
                        BYTES(l, pbinf, 2), BYTES(l, cinf, 1), BYTES(l, pinf, 1)};
    EXPECT(layout_ok("fold, n_pub = 0", r, l.bytes) && l.k == 0 && l.bases == 576 && l.binf == 2048 && l.pinf == 2069 && l.bytes == 2072, "no public inputs: %zu", l.bytes);
    EXPECT(fold_layout(2, 3, 3, SIZE_MAX / 8).bytes == SIZE_MAX && scalars_scratch_bytes(3, 2) == 384 && scalars_scratch_bytes(SIZE_MAX / 4, 2) == SIZE_MAX, "saturate");
  }
  {
    const VerifyLayout l = verify_layout(9);
    const Region r[] = {WORDS(l, C, 72), WORDS(l, PI, 72), WORDS(l, y, 36), WORDS(l, z, 36), BYTES(l, cinf, 9), BYTES(l, pinf, 9)};
    EXPECT(layout_ok("verify", r, l.bytes) && l.PI == 576 && l.y == 1152 && l.z == 1440 && l.cinf == 1728 && l.pinf == 1737 && l.bytes == 1752, "9 proofs: %zu", l.bytes);
    const VerifyLayout o = verify_layout(1);
    const Region q[] = {WORDS(o, C, 8), WORDS(o, PI, 8), WORDS(o, y, 4), WORDS(o, z, 4), BYTES(o, cinf, 1), BYTES(o, pinf, 1)};
    EXPECT(layout_ok("verify of one", q, o.bytes) && o.y == 128 && o.z == 160 && o.cinf == 192 && o.pinf == 193 && o.bytes == 200 && verify_layout(SIZE_MAX / 8).bytes == SIZE_MAX,
           "one proof: %zu", o.bytes);
  }
  {  // the weighted form, 2 proofs: K = 8 key points, P = 10 own, 10 columns in one part; 13 flag bytes, padded to 16
    const WeightedLayout l = weighted_layout(2, 3, 3, 2);
    const Region r[] = {WORDS(l, den, 48), WORDS(l, k, 144), WORDS(l, y, 8), WORDS(l, sc_own, 80), WORDS(l, sc_open, 16), WORDS(l, obases, 32), WORDS(l, partial, 40),
                        WORDS(l, ksum, 32), WORDS(l, s, 4), WORDS(l, bad, 4), WORDS(l, m_own, 8), WORDS(l, m2, 8), WORDS(l, m_key, 8), WORDS(l, m1, 8), WORDS(l, sg, 8),
                        WORDS(l, pxy, 16), WORDS(l, qxy, 32), BYTES(l, obinf, 4), BYTES(l, f_own, 1), BYTES(l, f2, 1), BYTES(l, f_key, 1), BYTES(l, f1, 1), BYTES(l, fsg, 1),
                        BYTES(l, pinf, 2), BYTES(l, qinf, 2)};
    EXPECT(layout_ok("weighted", r, l.bytes) && l.k == 384 && l.y == 1536 && l.sc_own == 1600 && l.sc_open == 2240 && l.obases == 2368 && l.partial == 2624 && l.ksum == 2944 &&
               l.s == 3200 && l.bad == 3232 && l.m_own == 3264, "weighted: %zu", l.m_own);
    EXPECT(l.m2 == 3328 && l.m_key == 3392 && l.m1 == 3456 && l.sg == 3520 && l.pxy == 3584 && l.qxy == 3712 && l.obinf == 3968 && l.f_own == 3972 && l.f2 == 3973 &&
               l.f_key == 3974 && l.f1 == 3975 && l.fsg == 3976 && l.pinf == 3977 && l.qinf == 3979 && l.bytes == 3984, "weighted: %zu", l.bytes);
  }
  {  // one proof without public inputs
    const WeightedLayout l = weighted_layout(2, 3, 0, 1);
    const Region r[] = {WORDS(l, den, 0), WORDS(l, k, 72), WORDS(l, y, 4), WORDS(l, sc_own, 40), WORDS(l, sc_open, 8), WORDS(l, obases, 16), WORDS(l, partial, 40),
                        WORDS(l, ksum, 32), WORDS(l, s, 4), WORDS(l, bad, 4), WORDS(l, m_own, 8), WORDS(l, m2, 8), WORDS(l, m_key, 8), WORDS(l, m1, 8), WORDS(l, sg, 8),
                        WORDS(l, pxy, 16), WORDS(l, qxy, 32), BYTES(l, obinf, 2), BYTES(l, f_own, 1), BYTES(l, f2, 1), BYTES(l, f_key, 1), BYTES(l, f1, 1), BYTES(l, fsg, 1),
                        BYTES(l, pinf, 2), BYTES(l, qinf, 2)};
    EXPECT(layout_ok("weighted of one", r, l.bytes) && l.k == 0 && l.y == 576 && l.sc_own == 608 && l.partial == 1120 && l.ksum == 1440 && l.m_own == 1760 && l.pxy == 2080 &&
               l.qxy == 2208 && l.obinf == 2464 && l.f_own == 2466 && l.pinf == 2471 && l.qinf == 2473 && l.bytes == 2480, "one proof: %zu", l.bytes);
    EXPECT(weighted_layout(2, 3, 3, SIZE_MAX / 8).bytes == SIZE_MAX, "saturates");
  }
}

int main() {
  constants_and_pins();
  terms_and_offsets();
  scratch_sums();
  chunks();
  layouts();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
