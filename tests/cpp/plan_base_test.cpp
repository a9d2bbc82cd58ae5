// CPU-only check of what every plan header counts with (sylow_amd/csrc/plan_base.hpp): the saturating product and sum at the sentinel, on
// both sides of SAT / b and with a zero operand, the carver of a scratch lease (empty, aligned, misaligned, saturated), the elements of a domain, the rule for a pinned grid, the two range tests where they agree
// (touching, overlapping) and where they must not (an empty range inside a non-empty one), and the aliasing table of an entry point on two
// inputs and three outputs.  Expected values are written out by hand.  Built with -fsanitize=address,undefined by tests/test_plan_base.py:
// host code only.
#include "../../sylow_amd/csrc/plan_base.hpp"

#include <cstdint>
#include <cstdio>

using namespace plan_base;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const size_t TOP = SIZE_MAX;

static void saturating() {
  EXPECT(SAT == TOP, "the sentinel is the largest size_t");
  EXPECT(mul_sat(SAT, 1) == SAT && mul_sat(1, SAT) == SAT && mul_sat(SAT, 2) == SAT && mul_sat(2, SAT) == SAT && mul_sat(SAT, SAT) == SAT, "products at SAT");
  // 2^64 - 1 = 7 q + 1 and = 2 h + 1: the last product that fits, then the first that does not, either operand first
  const size_t q = SAT / 7, h = SAT / 2;
  EXPECT(q == 0x2492492492492492ull && mul_sat(q, 7) == SAT - 1 && mul_sat(7, q) == SAT - 1, "SAT / 7 from below: %zx", mul_sat(q, 7));
  EXPECT(mul_sat(q + 1, 7) == SAT && mul_sat(7, q + 1) == SAT, "SAT / 7 from above");
  EXPECT(h == 0x7fffffffffffffffull && mul_sat(h, 2) == SAT - 1 && mul_sat(2, h) == SAT - 1 && mul_sat(h + 1, 2) == SAT && mul_sat(2, h + 1) == SAT, "SAT / 2 on both sides");
  EXPECT(mul_sat((size_t)1 << 32, (size_t)1 << 32) == SAT && mul_sat((size_t)1 << 32, ((size_t)1 << 32) - 1) == 0xffffffff00000000ull, "around 2^64");
  EXPECT(mul_sat(0, SAT) == 0 && mul_sat(SAT, 0) == 0 && mul_sat(0, 0) == 0 && mul_sat(0, 5) == 0 && mul_sat(5, 0) == 0, "a zero operand, and no division by it");
  EXPECT(add_sat(SAT, 0) == SAT && add_sat(0, SAT) == SAT && add_sat(SAT, 1) == SAT && add_sat(1, SAT) == SAT && add_sat(SAT, SAT) == SAT, "sums at SAT");
  EXPECT(add_sat(SAT - 2, 1) == SAT - 1 && add_sat(1, SAT - 2) == SAT - 1 && add_sat(SAT - 1, 1) == SAT && add_sat(SAT - 1, 2) == SAT && add_sat(2, SAT - 1) == SAT,
         "the last sum that fits, the sum that is the sentinel, the first that wraps");
  EXPECT(add_sat(0, 0) == 0 && add_sat(0, 7) == 7 && add_sat(7, 0) == 7 && add_sat(1, 2) == 3, "a zero operand");
}

// the carver of a scratch lease: offsets in bytes, a word region only on a multiple of 8, SAT for good once it is reached
static void carving() {
  Carve none;
  EXPECT(none.at == 0, "an empty lease");
  Carve c;
  EXPECT(c.words(3) == 0 && c.at == 24 && c.words(0) == 24 && c.at == 24 && c.bytes(5) == 24 && c.at == 29 && c.bytes(0) == 29 && c.at == 29, "words, bytes and empty regions: %zu", c.at);
  c.round();
  EXPECT(c.at == 32, "rounded up to a word: %zu", c.at);
  c.round();
  EXPECT(c.at == 32 && c.words(1) == 32 && c.at == 40, "rounding an aligned offset moves nothing, and words may follow: %zu", c.at);
  Carve odd;
  odd.bytes(3);
  EXPECT(odd.words(1) == SAT && odd.at == SAT, "words behind bytes that were not rounded: the whole lease is refused");
  Carve big;
  EXPECT(big.words(SAT) == 0 && big.at == SAT && big.bytes(1) == SAT && big.at == SAT && big.words(1) == SAT && big.at == SAT && big.bytes(0) == SAT && big.at == SAT, "SAT stays");
  big.round();
  EXPECT(big.at == SAT, "through a rounding too");
  Carve edge;
  EXPECT(edge.words(SAT / 8) == 0 && edge.at == SAT - 7, "the last word region that fits: %zx", edge.at);
  edge.round();
  EXPECT(edge.at == SAT - 7 && edge.bytes(7) == SAT - 7 && edge.at == SAT, "SAT - 7 is aligned; 7 bytes more reach the sentinel");
  Carve top;
  top.bytes(SAT - 3);
  top.round();
  EXPECT(top.at == SAT, "a rounding that would wrap saturates");
  Carve sum;
  sum.bytes(SAT - 8);
  EXPECT(sum.bytes(9) == SAT - 8 && sum.at == SAT && words_of(SAT) == SAT && words_of(24) == 3 && words_of(0) == 0 && words_of(SAT - 7) == SAT / 8, "a sum that would wrap; words_of");
}

static void domains_and_pins() {
  EXPECT(elems(0) == 1 && elems(1) == 2 && elems(27) == 134217728 && elems(28) == 268435456, "2^log_n");
  EXPECT(max_blocks_ok(-1) && max_blocks_ok(-9) && max_blocks_ok(1) && max_blocks_ok(4096) && !max_blocks_ok(0), "a cap of no block is refused");
}

static void ranges() {
  // touching: both accept, in either order
  EXPECT(disjoint(0, 8, 8, 8) && disjoint(8, 8, 0, 8) && disjoint_or_empty(0, 8, 8, 8) && disjoint_or_empty(8, 8, 0, 8), "touching ranges share no byte");
  // overlapping by one byte, one inside the other, equal: both refuse
  EXPECT(!disjoint(0, 9, 8, 8) && !disjoint(8, 8, 0, 9) && !disjoint_or_empty(0, 9, 8, 8) && !disjoint_or_empty(8, 8, 0, 9), "one byte shared");
  EXPECT(!disjoint(4, 1, 0, 8) && !disjoint(0, 8, 4, 1) && !disjoint_or_empty(4, 1, 0, 8) && !disjoint_or_empty(0, 8, 4, 1), "a range inside the other");
  EXPECT(!disjoint(1000, 64, 1000, 64) && !disjoint_or_empty(1000, 64, 1000, 64), "the same range");
  // an empty range inside a non-empty one: the strict test refuses it, the other accepts it
  EXPECT(!disjoint(4, 0, 0, 8) && !disjoint(0, 8, 4, 0), "strict: an empty range inside another collides");
  EXPECT(disjoint_or_empty(4, 0, 0, 8) && disjoint_or_empty(0, 8, 4, 0), "an empty range overlaps nothing");
  // an empty range at either end of the other lies outside it for both
  EXPECT(disjoint(0, 0, 0, 8) && disjoint(8, 0, 0, 8) && disjoint(0, 8, 8, 0) && disjoint_or_empty(0, 0, 0, 8) && disjoint_or_empty(8, 0, 0, 8), "an empty range at an end");
  EXPECT(disjoint(4, 0, 4, 0) && disjoint_or_empty(4, 0, 4, 0), "two empty ranges");
}

static void tables() {
  // inputs [100, 164) and [200, 232); outputs of 32, 32 and 1 bytes
  const Range in[2] = {{100, 64}, {200, 32}};
  {
    const Range out[3] = {{300, 32}, {332, 32}, {364, 1}};
    EXPECT(outputs_disjoint(in, out, disjoint) && outputs_disjoint(in, out, disjoint_or_empty), "everything apart, outputs touching");
  }
  {
    const Range out[3] = {{300, 32}, {0, 32}, {364, 1}};                 // NULL: 32 bytes from address 0 touch nothing, and nothing is asked
    EXPECT(outputs_disjoint(in, out, disjoint) && outputs_disjoint(in, out, disjoint_or_empty), "a NULL output takes no part");
    const Range over_null[3] = {{16, 32}, {0, 32}, {364, 1}};            // an output over the bytes a NULL one would span
    EXPECT(outputs_disjoint(in, over_null, disjoint), "not even against an output that lies there");
  }
  {
    const Range out[3] = {{300, 32}, {400, 32}, {331, 1}};               // the first output's last byte is the third output
    EXPECT(!outputs_disjoint(in, out, disjoint) && !outputs_disjoint(in, out, disjoint_or_empty), "an output over a LATER output");
    const Range swapped[3] = {{331, 1}, {400, 32}, {300, 32}};
    EXPECT(!outputs_disjoint(in, swapped, disjoint) && !outputs_disjoint(in, swapped, disjoint_or_empty), "and the same pair in the other order");
    const Range last_two[3] = {{300, 32}, {400, 32}, {431, 1}};
    EXPECT(!outputs_disjoint(in, last_two, disjoint), "the last two outputs");
  }
  {
    const Range out[3] = {{300, 32}, {332, 32}, {231, 1}};               // the last byte of the second input
    EXPECT(!outputs_disjoint(in, out, disjoint) && !outputs_disjoint(in, out, disjoint_or_empty), "an output over an input");
    const Range first[3] = {{163, 32}, {332, 32}, {364, 1}};             // the last byte of the first input
    EXPECT(!outputs_disjoint(in, first, disjoint) && !outputs_disjoint(in, first, disjoint_or_empty), "the first output over the first input");
    const Range null_in[2] = {{100, 64}, {0, 32}};                       // a NULL input is not compared either
    const Range low[3] = {{16, 8}, {332, 32}, {364, 1}};
    EXPECT(outputs_disjoint(null_in, low, disjoint), "a NULL input takes no part");
  }
  {
    const Range out[3] = {{300, 32}, {120, 0}, {364, 1}};                // an empty output inside the first input: the test the caller names decides
    EXPECT(!outputs_disjoint(in, out, disjoint) && outputs_disjoint(in, out, disjoint_or_empty), "the table asks the range test it is given");
    const Range empty_in[2] = {{310, 0}, {200, 32}};                     // an empty input inside the first output
    const Range plain[3] = {{300, 32}, {332, 32}, {364, 1}};
    EXPECT(!outputs_disjoint(empty_in, plain, disjoint) && outputs_disjoint(empty_in, plain, disjoint_or_empty), "for inputs too");
  }
  {
    const Range one_in[1] = {{100, 64}}, one_out[1] = {{164, 8}};
    EXPECT(outputs_disjoint(one_in, one_out, disjoint) && outputs_disjoint(in, one_out, disjoint), "tables of any length");
  }
}

int main() {
  saturating();
  carving();
  domains_and_pins();
  ranges();
  tables();
  if (fails) {
    printf("%d of %zu checks failed\n", fails, checked);
    return 1;
  }
  printf("OK %zu checks\n", checked);
  return 0;
}
