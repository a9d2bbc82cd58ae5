// CPU-only check of the planner of the two weighted checks that lease one block each (sylow_amd/csrc/weighted_plan.hpp): the parts of
// their Fr sums and the layout of the lease.  Every offset and total below is the chain of pointers the launch code of kzg.hip and
// groth16.hip walked before the layouts, written out by hand:
//   KZG      u64 words  4n | 8n | 16n | 4 parts | 4 | 8 | 8 | 8 | 16 | 32      then bytes  2n | 1 | 1 | 1 | 2 | 2,     parts = ceil(n / 256)
//   Groth16  u64 words  4n | 8n | 8nb | 4nb | 8nb | 8 | 8m | 16m | 4 cols parts  then bytes  n | nb | 1 | m | m,
//            cols = n_inputs + 1, nb = cols + 1, m = n + 3, parts = min(ceil(n / 2048), 256)
// Nothing on the expected side is computed from the header.  Built with -fsanitize=address,undefined by tests/test_weighted_plan.py: host
// code only.
#include "../../sylow_amd/csrc/weighted_plan.hpp"

#include <cstdint>
#include <cstdio>

using namespace weighted_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static void parts() {
  EXPECT(WEIGHTED_BLOCK == 256 && FR_ROWS_PER_LANE == 8 && FR_PARTS_MAX == 256, "constants");
  const size_t kzg[][2] = {{1, 1}, {256, 1}, {257, 2}, {65537, 257}, {SIZE_MAX, (size_t)1 << 56}};
  for (const auto& k : kzg) EXPECT(kzg_parts(k[0]) == k[1], "kzg_parts(%zu) = %zu", k[0], kzg_parts(k[0]));
  // 2048 rows to a part; one part becomes two at 2049; 524288 rows fill the 256 parts and one more row meets the cap
  const size_t g16[][2] = {{1, 1}, {5, 1}, {2048, 1}, {2049, 2}, {4096, 2}, {4097, 3}, {524288, 256}, {524289, 256}, {(size_t)1 << 40, 256}, {SIZE_MAX, 256}};
  for (const auto& g : g16) EXPECT(groth16_parts(g[0]) == g[1], "groth16_parts(%zu) = %zu", g[0], groth16_parts(g[0]));
  EXPECT(groth16_columns(0) == 1 && groth16_columns(3) == 4 && groth16_bases(0) == 2 && groth16_bases(3) == 5 && groth16_pairs(1) == 4 && groth16_pairs(2049) == 2052, "counts");
}

// one KZG case: the sizes of the regions from n and parts, the offsets as given
struct KzgCase { size_t n, parts, sc, bases, partial, s, m1, m2, sg, pxy, qxy, binf, m1inf, m2inf, sginf, pinf, qinf, bytes; };
static void kzg_layouts() {
  const KzgCase cases[] = {
      {1, 1, 32, 96, 224, 256, 288, 352, 416, 480, 608, 864, 866, 867, 868, 869, 871, 873},
      {256, 1, 8192, 24576, 57344, 57376, 57408, 57472, 57536, 57600, 57728, 57984, 58496, 58497, 58498, 58499, 58501, 58503},
      {257, 2, 8224, 24672, 57568, 57632, 57664, 57728, 57792, 57856, 57984, 58240, 58754, 58755, 58756, 58757, 58759, 58761},
      {65537, 257, 2097184, 6291552, 14680288, 14688512, 14688544, 14688608, 14688672, 14688736, 14688864, 14689120, 14820194, 14820195, 14820196, 14820197, 14820199,
       14820201},
  };
  for (const KzgCase& c : cases) {
    const KzgWeightedLayout l = kzg_weighted_layout(c.n);
    const Region r[] = {WORDS(l, wr, 4 * c.n), WORDS(l, sc, 8 * c.n), WORDS(l, bases, 16 * c.n), WORDS(l, partial, 4 * c.parts), WORDS(l, s, 4), WORDS(l, m1, 8),
                        WORDS(l, m2, 8), WORDS(l, sg, 8), WORDS(l, pxy, 16), WORDS(l, qxy, 32), BYTES(l, binf, 2 * c.n), BYTES(l, m1inf, 1), BYTES(l, m2inf, 1),
                        BYTES(l, sginf, 1), BYTES(l, pinf, 2), BYTES(l, qinf, 2)};
    EXPECT(layout_ok("kzg weighted", r, l.bytes), "n = %zu", c.n);
    EXPECT(l.wr == 0 && l.sc == c.sc && l.bases == c.bases && l.partial == c.partial && l.s == c.s && l.m1 == c.m1 && l.m2 == c.m2 && l.sg == c.sg && l.pxy == c.pxy &&
               l.qxy == c.qxy, "the words of n = %zu", c.n);
    EXPECT(l.binf == c.binf && l.m1inf == c.m1inf && l.m2inf == c.m2inf && l.sginf == c.sginf && l.pinf == c.pinf && l.qinf == c.qinf, "the flags of n = %zu", c.n);
    EXPECT(l.bytes == c.bytes && l.bytes == (28 * c.n + 4 * c.parts + 76) * 8 + 2 * c.n + 7 && l.qinf + 2 == l.bytes, "n = %zu: %zu bytes", c.n, l.bytes);
  }
  // the sum the entry point formed in size_t wrapped from here on; the layout saturates and the entry point refuses it
  EXPECT(kzg_weighted_layout(SIZE_MAX / 128).bytes == SIZE_MAX && kzg_weighted_layout(SIZE_MAX / 226).bytes == SIZE_MAX && kzg_weighted_layout(SIZE_MAX).bytes == SIZE_MAX,
         "saturates");
  EXPECT(kzg_weighted_layout((size_t)1 << 40).bytes != SIZE_MAX, "2^40 openings fit size_t");
}

struct Groth16Case { size_t n, n_inputs, parts, ra, bases, sums, prod, sc, pxy, qxy, partial, ra_inf, prod_inf, sc_inf, pinf, qinf, bytes; };
static void groth16_layouts() {
  const Groth16Case cases[] = {
      {1, 0, 1, 32, 96, 224, 288, 416, 480, 736, 1248, 1280, 1281, 1283, 1284, 1288, 1292},
      {5, 3, 1, 160, 480, 800, 960, 1280, 1344, 1856, 2880, 3008, 3013, 3018, 3019, 3027, 3035},
      {2048, 3, 1, 65536, 196608, 196928, 197088, 197408, 197472, 328736, 591264, 591392, 593440, 593445, 593446, 595497, 597548},
      {2049, 3, 2, 65568, 196704, 197024, 197184, 197504, 197568, 328896, 591552, 591808, 593857, 593862, 593863, 595915, 597967},
      {524289, 1, 256, 16777248, 50331744, 50331936, 50332032, 50332224, 50332288, 83886976, 150996352, 151012736, 151537025, 151537028, 151537029, 152061321, 152585613},
  };
  for (const Groth16Case& c : cases) {
    const size_t cols = c.n_inputs + 1, nb = c.n_inputs + 2, m = c.n + 3;
    const Groth16WeightedLayout l = groth16_weighted_layout(c.n, c.n_inputs);
    const Region r[] = {WORDS(l, wr, 4 * c.n), WORDS(l, ra, 8 * c.n), WORDS(l, bases, 8 * nb), WORDS(l, sums, 4 * nb), WORDS(l, prod, 8 * nb), WORDS(l, sc, 8),
                        WORDS(l, pxy, 8 * m), WORDS(l, qxy, 16 * m), WORDS(l, partial, 4 * cols * c.parts), BYTES(l, ra_inf, c.n), BYTES(l, prod_inf, nb),
                        BYTES(l, sc_inf, 1), BYTES(l, pinf, m), BYTES(l, qinf, m)};
    EXPECT(layout_ok("groth16 weighted", r, l.bytes), "n = %zu, %zu inputs", c.n, c.n_inputs);
    EXPECT(l.wr == 0 && l.ra == c.ra && l.bases == c.bases && l.sums == c.sums && l.prod == c.prod && l.sc == c.sc && l.pxy == c.pxy && l.qxy == c.qxy &&
               l.partial == c.partial, "the words of n = %zu, %zu inputs", c.n, c.n_inputs);
    EXPECT(l.ra_inf == c.ra_inf && l.prod_inf == c.prod_inf && l.sc_inf == c.sc_inf && l.pinf == c.pinf && l.qinf == c.qinf, "the flags of n = %zu, %zu inputs", c.n,
           c.n_inputs);
    EXPECT(l.bytes == c.bytes && l.bytes == (12 * c.n + 20 * nb + 8 + 24 * m + 4 * cols * c.parts) * 8 + c.n + nb + 1 + 2 * m && l.qinf + m == l.bytes,
           "n = %zu, %zu inputs: %zu bytes", c.n, c.n_inputs, l.bytes);
  }
  EXPECT(groth16_weighted_layout(SIZE_MAX / 128, 1).bytes == SIZE_MAX && groth16_weighted_layout(1, SIZE_MAX / 64).bytes == SIZE_MAX &&
             groth16_weighted_layout(SIZE_MAX, 0).bytes == SIZE_MAX && groth16_weighted_layout(1, SIZE_MAX).bytes == SIZE_MAX &&
             groth16_weighted_layout(SIZE_MAX - 2, 0).bytes == SIZE_MAX, "saturates");
  EXPECT(groth16_weighted_layout((size_t)1 << 40, (size_t)1 << 20).bytes != SIZE_MAX, "2^40 proofs of 2^20 inputs fit size_t");
}

int main() {
  parts();
  kzg_layouts();
  groth16_layouts();
  if (fails) { printf("%d of %zu checks failed\n", fails, checked); return 1; }
  printf("OK %zu checks\n", checked);
  return 0;
}
