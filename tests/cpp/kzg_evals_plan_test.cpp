// CPU-only check of the planner of the evaluation-form KZG unit (sylow_amd/csrc/kzg_evals_plan.hpp) and of the lone-lane inversion it
// prices (sylow_amd/csrc/bn254_fr_euclid.hpp).  Every expected value of the geometry is written out by hand from the rules in the header's
// comments (a lane owns 8 elements, a block 256 lanes, no level above the chunk, 29 root slots of 4 words); the inverses are Python's
// pow(a, -1, r), pasted.  Built with -fsanitize=address,undefined by tests/test_kzg_evals_plan.py: host code only.
#include "../../sylow_amd/csrc/bn254_fr_euclid.hpp"
#include "../../sylow_amd/csrc/kzg_evals_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>

using namespace kzg_evals_plan;
static int fails = 0;
static size_t checked = 0;
#define EXPECT(cond, ...) do { ++checked; if (!(cond)) { ++fails; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)
#include "layout_check.hpp"

static void chunk_geometry() {
  EXPECT(EVALS_BLOCK == 256 && EVALS_LANE_ELEMS == 8 && EVALS_CHUNK == 2048 && EVALS_LOG_N_MAX == 28, "constants");
  const size_t ch[][2] = {{0, 0}, {1, 1}, {7, 1}, {8, 1}, {9, 1}, {2047, 1}, {2048, 1}, {2049, 2}, {4096, 2}, {4097, 3}, {6153, 4}, {524289, 257},
                          {1u << 20, 512}, {(1u << 20) + 1, 513}};
  for (const auto& c : ch) EXPECT(chunks(c[0]) == c[1], "chunks(%zu) = %zu", c[0], chunks(c[0]));
  EXPECT(grid(10) == 10 && grid(1048576) == 1048576 && grid(1048577) == 1048576 && grid(0) == 0, "grid");
  // live lanes: a full chunk has 256; a tail of k elements has ceil(k / 8)
  struct Live { size_t n, c; int live; };
  const Live lv[] = {{1, 0, 1}, {7, 0, 1}, {8, 0, 1}, {9, 0, 2}, {16, 0, 2}, {17, 0, 3}, {256, 0, 32}, {2047, 0, 256}, {2048, 0, 256}, {2049, 0, 256}, {2049, 1, 1},
                     {4096, 1, 256}, {6153, 2, 256}, {6153, 3, 2}, {(size_t)1 << 33, 4194303, 256}, {((size_t)1 << 33) + 2040, 4194304, 255}};
  for (const Live& l : lv) EXPECT(live_lanes(l.n, l.c) == l.live, "live_lanes(%zu, %zu) = %d", l.n, l.c, live_lanes(l.n, l.c));
  // a scan over `live` lanes doubles until it spans them
  const int st[][2] = {{1, 0}, {2, 1}, {3, 2}, {4, 2}, {5, 3}, {32, 5}, {33, 6}, {255, 8}, {256, 8}};
  for (const auto& s : st) EXPECT(scan_steps(s[0]) == s[1], "scan_steps(%d) = %d", s[0], scan_steps(s[0]));
  // byte ranges of equal length: touching ends do not overlap, one shared byte does, an empty range never
  EXPECT(!overlaps(1000, 1032, 32) && !overlaps(1032, 1000, 32) && overlaps(1000, 1031, 32) && overlaps(1031, 1000, 32) && overlaps(1000, 1000, 32), "overlaps");
  EXPECT(!overlaps(1000, 1000, 0), "an empty range");
}

static void batch_inv_plan() {
  // a block per chunk up to the cap: there is no level above the chunk
  EXPECT(batch_inv_grid(1) == 1 && batch_inv_grid(2048) == 1 && batch_inv_grid(2049) == 2 && batch_inv_grid(524289) == 257, "grid");
  EXPECT(batch_inv_grid((size_t)1 << 31) == 1048576 && batch_inv_grid(((size_t)1 << 31) + 1) == 1048576 && batch_inv_grid((size_t)1 << 33) == 1048576, "the cap: 2^20 blocks");
  EXPECT(fr_array_bytes(1) == 32 && fr_array_bytes(2049) == 65568 && fr_array_bytes((size_t)1 << 33) == ((size_t)1 << 38), "bytes");
  EXPECT(fr_array_bytes(SIZE_MAX / 16) == SIZE_MAX && fr_array_bytes(SIZE_MAX) == SIZE_MAX, "saturates");
}

static void quotient_plan() {
  EXPECT(elems(0) == 1 && elems(11) == 2048 && elems(28) == 268435456, "elems");
  const size_t pc[][2] = {{0, 1}, {3, 1}, {10, 1}, {11, 1}, {12, 2}, {13, 4}, {14, 8}, {20, 512}, {28, 131072}};
  for (const auto& c : pc) EXPECT(poly_chunks((int)c[0]) == c[1], "poly_chunks(%zu) = %zu", c[0], poly_chunks((int)c[0]));
  EXPECT(items(8, 4096) == 4096 && items(14, 64) == 512 && items(20, 1) == 512 && items(12, 5) == 10 && items(20, 0) == 0, "items");
  EXPECT(items(13, (size_t)1 << 20) == 4194304 && grid(items(13, (size_t)1 << 20)) == 1048576, "2^13 x 2^20: nothing wraps at 32 bits");
  EXPECT(ROOT_SLOTS == 29 && roots_words() == 116, "roots");
  // 116 words of roots + 4 per item + 1 per polynomial, + 4 per polynomial when the caller takes no y
  EXPECT(quotient_scratch_words(0, 1, true) == 116 + 4 + 1 && quotient_scratch_words(0, 1, false) == 116 + 4 + 1 + 4, "scratch (1, 2^0)");
  EXPECT(quotient_scratch_words(14, 64, true) == 116 + 2048 + 64 && quotient_scratch_words(14, 64, false) == 116 + 2048 + 64 + 256, "scratch (64, 2^14)");
  EXPECT(quotient_scratch_words(20, 1, true) == 116 + 2048 + 1 && quotient_scratch_words(8, 4096, true) == 116 + 16384 + 4096, "scratch (1, 2^20), (4096, 2^8)");
  EXPECT(batch_words(12, 5) == 81920 && batch_words(20, 1) == 4194304 && batch_words(28, (size_t)1 << 40) == SIZE_MAX, "batch words");
  EXPECT(open_scratch_words(12, 5) == 81920 && open_scratch_words(6, 3) == 768, "the opening's buffer");
  EXPECT(NO_HIT == 0xffffffffffffffffull, "NO_HIT is no index of a domain");
}

struct Pair { uint32_t a[8], inv[8]; };
static const Pair KNOWN[] = {
    {{0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
     {0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}},
    {{0x00000002u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
     {0xf8000001u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u}},
    {{0x00000003u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
     {0xa0000001u, 0x2d414e62u, 0xfbd0f5b6u, 0x70229adau, 0x0100e593u, 0xd03583cfu, 0x40cbc01bu, 0x2042def7u}},
    {{0xf0000000u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u},      // r - 1
     {0xf0000000u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}},
    {{0xefffffffu, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u},      // r - 2
     {0xf8000000u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u}},
    {{0xf8000001u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u},      // (r + 1) / 2
     {0x00000002u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}},
    {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x20000000u},      // 2^253: 253 halvings first
     {0x9d88ca6du, 0x17371f6fu, 0x9b63128bu, 0xcfdbf475u, 0xf13ee1d0u, 0x183f9e01u, 0x7295c869u, 0x1e32df33u}},
    {{0x725b19f0u, 0x9bd61b6eu, 0x41112ed4u, 0x402d111eu, 0x8ef62abcu, 0x00e0a7ebu, 0xa58a7e85u, 0x2a3c09f0u},      // the 2^28-th root
     {0x9d18157eu, 0x72394277u, 0xfd399d5du, 0xec9d51f8u, 0x49d5387fu, 0x6117635du, 0x9c229cd5u, 0x01b77519u}},
    {{0x00000005u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
     {0xc6666667u, 0xe7f3fbd4u, 0xca4a2d06u, 0xa9ae5ce9u, 0x33cd568bu, 0x49b9b57cu, 0x5a13d9aau, 0x135b5294u}},
    {{0x892f902cu, 0x1818e811u, 0x5d9dc9f8u, 0x9531985du, 0x0ed90475u, 0xe8e25d94u, 0x81e74ef5u, 0x0dbd9d73u},
     {0x5ebc859au, 0x4cf227c8u, 0x14ffc188u, 0xd0b58e6au, 0x2f8aef3cu, 0xd8a2e2b5u, 0x8c767823u, 0x04e3fa32u}},
    {{0x099950d9u, 0x1600a35au, 0x6f03675au, 0x6b0d549bu, 0x11e20b8fu, 0x3d9c1724u, 0x1738f7d9u, 0x23445bb3u},
     {0xb4afbf8cu, 0xfdf0e041u, 0x561530e6u, 0x25dc2a19u, 0x69ce2bb9u, 0x1acb74deu, 0xcd94c28cu, 0x27da8c83u}},
    {{0x6cad4a27u, 0x0f21ddb6u, 0xd3ac94afu, 0x90c192cfu, 0x1fb17c23u, 0xf28c105du, 0x39263059u, 0x285c2cceu},
     {0x5432e3f4u, 0x3cf4f5eeu, 0x71905893u, 0xc2da94edu, 0x231f298au, 0xfde764fcu, 0xe707c041u, 0x18e92d04u}},
};

static void lone_inversion() {
  EXPECT(fr_euclid::MAX_STEPS == 1016, "2 * (254 + 254) steps");
  for (const Pair& k : KNOWN) {
    uint32_t o[8];
    fr_euclid::inverse(k.a, o);
    EXPECT(memcmp(o, k.inv, sizeof(o)) == 0, "inverse of %08x...%08x", k.a[7], k.a[0]);
    fr_euclid::inverse(k.inv, o);
    EXPECT(memcmp(o, k.a, sizeof(o)) == 0, "inverse of the inverse of %08x...%08x", k.a[7], k.a[0]);
  }
  // the inverse of the inverse is the value, for 2000 values below r from a fixed generator; every result is below r
  uint64_t s = 0x9e3779b97f4a7c15ull;
  size_t bad = 0;
  for (int it = 0; it < 2000; ++it) {
    uint32_t a[8], o[8], b[8];
    for (int i = 0; i < 8; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      a[i] = (uint32_t)(s >> 32);
    }
    a[7] &= 0x1fffffffu;                                     // below 2^253 < r
    a[0] |= (it & 1);                                        // both parities; never zero in practice, but keep it so
    if (!(a[0] | a[1] | a[2] | a[3] | a[4] | a[5] | a[6] | a[7])) a[0] = 1;
    fr_euclid::inverse(a, o);
    fr_euclid::inverse(o, b);
    if (memcmp(a, b, sizeof(a)) != 0 || !fr_euclid::geq(fr_euclid::R, o) || memcmp(o, fr_euclid::R, sizeof(o)) == 0) ++bad;
  }
  EXPECT(bad == 0, "%zu of 2000 round trips", bad);
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t o[8];
  fr_euclid::inverse(zero, o);                               // no caller passes it; it must end, with 0
  EXPECT(memcmp(o, zero, sizeof(o)) == 0, "inverse(0) ends with 0");
}

// The layout of every scratch lease: the regions in order with their sizes in u64 words (flags in bytes), and offsets and totals as the chain
// of pointers in the launch code gave them before the layouts, written out by hand
static void layouts() {
  {  // n = 4096: two chunks a polynomial, 6 items; the 29 root slots first
    const QuotientLayout l = quotient_layout(12, 3, false);
    const Region r[] = {WORDS(l, roots, 116), WORDS(l, totals, 24), WORDS(l, hit, 3), WORDS(l, y, 12)};
    EXPECT(layout_ok("quotient", r, l.bytes) && l.totals == 928 && l.hit == 1120 && l.y == 1144 && l.bytes == 1240, "quotient: %zu", l.bytes);
  }
  {  // the caller takes y: none in scratch
    const QuotientLayout l = quotient_layout(12, 3, true);
    const Region r[] = {WORDS(l, roots, 116), WORDS(l, totals, 24), WORDS(l, hit, 3), WORDS(l, y, 0)};
    EXPECT(layout_ok("quotient, y out", r, l.bytes) && l.y == 1144 && l.bytes == 1144, "y out: %zu", l.bytes);
  }
  {
    const QuotientLayout l = quotient_layout(0, 1, false);
    const Region r[] = {WORDS(l, roots, 116), WORDS(l, totals, 4), WORDS(l, hit, 1), WORDS(l, y, 4)};
    EXPECT(layout_ok("quotient of one", r, l.bytes) && l.totals == 928 && l.hit == 960 && l.y == 968 && l.bytes == 1000, "n = m = 1: %zu", l.bytes);
  }
  EXPECT(quotient_layout(0, SIZE_MAX, true).bytes == SAT && open_scratch_bytes(3, 2) == 512 && open_scratch_bytes(28, (size_t)1 << 40) == SAT, "saturate");
}

int main() {
  chunk_geometry();
  batch_inv_plan();
  quotient_plan();
  lone_inversion();
  layouts();
  if (fails) { printf("%d of %zu checks failed\n", fails, checked); return 1; }
  printf("OK %zu checks\n", checked);
  return 0;
}
