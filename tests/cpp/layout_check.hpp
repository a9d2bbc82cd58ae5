// Shared by the host plan tests: what the layout of every scratch lease must satisfy (plan_base.hpp: Carve).  A test lists a layout's regions
// in order with the sizes it expects, written out by hand, and asks layout_ok: the offsets ascend, no region starts before the end of the one
// before, every region of u64 words starts on a multiple of 8, and the last region ends at most 7 bytes before the total and never after it.
// It prints what it finds and returns false; the test puts the result into its own EXPECT.
#pragma once
#include <cstddef>
#include <cstdio>

struct Region {
  const char* name;
  size_t off, bytes;
  bool words;
};
#define WORDS(l, field, n) Region{#field, (l).field, (size_t)(n) * 8, true}
#define BYTES(l, field, n) Region{#field, (l).field, (size_t)(n), false}

template <size_t N> static bool layout_ok(const char* what, const Region (&r)[N], size_t total) {
  bool ok = true;
  size_t end = 0;
  for (size_t i = 0; i < N; ++i) {
    if (r[i].off < end) ok = false, printf("%s: %s starts at %zu, before the end %zu of the region before it\n", what, r[i].name, r[i].off, end);
    if (r[i].words && r[i].off % 8) ok = false, printf("%s: %s, a word region, starts at %zu\n", what, r[i].name, r[i].off);
    end = r[i].off + r[i].bytes;
  }
  if (end > total || total - end > 7) ok = false, printf("%s: the last region ends at %zu, the lease at %zu\n", what, end, total);
  return ok;
}
