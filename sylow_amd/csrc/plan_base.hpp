// plan_base.hpp -- what every *_plan.hpp counts with, once: sizes that saturate instead of wrapping, the elements of a radix-2 domain, the
// rule for a pinned grid, the two tests of byte ranges and the aliasing table built on them.  Plain C++ so that tests/cpp/plan_base_test.cpp can compile it with g++ on a
// box without a GPU.  A plan header takes what it needs with `using plan_base::...`.
#pragma once
#include <cstddef>
#include <cstdint>

namespace plan_base {
constexpr size_t SAT = (size_t)-1;               // "does not fit size_t": an entry point refuses it before any lease
constexpr size_t mul_sat(size_t a, size_t b) { return b && a > SAT / b ? SAT : a * b; }
constexpr size_t add_sat(size_t a, size_t b) { return a > SAT - b ? SAT : a + b; }
// ---- the regions of ONE scratch lease, listed once: a plan header walks a Carve over the lease's regions in order, keeps the byte offset
// each call returns and, last, `at`: the byte count acquire() receives.  The launch code takes its pointers from the same offsets
// (host::Lease::at), so a lease has one description.  Saturates like the sizes above and stays SAT; a word region on an offset that is no
// multiple of 8 makes the whole lease SAT, which every entry point refuses.
struct Carve {
  size_t at = 0;
  constexpr size_t bytes(size_t n) { const size_t off = at; at = add_sat(at, n); return off; }
  constexpr size_t words(size_t n) { if (at % 8) at = SAT; return bytes(mul_sat(n, 8)); }     // n u64
  constexpr void round() { at = at > SAT - 7 ? SAT : (at + 7) & ~(size_t)7; }                 // up to a word
};
constexpr size_t words_of(size_t bytes) { return bytes == SAT ? SAT : bytes / 8; }            // a layout's bytes as u64 words, SAT kept
constexpr size_t elems(int log_n) { return (size_t)1 << log_n; }
constexpr bool max_blocks_ok(long long max_blocks) { return max_blocks != 0; }      // a pin: < 0 the default, > 0 a cap; no block is refused
// [a, a + a_bytes) and [b, b + b_bytes) share no byte and neither lies inside the other: an empty range inside a non-empty one collides
// (the sizes are not SAT; the sums cannot wrap for ranges that exist)
constexpr bool disjoint(uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) { return a + a_bytes <= b || b + b_bytes <= a; }
// the same, but an empty range overlaps nothing, wherever it points
constexpr bool disjoint_or_empty(uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) { return !a_bytes || !b_bytes || disjoint(a, a_bytes, b, b_bytes); }

// ---- the aliasing table of an entry point (host.hpp hands it on as host::outputs_disjoint): its arrays as byte ranges, and every output
// against every input and against the outputs after it, under the range test the entry point names.  A NULL array takes no part.
struct Range {
  uintptr_t p;
  size_t bytes;
};
using RangeTest = bool (*)(uintptr_t, size_t, uintptr_t, size_t);
template <size_t NI, size_t NO> constexpr bool outputs_disjoint(const Range (&in)[NI], const Range (&out)[NO], RangeTest apart) {
  for (size_t o = 0; o < NO; ++o) {
    if (!out[o].p) continue;
    for (size_t i = 0; i < NI; ++i)
      if (in[i].p && !apart(in[i].p, in[i].bytes, out[o].p, out[o].bytes)) return false;
    for (size_t k = o + 1; k < NO; ++k)
      if (out[k].p && !apart(out[k].p, out[k].bytes, out[o].p, out[o].bytes)) return false;
  }
  return true;
}
}  // namespace plan_base
