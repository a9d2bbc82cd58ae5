// poseidon_params.hpp -- the parameters of Poseidon over Fr as circomlib deploys it (x^5, t = 2 .. 17, R_F = 8, R_P per width), drawn on the
// HOST by the Poseidon paper's Grain LFSR.  Plain C++ with no include of the project's: g++ compiles it alone
// (tests/cpp/poseidon_params_main.cpp prints what it draws, and tests/test_poseidon_params.py compares that with the Python model).
//   seed (80 bits, each field MSB first): 2 bits = 1 (a prime field), 4 bits = 0 (x^alpha), 12 bits = 254, 12 bits = t, 10 bits = R_F,
//   10 bits = R_P, 30 ones.  update bit = b62 ^ b51 ^ b38 ^ b23 ^ b13 ^ b0, shifted in at the end; the first 160 are discarded; an output
//   bit comes from a pair of update bits: first 1 -> emit the second, first 0 -> drop both.
//   round constants: (R_F + R_P) t draws of 254 output bits MSB first, a draw >= r rejected and redrawn; round-major.
//   matrix: 2 t draws of 254 bits, each mod r, all redrawn while two are equal; xs the first t, ys the last t, M[i][j] = (xs[i] + ys[j])^-1.
// This header yields the constants and the t^2 SUMS xs[i] + ys[j] mod r; the inverses are the device's (poseidon.hip: fr_inv, once per table).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace poseidon_params {
constexpr int T_MIN = 2, T_MAX = 17, FULL_ROUNDS = 8, FIELD_BITS = 254;
constexpr int PARTIAL_ROUNDS[T_MAX - T_MIN + 1] = {56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68};
constexpr bool width_ok(int t) { return t >= T_MIN && t <= T_MAX; }
constexpr int partial_rounds(int t) { return PARTIAL_ROUNDS[t - T_MIN]; }
constexpr int rounds(int t) { return FULL_ROUNDS + partial_rounds(t); }

struct U256 {
  uint64_t w[4];                                 // little-endian words
};
constexpr U256 FR_R = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};
inline bool less(const U256& a, const U256& b) {
  for (int i = 3; i >= 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}
inline bool equal(const U256& a, const U256& b) { return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]; }
// a - r when a >= r; for a < 2 r
inline U256 reduce_once(const U256& a) {
  if (less(a, FR_R)) return a;
  U256 o{};
  uint64_t borrow = 0;
  for (int i = 0; i < 4; ++i) {
    const uint64_t x = a.w[i], y = FR_R.w[i], d = x - y - borrow;
    borrow = (x < y) || (x == y && borrow) ? 1 : 0;
    o.w[i] = d;
  }
  return o;
}
// a + b mod r for a, b < r: the sum is below 2^255, no carry out
inline U256 add_mod(const U256& a, const U256& b) {
  U256 s{};
  uint64_t carry = 0;
  for (int i = 0; i < 4; ++i) {
    const uint64_t x = a.w[i] + carry;
    const uint64_t c1 = x < carry ? 1 : 0;
    s.w[i] = x + b.w[i];
    carry = c1 + (s.w[i] < x ? 1 : 0);
  }
  return reduce_once(s);
}

class Grain {
 public:
  explicit Grain(int t) {
    int at = 0;
    const auto put = [&](int width, uint32_t v) {
      for (int k = width - 1; k >= 0; --k) b_[at++] = (uint8_t)((v >> k) & 1);
    };
    put(2, 1); put(4, 0); put(12, FIELD_BITS); put(12, (uint32_t)t); put(10, FULL_ROUNDS); put(10, (uint32_t)partial_rounds(t)); put(30, (1u << 30) - 1);
    for (int i = 0; i < 160; ++i) update();
  }
  int bit() {
    while (!update()) update();
    return update();
  }
  // 254 output bits, MSB first: below 2^254 < 2 r
  U256 draw() {
    U256 v = {{0, 0, 0, 0}};
    for (int k = FIELD_BITS - 1; k >= 0; --k)
      if (bit()) v.w[k / 64] |= (uint64_t)1 << (k % 64);
    return v;
  }

 private:
  // the register as a ring: b_[(head_ + i) % 80] is bit i, bit 0 the oldest
  int update() {
    const auto at = [&](int i) { return b_[(head_ + i) % 80]; };
    const uint8_t n = (uint8_t)(at(62) ^ at(51) ^ at(38) ^ at(23) ^ at(13) ^ at(0));
    b_[head_] = n;                               // the oldest bit leaves, the new one is bit 79 of the shifted register
    head_ = (head_ + 1) % 80;
    return n;
  }
  uint8_t b_[80] = {};
  int head_ = 0;
};

struct Draws {
  std::vector<U256> constants;                   // [(R_F + R_P) t], round-major
  std::vector<U256> xs, ys;                      // [t] each
  std::vector<U256> sums;                        // [t][t]: xs[i] + ys[j] mod r, never 0 for the deployed widths' first draw (checked by the caller's inverse: inv(0) = 0)
};
inline Draws draw(int t) {
  Draws d;
  Grain g(t);
  const size_t n = (size_t)rounds(t) * (size_t)t;
  while (d.constants.size() < n) {
    const U256 v = g.draw();
    if (less(v, FR_R)) d.constants.push_back(v);
  }
  std::vector<U256> c((size_t)2 * t);
  for (;;) {
    for (auto& v : c) v = reduce_once(g.draw());
    bool distinct = true;
    for (size_t i = 0; i < c.size() && distinct; ++i)
      for (size_t j = i + 1; j < c.size(); ++j)
        if (equal(c[i], c[j])) { distinct = false; break; }
    if (distinct) break;
  }
  d.xs.assign(c.begin(), c.begin() + t);
  d.ys.assign(c.begin() + t, c.end());
  d.sums.resize((size_t)t * t);
  for (int i = 0; i < t; ++i)
    for (int j = 0; j < t; ++j) d.sums[(size_t)i * t + j] = add_mod(d.xs[i], d.ys[j]);
  return d;
}
}  // namespace poseidon_params
