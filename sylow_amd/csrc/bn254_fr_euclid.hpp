// bn254_fr_euclid.hpp -- ONE inversion in Fr by the binary extended Euclidean algorithm (HAC 14.61 for an odd prime modulus), on 8 limbs of
// 32 bits: shifts, additions and subtractions only.  For the lone lane that inverts the product of a whole chunk (kzg_evals.hip) it
// replaces the Fermat power of bn254_fr.hpp (about 380 dependent Barrett products, each some 190 wide multiply-adds) by at most 1016 steps of
// a few dozen 32-bit instructions.  The inverse mod r is unique, so the words are those fr_inv yields.  Data-dependent branches: meant for
// ONE lane, never for a wavefront of different values.  Plain C++ under g++ (tests/cpp/kzg_evals_plan_test.cpp runs it against known
// inverses on a box without a GPU); __host__ __device__ under hipcc.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FR_EUCLID_FN __host__ __device__ inline
#else
#define FR_EUCLID_FN inline
#endif

namespace fr_euclid {
constexpr uint32_t R[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
// every halving takes a bit off u or v (508 bits between them at most) and every subtraction is followed by one: 1016 steps end any input
constexpr int MAX_STEPS = 1016;

FR_EUCLID_FN bool is_one(const uint32_t (&a)[8]) { return a[0] == 1 && (a[1] | a[2] | a[3] | a[4] | a[5] | a[6] | a[7]) == 0; }
FR_EUCLID_FN bool geq(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) borrow = ((uint64_t)a[i] - b[i] - borrow) >> 63;
  return borrow == 0;
}
FR_EUCLID_FN void sub(uint32_t (&a)[8], const uint32_t (&b)[8]) {      // a -= b mod 2^256
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)a[i] - b[i] - borrow;
    a[i] = (uint32_t)d;
    borrow = d >> 63;
  }
}
FR_EUCLID_FN void add_r(uint32_t (&a)[8]) {                            // a += r; a < r on entry, so the sum is below 2^255
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a[i] + R[i];
    a[i] = (uint32_t)c;
    c >>= 32;
  }
}
FR_EUCLID_FN void shr1(uint32_t (&a)[8]) {
#pragma unroll
  for (int i = 0; i < 7; ++i) a[i] = (a[i] >> 1) | (a[i + 1] << 31);
  a[7] >>= 1;
}
FR_EUCLID_FN void half_mod(uint32_t (&x)[8]) {                         // x / 2 mod r for x < r
  if (x[0] & 1) add_r(x);
  shr1(x);
}
FR_EUCLID_FN void sub_mod(uint32_t (&x)[8], const uint32_t (&y)[8]) {  // x - y mod r for x, y < r
  const bool wrap = !geq(x, y);
  sub(x, y);
  if (wrap) add_r(x);
}

// a in [1, r): a^-1 mod r in [1, r).  Invariants: x1 a = u and x2 a = v mod r, gcd(u, v) = 1, x1 and x2 below r.  a = 0 (which no caller
// passes) ends at the step bound with 0.
FR_EUCLID_FN void inverse(const uint32_t (&a)[8], uint32_t (&out)[8]) {
  uint32_t u[8], v[8], x1[8] = {1, 0, 0, 0, 0, 0, 0, 0}, x2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) { u[i] = a[i]; v[i] = R[i]; }
  for (int step = 0; step < MAX_STEPS && !is_one(u) && !is_one(v); ++step) {
    if (!(u[0] & 1)) { shr1(u); half_mod(x1); }
    else if (!(v[0] & 1)) { shr1(v); half_mod(x2); }
    else if (geq(u, v)) { sub(u, v); sub_mod(x1, x2); }
    else { sub(v, u); sub_mod(x2, x1); }
  }
  const bool from_u = is_one(u), any = from_u || is_one(v);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = any ? (from_u ? x1[i] : x2[i]) : 0u;
}
}  // namespace fr_euclid
