// SHA-256 (FIPS 180-4) for RFC 9380's expand_message_xmd, one message per lane.  Host and device: the host shortens oversize tags
// with it (hasher.rs:157-173), the device hashes with it (XMDExpander<Sha256>, hasher.rs:201-250).
//
// The reference takes SHA-256 from the un-vendored crate sha2 (Cargo.toml); the function is restated here from the standard.  On the
// device every rotation is one v_alignbit_b32, Ch, Maj and the three-way XORs of the sigma functions one v_bitop3_b32 each, as the
// Keccak rounds of bn254_hash.hpp do.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include <hip/hip_runtime.h>

namespace bn254 {

#define BN_SHA256_K_LIST                                                                                                              \
  0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,  \
  0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,  \
  0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,  \
  0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,  \
  0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,  \
  0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,  \
  0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u
#if defined(__HIP_DEVICE_COMPILE__)
static __device__ const uint32_t SHA256_K[64] = {BN_SHA256_K_LIST};
#else
static const uint32_t SHA256_K[64] = {BN_SHA256_K_LIST};
#endif
#undef BN_SHA256_K_LIST

__host__ __device__ inline uint32_t sha_rotr(uint32_t x, int n) {       // n a compile-time constant in 1 .. 31
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(x, x, n);
#else
  return (x >> n) | (x << (32 - n));
#endif
}
__host__ __device__ inline uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
  return a ^ b ^ c;
#endif
}
__host__ __device__ inline uint32_t sha_ch(uint32_t e, uint32_t f, uint32_t g) {       // (e & f) ^ (~e & g): truth table 0xCA
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA);
#else
  return (e & f) ^ (~e & g);
#endif
}
__host__ __device__ inline uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) {      // majority: truth table 0xE8
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
#else
  return (a & b) ^ (a & c) ^ (b & c);
#endif
}

// One compression: h += F(h, w).  The sixteen block words double as the schedule ring -- w[t & 15] is W_t once round t has rewritten it --
// and every index into it is a compile-time constant: sixteen rounds are written out, the loop around them runs four times.  `w` is
// consumed (it holds W_48 .. W_63 afterwards).
__host__ __device__ inline void sha256_compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
  auto round = [&](uint32_t kw) {                       // kw = K_t + W_t
    const uint32_t S1 = sha_xor3(sha_rotr(e, 6), sha_rotr(e, 11), sha_rotr(e, 25));
    const uint32_t t1 = hh + S1 + sha_ch(e, f, g) + kw;
    const uint32_t S0 = sha_xor3(sha_rotr(a, 2), sha_rotr(a, 13), sha_rotr(a, 22));
    const uint32_t t2 = S0 + sha_maj(a, b, c);
    hh = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
  };
#pragma unroll
  for (int j = 0; j < 16; ++j) round(SHA256_K[j] + w[j]);
#pragma unroll 1
  for (int t0 = 16; t0 < 64; t0 += 16) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {                       // W_t = s1(W_(t-2)) + W_(t-7) + s0(W_(t-15)) + W_(t-16)
      const uint32_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
      const uint32_t s0 = sha_xor3(sha_rotr(w15, 7), sha_rotr(w15, 18), w15 >> 3);
      const uint32_t s1 = sha_xor3(sha_rotr(w2, 17), sha_rotr(w2, 19), w2 >> 10);
      w[j] = w[j] + s0 + w[(j + 9) & 15] + s1;
      round(SHA256_K[t0 + j] + w[j]);
    }
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// Streaming absorber.  Bytes are collected big-endian in a 32-bit staging register and enter the block one WORD at a time through a
// select over its sixteen words, so neither the block nor the state is ever indexed with a run-time value and both stay in registers (the
// comment above struct Keccak256 in bn254_hash.hpp has the price of the alternative).  The block is cleared after every compression:
// the padding's zero bytes are then already in place.
struct Sha256 {
  uint32_t h[8], w[16];
  uint32_t cur, fill, nblk;        // staging word, bytes in the open block (0 .. 63), blocks compressed so far
  __host__ __device__ inline void init() {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
    clear();
    nblk = 0;
  }
  // The state after one block of 64 zero bytes -- RFC 9380's Z_pad for this hash: a constant, as Keccak-f[1600](0) is for Keccak-256
  __host__ __device__ inline void init_zpad() {
    h[0] = 0xda5698beu; h[1] = 0x17b9b469u; h[2] = 0x62335799u; h[3] = 0x779fbecau;
    h[4] = 0x8ce5d491u; h[5] = 0xc0d26243u; h[6] = 0xbafef9eau; h[7] = 0x1837a9d8u;
    clear();
    nblk = 1;
  }
  __host__ __device__ inline void clear() {
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = 0;
    cur = 0;
    fill = 0;
  }
  __host__ __device__ inline void block() { sha256_compress(h, w); clear(); ++nblk; }
  __host__ __device__ inline void flush_word(uint32_t idx) {          // w[idx] = cur, idx in 0 .. 15
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) w[k] = (k == idx) ? cur : w[k];
    cur = 0;
  }
  __host__ __device__ inline void put(uint8_t byte) {
    cur = (cur << 8) | byte;
    ++fill;
    if ((fill & 3) == 0) {
      flush_word((fill >> 2) - 1);
      if (fill == 64) block();
    }
  }
  __host__ __device__ inline void update(const uint8_t* d, size_t n) {
    for (size_t i = 0; i < n; ++i) put(d[i]);
  }
  // the digest as eight big-endian words (byte j of the digest = byte 3 - (j & 3), counted from the low end, of out[j >> 2])
  __host__ __device__ inline void finish(uint32_t (&out)[8]) {
    const uint64_t bits = ((uint64_t)nblk * 64 + fill) * 8;
    cur = (cur << 8) | 0x80;
    ++fill;
    cur <<= 8 * ((4 - (fill & 3)) & 3);                 // the open word, left-aligned; the bytes behind it are zero already
    flush_word((fill - 1) >> 2);
    fill = (fill + 3) & ~3u;                            // 4 .. 64
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {              // one compression site: a block without room for the length goes first
      const bool last = fill <= 56;
      if (last) { w[14] = (uint32_t)(bits >> 32); w[15] = (uint32_t)bits; }
      sha256_compress(h, w);
      clear();
      if (last) break;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = h[i];
  }
};

inline void sha256_host(uint8_t out[32], const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {      // H(a || b), host side
  Sha256 s;
  uint32_t d[8];
  s.init();
  s.update(a, na);
  s.update(b, nb);
  s.finish(d);
  for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(d[i >> 2] >> (8 * (3 - (i & 3))));
}

}  // namespace bn254
