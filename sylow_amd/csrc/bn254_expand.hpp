// RFC 9380 expand_message under a caller-chosen expander, one message per lane: expand_message_xmd over Keccak-256 or SHA-256
// (XMDExpander<D>, hasher.rs:201-250) and expand_message_xof over SHAKE128 (XOFExpander<D>, hasher.rs:315-329), any output length, and
// Expander::hash_to_field(msg, 2, 48) (hasher.rs:84-128) / G1Projective::hash_to_curve (g1.rs:307-331) on top of them.  The fixed
// Keccak-256 suite with its 96-byte shortcuts stays in bn254_hash.hpp; fp_from_be48, svdw_map2 and g1_add are shared with it.
//
// Every hash here is fed from ONE loop over the bytes of msg' (MsgPrime below) and closed by one padding routine: each call site of a
// compression function is a copy of it in the kernel, and a copy per put() of the header bytes is ~1 k instructions each for SHA-256.
#pragma once
#include <string.h>

#include "bn254_hash.hpp"
#include "bn254_sha256.hpp"

namespace bn254 {

enum { EXPANDER_XMD_KECCAK256 = 0, EXPANDER_XMD_SHA256 = 1, EXPANDER_XOF_SHAKE128 = 2 };

// The tag record of one call, prepared on the host (make_expander_tag): DST' and what the b_i blocks of its expander can take ready-made.
struct ExpanderTag {
  DstPrime dp;             // DST || I2OSP(len(DST), 1), the tag already shortened by the expander's own hash if it was > 255 bytes;
                           // tail / tail_ok (Keccak's one-block b_i) only for EXPANDER_XMD_KECCAK256
  // SHA-256's one-block b_i message (32 bytes, the block counter, DST', 0x80, zeros, the bit length) from byte 32 on, as the big-endian
  // block words 8 .. 15 with the counter byte zero (it is OR-ed in).  Valid when 33 + len(DST') + 9 <= 64 (sha_tail_ok).
  uint32_t sha_tail[8];
  uint32_t sha_tail_ok;
};

// SHAKE128 (FIPS 202): the sponge of Keccak256 at rate 168 bytes = 21 words, domain byte 0x1F, final bit 0x80.  Same staging as
// Keccak256 (bn254_hash.hpp): the state is only ever indexed with constants.
struct Shake128 {
  u64 s[25];
  u64 cur;
  uint32_t fill;
  __host__ __device__ inline void init() {
#pragma unroll
    for (int i = 0; i < 25; ++i) s[i] = 0;
    cur = 0;
    fill = 0;
  }
  __host__ __device__ inline void flush_word(uint32_t idx) {          // s[idx] ^= cur, idx in 0 .. 20
#pragma unroll
    for (uint32_t w = 0; w < 21; ++w) s[w] ^= (w == idx) ? cur : 0ull;
    cur = 0;
  }
  __host__ __device__ inline void put(uint8_t byte) {
    cur |= (u64)byte << (8 * (fill & 7));
    ++fill;
    if ((fill & 7) == 0) {
      flush_word((fill >> 3) - 1);
      if (fill == 168) { keccak_f1600(s); fill = 0; }
    }
  }
  __host__ __device__ inline void update(const uint8_t* d, size_t n) {
    for (size_t i = 0; i < n; ++i) put(d[i]);
  }
  // pads and permutes: s[0 .. 20] is then the first 168 bytes of output, little-endian; keccak_f1600(s) gives each further 168
  __host__ __device__ inline void pad() {
    cur |= (u64)0x1F << (8 * (fill & 7));
    flush_word(fill >> 3);
    s[20] ^= 0x8000000000000000ull;                   // last byte of the 168-byte rate block
    keccak_f1600(s);
  }
};

inline void shake128_host(uint8_t* out, size_t n_out, const uint8_t* a, size_t na, const uint8_t* b, size_t nb) {   // SHAKE128(a || b, n_out)
  Shake128 k;
  k.init();
  k.update(a, na);
  k.update(b, nb);
  k.pad();
  for (size_t i = 0; i < n_out; ++i) {
    if (i && i % 168 == 0) keccak_f1600(k.s);
    const size_t j = i % 168;
    out[i] = (uint8_t)(k.s[j >> 3] >> (8 * (j & 7)));
  }
}

// hasher.rs:157-173 / 274-290: DST' for the expander (host side, once per call).  security_bits only sizes SHAKE128's shortened tag.
inline void make_expander_tag(ExpanderTag& t, int expander, const uint8_t* dst, size_t len, unsigned security_bits) {
  memset(&t, 0, sizeof(t));
  if (expander == EXPANDER_XMD_KECCAK256) { make_dst_prime(t.dp, dst, len); return; }
  uint8_t h[256];
  if (len > 255) {
    const uint8_t* prefix = (const uint8_t*)"H2C-OVERSIZE-DST-";
    if (expander == EXPANDER_XMD_SHA256) {
      sha256_host(h, prefix, 17, dst, len);
      len = 32;
    } else {
      const size_t out = (2 * (size_t)security_bits + 7) / 8;      // <= 255: checked with the other whole-call conditions
      shake128_host(h, out, prefix, 17, dst, len);
      len = out;
    }
    dst = h;
  }
  for (size_t i = 0; i < len; ++i) t.dp.bytes[i] = dst[i];
  t.dp.bytes[len] = (uint8_t)len;
  t.dp.len = (uint32_t)len + 1;
  if (expander == EXPANDER_XMD_SHA256 && 33 + t.dp.len + 9 <= 64) {
    uint8_t blk[64];
    for (int i = 0; i < 64; ++i) blk[i] = 0;
    for (uint32_t i = 0; i < t.dp.len; ++i) blk[33 + i] = t.dp.bytes[i];
    blk[33 + t.dp.len] = 0x80;
    const uint32_t bits = 8 * (33 + t.dp.len);
    blk[62] = (uint8_t)(bits >> 8);
    blk[63] = (uint8_t)bits;
    for (int w = 0; w < 8; ++w)
      t.sha_tail[w] = ((uint32_t)blk[32 + 4 * w] << 24) | ((uint32_t)blk[33 + 4 * w] << 16) | ((uint32_t)blk[34 + 4 * w] << 8) | blk[35 + 4 * w];
    t.sha_tail_ok = 1;
  }
}

// msg || I2OSP(len_in_bytes, 2) [|| I2OSP(0, 1)] || DST' as one byte stream: what b_0 (XMD, after Z_pad) and the XOF absorb
struct MsgPrime {
  const uint8_t* msg;
  size_t msg_len;
  uint32_t len_in_bytes, n_hdr;        // n_hdr = 3 for XMD, 2 for XOF
  __device__ inline size_t size(const DstPrime& dp) const { return msg_len + n_hdr + dp.len; }
  __device__ inline uint8_t at(size_t pos, const DstPrime& dp) const {
    if (pos < msg_len) return msg[pos];
    const size_t q = pos - msg_len;
    if (q < n_hdr) return q == 0 ? (uint8_t)(len_in_bytes >> 8) : q == 1 ? (uint8_t)len_in_bytes : (uint8_t)0;
    return dp.bytes[q - n_hdr];
  }
};

// ---- expand_message_xmd (hasher.rs:201-250), split at the hash: b_0, then b_i from b_0 xor b_(i-1) ---------------------------------
// An XMD hash gives: word / NW (the 32-byte digest as NW words), b0(), bi() and byte() (byte j of a digest, j a compile-time constant).
struct XmdSha256 {
  typedef u32 word;
  static constexpr int NW = 8;                       // big-endian words
  __device__ static inline void b0(word (&b)[8], const MsgPrime& mp, const ExpanderTag& t) {
    Sha256 s;
    s.init_zpad();
    const size_t total = mp.size(t.dp);
#pragma unroll 1
    for (size_t pos = 0; pos < total; ++pos) s.put(mp.at(pos, t.dp));
    s.finish(b);
  }
  // x = b_0 xor b_(i-1) (b_0 for i = 1): H(x || I2OSP(i, 1) || DST')
  __device__ static inline void bi(word (&o)[8], const word (&x)[8], u32 blk, const ExpanderTag& t) {
    Sha256 s;
    s.init();
#pragma unroll
    for (int i = 0; i < 8; ++i) s.w[i] = x[i];
    if (t.sha_tail_ok) {                                 // one block, its second half the same for every message
#pragma unroll
      for (int i = 0; i < 8; ++i) s.w[8 + i] = t.sha_tail[i];
      s.w[8] |= blk << 24;
      sha256_compress(s.h, s.w);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = s.h[i];
      return;
    }
    s.fill = 32;
    const u32 total = 1 + t.dp.len;
#pragma unroll 1
    for (u32 q = 0; q < total; ++q) s.put(q == 0 ? (uint8_t)blk : t.dp.bytes[q - 1]);
    s.finish(o);
  }
  __device__ static inline uint8_t byte(const word (&b)[8], int j) { return (uint8_t)(b[j >> 2] >> (8 * (3 - (j & 3)))); }
};

struct XmdKeccak256 {
  typedef u64 word;
  static constexpr int NW = 4;                       // little-endian words
  __device__ static inline void close(Keccak256& k) {   // Keccak256::finish without the byte output: the digest stays in s[0 .. 3]
    k.cur |= (u64)0x01 << (8 * (k.fill & 7));
    k.flush_word(k.fill >> 3);
    k.s[16] ^= 0x8000000000000000ull;
    keccak_f1600(k.s);
  }
  __device__ static inline void b0(word (&b)[4], const MsgPrime& mp, const ExpanderTag& t) {
    Keccak256 k;
    k.init();
    {                                                    // Z_pad absorbed: Keccak-f[1600](0), as in expand_message_xmd96
      const u64 z[25] = {0xf1258f7940e1dde7ull, 0x84d5ccf933c0478aull, 0xd598261ea65aa9eeull, 0xbd1547306f80494dull, 0x8b284e056253d057ull,
                         0xff97a42d7f8e6fd4ull, 0x90fee5a0a44647c4ull, 0x8c5bda0cd6192e76ull, 0xad30a6f71b19059cull, 0x30935ab7d08ffc64ull,
                         0xeb5aa93f2317d635ull, 0xa9a6e6260d712103ull, 0x81a57c16dbcf555full, 0x43b831cd0347c826ull, 0x01f22f1a11a5569full,
                         0x05e5635a21d9ae61ull, 0x64befef28cc970f2ull, 0x613670957bc46611ull, 0xb87c5a554fd00ecbull, 0x8c3ee88a1ccf32c8ull,
                         0x940c7922ae3a2614ull, 0x1841f924a2c509e4ull, 0x16f53526e70465c2ull, 0x75f644e97f30a13bull, 0xeaf1ff7b5ceca249ull};
#pragma unroll
      for (int i = 0; i < 25; ++i) k.s[i] = z[i];
    }
    const size_t total = mp.size(t.dp);
#pragma unroll 1
    for (size_t pos = 0; pos < total; ++pos) k.put(mp.at(pos, t.dp));
    close(k);
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = k.s[i];
  }
  __device__ static inline void bi(word (&o)[4], const word (&x)[4], u32 blk, const ExpanderTag& t) {
    Keccak256 k;
    k.init();
#pragma unroll
    for (int i = 0; i < 4; ++i) k.s[i] = x[i];
    if (t.dp.tail_ok) {                                  // one block whose words 4 .. 16 are the same for every message
#pragma unroll
      for (int i = 4; i < 17; ++i) k.s[i] = t.dp.tail[i];
      k.s[4] |= (u64)blk;
      keccak_f1600(k.s);
    } else {
      k.fill = 32;
      const u32 total = 1 + t.dp.len;
#pragma unroll 1
      for (u32 q = 0; q < total; ++q) k.put(q == 0 ? (uint8_t)blk : t.dp.bytes[q - 1]);
      close(k);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = k.s[i];
  }
  __device__ static inline uint8_t byte(const word (&b)[4], int j) { return (uint8_t)(b[j >> 3] >> (8 * (j & 7))); }
};

// out[0 .. len_in_bytes) = b_1 || b_2 || ... truncated; 1 <= len_in_bytes <= 255 * 32 (checked on the host)
template <class X>
__device__ inline void expand_message_xmd(uint8_t* out, u32 len_in_bytes, const uint8_t* msg, size_t msg_len, const ExpanderTag& t) {
  typename X::word b0[X::NW], x[X::NW], b[X::NW];
  X::b0(b0, MsgPrime{msg, msg_len, len_in_bytes, 3}, t);
#pragma unroll
  for (int i = 0; i < X::NW; ++i) x[i] = b0[i];
  const u32 ell = (len_in_bytes + 31) / 32;
#pragma unroll 1
  for (u32 blk = 1; blk <= ell; ++blk) {
    X::bi(b, x, blk, t);
    const u32 base = 32 * (blk - 1);
#pragma unroll
    for (int j = 0; j < 32; ++j)
      if (base + j < len_in_bytes) out[base + j] = X::byte(b, j);
#pragma unroll
    for (int i = 0; i < X::NW; ++i) x[i] = b0[i] ^ b[i];
  }
}

// ---- expand_message_xof (hasher.rs:315-329): SHAKE128(msg || I2OSP(len, 2) || DST', len) --------------------------------------------
__device__ inline void shake128_absorb_msg_prime(Shake128& k, u32 len_in_bytes, const uint8_t* msg, size_t msg_len, const ExpanderTag& t) {
  const MsgPrime mp{msg, msg_len, len_in_bytes, 2};
  k.init();
  const size_t total = mp.size(t.dp);
#pragma unroll 1
  for (size_t pos = 0; pos < total; ++pos) k.put(mp.at(pos, t.dp));
  k.pad();
}
__device__ inline void expand_message_xof(uint8_t* out, u32 len_in_bytes, const uint8_t* msg, size_t msg_len, const ExpanderTag& t) {
  Shake128 k;
  shake128_absorb_msg_prime(k, len_in_bytes, msg, msg_len, t);
#pragma unroll 1
  for (u32 base = 0; base < len_in_bytes; base += 168) {     // one rate block of output per permutation
    if (base) keccak_f1600(k.s);
#pragma unroll
    for (int j = 0; j < 168; ++j)
      if (base + j < len_in_bytes) out[base + j] = (uint8_t)(k.s[j >> 3] >> (8 * (j & 7)));
  }
}

// ---- Expander::hash_to_field(msg, 2, 48) (hasher.rs:84-128): 96 bytes, two 48-byte big-endian values mod p ----------------------------
struct ExpandSha256 {
  __device__ static inline void hash_to_field(Fp& u0, Fp& u1, const uint8_t* msg, size_t msg_len, const ExpanderTag& t) {
    u32 b0[8], x[8], b[8], em[24];                      // em: the 96 bytes as big-endian words -- the limbs of the two values as they are
    XmdSha256::b0(b0, MsgPrime{msg, msg_len, 96, 3}, t);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = b0[i];
#pragma unroll
    for (int i = 0; i < 24; ++i) em[i] = 0;
#pragma unroll 1
    for (u32 blk = 1; blk <= 3; ++blk) {                 // one copy of b_i's code; the store is a select, not an index
      XmdSha256::bi(b, x, blk, t);
#pragma unroll
      for (int i = 0; i < 24; ++i) em[i] = ((u32)(i >> 3) == blk - 1) ? b[i & 7] : em[i];
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = b0[i] ^ b[i];
    }
    Fp lo, hi;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
#pragma unroll
      for (int i = 0; i < 8; ++i) lo.v[i] = em[12 * e + 11 - i];
#pragma unroll
      for (int i = 0; i < 8; ++i) hi.v[i] = i < 4 ? em[12 * e + 3 - i] : 0u;
      (e ? u1 : u0) = fp_from_wide_limbs(lo, hi);
    }
  }
};
struct ExpandShake128 {
  __device__ static inline void hash_to_field(Fp& u0, Fp& u1, const uint8_t* msg, size_t msg_len, const ExpanderTag& t) {
    Shake128 k;
    shake128_absorb_msg_prime(k, 96, msg, msg_len, t);    // 96 <= 168: the first output block holds it all
    const u64 a[6] = {k.s[0], k.s[1], k.s[2], k.s[3], k.s[4], k.s[5]}, b[6] = {k.s[6], k.s[7], k.s[8], k.s[9], k.s[10], k.s[11]};
    u0 = fp_from_be48_words(a);
    u1 = fp_from_be48_words(b);
  }
};
struct ExpandKeccak256 {                                 // the fixed suite's 96-byte route (bn254_hash.hpp) under the same interface
  __device__ static inline void hash_to_field(Fp& u0, Fp& u1, const uint8_t* msg, size_t msg_len, const ExpanderTag& t) {
    u64 em[12];
    expand_message_xmd96_words(em, msg, msg_len, t.dp);
    const u64 a[6] = {em[0], em[1], em[2], em[3], em[4], em[5]}, b[6] = {em[6], em[7], em[8], em[9], em[10], em[11]};
    u0 = fp_from_be48_words(a);
    u1 = fp_from_be48_words(b);
  }
};

// g1.rs:307-331 under expander E: map(u0) + map(u1) with the complete projective addition; projective result
template <class E>
__device__ inline bool hash_to_g1_expander(G1P& out, const uint8_t* msg, size_t msg_len, const ExpanderTag& t) {
  Fp u0, u1;
  E::hash_to_field(u0, u1, msg, msg_len, t);
  Fp x0, y0, x1, y1;
  const bool ok = svdw_map2(x0, y0, x1, y1, u0, u1);
  const G1P a{x0, y0, fp_one()}, b{x1, y1, fp_one()};
  out = g1_add(a, b);
  return ok;
}

}  // namespace bn254
