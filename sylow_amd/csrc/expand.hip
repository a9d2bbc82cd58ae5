// expand.hip -- hashing under a caller-chosen RFC 9380 expander and tag (bn254_expand.hpp): expand_message, hash_to_field and
// hash-to-G1 for XMD over SHA-256 and XOF over SHAKE128, expand_message of any length for XMD over Keccak-256 too, one message per
// lane at every batch size, and BLS signing on top.  A unit of its own for the reason hash.hip is one: the SvdW map wants FOUR
// wavefronts per SIMD, and amdgpu_waves_per_eu reaches the device functions only when EVERY kernel of the unit carries it -- keep it
// that way.  Expander 0 with 96 bytes goes to the existing Keccak-256 routes (hash.hip, g1.hip, sign.hip): same code, same bits.
#include "host.hpp"
#include "bn254_expand.hpp"

#define EXPAND_BOUNDS __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4)))

// Expander::expand_message: row i of the output at out + i * len_in_bytes
template <class X>
__global__ void EXPAND_BOUNDS k_expand_message_xmd(const uint8_t* msgs, const u64* off, ExpanderTag t, u32 len_in_bytes, uint8_t* out, size_t n) {
  size_t i = TID;
  if (i >= n) return;
  expand_message_xmd<X>(out + i * (size_t)len_in_bytes, len_in_bytes, msgs + off[i], (size_t)(off[i + 1] - off[i]), t);
}
__global__ void EXPAND_BOUNDS k_expand_message_xof(const uint8_t* msgs, const u64* off, ExpanderTag t, u32 len_in_bytes, uint8_t* out, size_t n) {
  size_t i = TID;
  if (i >= n) return;
  expand_message_xof(out + i * (size_t)len_in_bytes, len_in_bytes, msgs + off[i], (size_t)(off[i + 1] - off[i]), t);
}
// Expander::hash_to_field(msg, 2, 48) (hasher.rs:84-128) under expander E
template <class E>
__global__ void EXPAND_BOUNDS k_hash_to_field_expander(const uint8_t* msgs, const u64* off, ExpanderTag t, u64* out, size_t n) {
  size_t i = TID;
  if (i >= n) return;
  Fp u0, u1;
  E::hash_to_field(u0, u1, msgs + off[i], (size_t)(off[i + 1] - off[i]), t);
  store_fp(out, n, i, 0, u0);
  store_fp(out, n, i, 4, u1);
}
// k_hash_to_g1 (hash.hip) under expander E: affine, negated (the verifier's -H(m)) or projective [12][n]
template <class E>
__global__ void EXPAND_BOUNDS k_hash_to_g1_expander(const uint8_t* msgs, const u64* off, ExpanderTag t, u64* oxy, uint8_t* oinf, size_t n, int negate, u64* proj) {
  size_t i = TID;
  if (i >= n) return;
  G1P h;
  hash_to_g1_expander<E>(h, msgs + off[i], (size_t)(off[i + 1] - off[i]), t);
  if (proj) {
    store_fp(proj, n, i, 0, h.x); store_fp(proj, n, i, 4, h.y); store_fp(proj, n, i, 8, h.z);
    return;
  }
  Fp x, y; bool inf;
  g1_to_affine(x, y, inf, h);
  if (negate && !inf) y = fp_neg(y);
  store_fp(oxy, n, i, 0, x); store_fp(oxy, n, i, 4, y);
  oinf[i] = inf ? 1 : 0;
}

namespace {
int32_t refuse(const char* why) {
  snprintf(sylow_g_err, sizeof(sylow_g_err), "bad argument: %s", why);
  return SYLOW_HIP_E_ARG;
}
// the tag record of a call that passed expander_check; dst NULL = the library tag
void tag_arg(ExpanderTag& t, int32_t expander, const uint8_t* dst, size_t dst_len, int32_t security_bits) {
  DstPrime lib;
  if (!dst) { host::dst_arg(lib, nullptr, 0); dst = lib.bytes; dst_len = lib.len - 1; }
  make_expander_tag(t, expander, dst, dst_len, (unsigned)security_bits);
}
}  // namespace

namespace g1h {
// The conditions under which the reference's expand_message answers HashError::ExpandMessage (hasher.rs:211-216, and i2osp's range for
// the two length fields), checked for the whole call before anything is launched.  len_in_bytes = 96 for the hash_to_field shapes.
int32_t expander_check(int32_t expander, int32_t security_bits, size_t len_in_bytes) {
  if (expander != SYLOW_HIP_EXPANDER_XMD_KECCAK256 && expander != SYLOW_HIP_EXPANDER_XMD_SHA256 && expander != SYLOW_HIP_EXPANDER_XOF_SHAKE128)
    return refuse("unknown expander (SYLOW_HIP_EXPANDER_*)");
  if (security_bits < 1) return refuse("security_bits < 1");
  if (len_in_bytes == 0) return refuse("len_in_bytes == 0");
  if (len_in_bytes > 65535) return refuse("len_in_bytes > 65535 (I2OSP(len_in_bytes, 2))");
  if (expander == SYLOW_HIP_EXPANDER_XOF_SHAKE128) {
    if ((2 * (size_t)security_bits + 7) / 8 > 255) return refuse("XOF: ceil(2 * security_bits / 8) > 255");
  } else {
    if ((len_in_bytes + 31) / 32 > 255) return refuse("XMD: ceil(len_in_bytes / 32) > 255");
    if (2 * (size_t)security_bits > 256) return refuse("XMD: 2 * security_bits > 256, the hash's output");
  }
  return SYLOW_HIP_OK;
}
// H(m_i) or -H(m_i) affine under the expander (checked by the caller with expander_check)
int32_t hash_to_g1_expander(int32_t expander, const uint8_t* dst, size_t dst_len, int32_t security_bits, const uint8_t* msgs, const uint64_t* msg_offsets,
                            uint64_t* out_xy, uint8_t* out_inf, size_t n, int negate, void* stream) {
  if (!n) return SYLOW_HIP_OK;
  if (expander == SYLOW_HIP_EXPANDER_XMD_KECCAK256) {
    DstPrime dp; host::dst_arg(dp, dst, dst_len);
    return hash_to_g1_dst(msgs, msg_offsets, dp, out_xy, out_inf, n, negate, stream);
  }
  ExpanderTag t; tag_arg(t, expander, dst, dst_len, security_bits);
  if (expander == SYLOW_HIP_EXPANDER_XMD_SHA256) k_hash_to_g1_expander<ExpandSha256><<<GRID(n)>>>(msgs, msg_offsets, t, out_xy, out_inf, n, negate, nullptr);
  else k_hash_to_g1_expander<ExpandShake128><<<GRID(n)>>>(msgs, msg_offsets, t, out_xy, out_inf, n, negate, nullptr);
  LAUNCHED();
}
}  // namespace g1h

extern "C" {
int32_t sylow_hip_expand_message_batch(int32_t expander, const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* dst_host, size_t dst_len,
                                       int32_t security_bits, size_t len_in_bytes, uint8_t* out, size_t n, void* stream) {
  const int32_t rc = g1h::expander_check(expander, security_bits, len_in_bytes);
  if (rc != SYLOW_HIP_OK) return rc;
  ARGCHK(msgs && msg_offsets && out); if (!n) return SYLOW_HIP_OK;
  ExpanderTag t; tag_arg(t, expander, dst_host, dst_len, security_bits);
  const u32 len = (u32)len_in_bytes;
  if (expander == SYLOW_HIP_EXPANDER_XMD_KECCAK256) k_expand_message_xmd<XmdKeccak256><<<GRID(n)>>>(msgs, msg_offsets, t, len, out, n);
  else if (expander == SYLOW_HIP_EXPANDER_XMD_SHA256) k_expand_message_xmd<XmdSha256><<<GRID(n)>>>(msgs, msg_offsets, t, len, out, n);
  else k_expand_message_xof<<<GRID(n)>>>(msgs, msg_offsets, t, len, out, n);
  LAUNCHED();
}
int32_t sylow_hip_hash_to_field_expander_batch(int32_t expander, const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* dst_host, size_t dst_len,
                                               int32_t security_bits, uint64_t* out_u, size_t n, void* stream) {
  const int32_t rc = g1h::expander_check(expander, security_bits, 96);
  if (rc != SYLOW_HIP_OK) return rc;
  if (expander == SYLOW_HIP_EXPANDER_XMD_KECCAK256) return sylow_hip_hash_to_field_batch(msgs, msg_offsets, dst_host, dst_len, out_u, n, stream);
  ARGCHK(msgs && msg_offsets && out_u); if (!n) return SYLOW_HIP_OK;
  ExpanderTag t; tag_arg(t, expander, dst_host, dst_len, security_bits);
  if (expander == SYLOW_HIP_EXPANDER_XMD_SHA256) k_hash_to_field_expander<ExpandSha256><<<GRID(n)>>>(msgs, msg_offsets, t, out_u, n);
  else k_hash_to_field_expander<ExpandShake128><<<GRID(n)>>>(msgs, msg_offsets, t, out_u, n);
  LAUNCHED();
}
int32_t sylow_hip_hash_to_g1_expander_batch(int32_t expander, const uint8_t* msgs, const uint64_t* msg_offsets, const uint8_t* dst_host, size_t dst_len,
                                            int32_t security_bits, uint64_t* out_xy, uint8_t* out_inf, size_t n, void* stream) {
  const int32_t rc = g1h::expander_check(expander, security_bits, 96);
  if (rc != SYLOW_HIP_OK) return rc;
  ARGCHK(msgs && msg_offsets && out_xy && out_inf);
  return g1h::hash_to_g1_expander(expander, dst_host, dst_len, security_bits, msgs, msg_offsets, out_xy, out_inf, n, 0, stream);
}
// lib.rs:179-187 with H from the chosen suite: H(m_i) into a leased block, then the scalar multiplication of sylow_hip_g1_scalar_mul_batch
int32_t sylow_hip_bls_sign_expander_batch(int32_t expander, const uint8_t* dst_host, size_t dst_len, int32_t security_bits, const uint64_t* sk,
                                          const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t* sig_xy, uint8_t* sig_inf, size_t n, void* stream) {
  int32_t rc = g1h::expander_check(expander, security_bits, 96);
  if (rc != SYLOW_HIP_OK) return rc;
  if (expander == SYLOW_HIP_EXPANDER_XMD_KECCAK256 && !dst_host) return sylow_hip_bls_sign_batch(sk, msgs, msg_offsets, sig_xy, sig_inf, n, stream);
  ARGCHK(sk && msgs && msg_offsets && sig_xy && sig_inf); if (!n) return SYLOW_HIP_OK;
  host::Lease ws;
  if ((rc = ws.acquire(8 * n * sizeof(u64) + n, (hipStream_t)stream)) != SYLOW_HIP_OK) return rc;
  u64* h = (u64*)ws.p;
  uint8_t* hinf = (uint8_t*)(h + 8 * n);
  rc = g1h::hash_to_g1_expander(expander, dst_host, dst_len, security_bits, msgs, msg_offsets, h, hinf, n, 0, stream);
  if (rc == SYLOW_HIP_OK) rc = sylow_hip_g1_scalar_mul_batch(h, hinf, sk, sig_xy, sig_inf, n, stream);
  return host::finish(rc, ws);
}
}  // extern "C"
