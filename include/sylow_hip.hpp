// sylow_hip.hpp -- header-only C++17 host layer over the C ABI (sylow_hip.h).
//
// The reference is a compiled (Rust) library and no Rust toolchain exists in the build image, so
// this is the host side "in the reference's shape" that CAN be compiled here: the same item names
// and argument meaning as sylow's public API for the hot path (src/lib.rs:71-84,179-236;
// src/pairing.rs:870-893,1029-1037), batch-first.  A Rust shim binding the same C entry points
// is listed in INTEGRATION.md.  Host containers are array-of-structs (what a Rust
// Vec<G1Affine> would convert to); the device-side transposition to struct-of-arrays is done by
// sylow_hip_aos_to_soa / _soa_to_aos, so no host loop touches the limbs.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sylow_hip.h"

namespace sylow {

struct Fp { uint64_t w[4]; };                       // canonical value, little-endian limbs (Fp::value().to_words())
struct Fp2 { Fp c0, c1; };
struct Fp12 { Fp c[12]; };
struct G1Affine { Fp x, y; };                       // 8 words; infinity flags travel separately
struct G2Affine { Fp2 x, y; };                      // 16 words
struct Gt { Fp12 v; };
inline bool operator==(const Gt& a, const Gt& b) {
  for (int i = 0; i < 12; ++i) for (int k = 0; k < 4; ++k) if (a.v.c[i].w[k] != b.v.c[i].w[k]) return false;
  return true;
}
enum class GroupError { NotOnCurve = 1, NotInSubgroup = 2, CannotHashToGroup = 3, DecodeError = 4 };   // groups/group.rs:38-47

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };
inline void check(int32_t rc, const char* what) {
  if (rc != SYLOW_HIP_OK) throw Error(std::string(what) + ": " + sylow_hip_last_error());
}

class DeviceBuffer {                                 // RAII hipMalloc'ed bytes
 public:
  explicit DeviceBuffer(size_t bytes) : bytes_(bytes) { check(sylow_hip_malloc(&p_, bytes), "sylow_hip_malloc"); }
  ~DeviceBuffer() { if (p_) sylow_hip_free(p_); }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; }
  template <class T> T* as() const { return static_cast<T*>(p_); }
  size_t bytes() const { return bytes_; }
 private:
  void* p_ = nullptr;
  size_t bytes_;
};

// host AoS vector of W-word structs -> device SoA [W][n]
template <class T>
DeviceBuffer to_device_soa(const std::vector<T>& v, void* stream = nullptr) {
  constexpr size_t W = sizeof(T) / 8;
  const size_t n = v.size();
  DeviceBuffer aos(n * sizeof(T) + 8), soa(n * sizeof(T) + 8);
  if (n) {
    check(sylow_hip_memcpy_h2d(aos.as<void>(), v.data(), n * sizeof(T), stream), "h2d");
    check(sylow_hip_aos_to_soa(aos.as<uint64_t>(), soa.as<uint64_t>(), W, n, stream), "aos_to_soa");
    check(sylow_hip_stream_sync(stream), "sync");
  }
  return soa;
}
template <class T>
std::vector<T> from_device_soa(const DeviceBuffer& soa, size_t n, void* stream = nullptr) {
  constexpr size_t W = sizeof(T) / 8;
  std::vector<T> out(n);
  if (n) {
    DeviceBuffer aos(n * sizeof(T));
    check(sylow_hip_soa_to_aos(soa.as<uint64_t>(), aos.as<uint64_t>(), W, n, stream), "soa_to_aos");
    check(sylow_hip_memcpy_d2h(out.data(), aos.as<void>(), n * sizeof(T), stream), "d2h");
    check(sylow_hip_stream_sync(stream), "sync");
  }
  return out;
}
inline DeviceBuffer to_device_bytes(const std::vector<uint8_t>& v) {
  DeviceBuffer d(v.size() + 8);
  if (!v.empty()) { check(sylow_hip_memcpy_h2d(d.as<void>(), v.data(), v.size(), nullptr), "h2d"); check(sylow_hip_stream_sync(nullptr), "sync"); }
  return d;
}

// optional identity flags (one byte per element; nullptr = no element is the identity)
struct Flags {
  DeviceBuffer d;
  const uint8_t* ptr;
  Flags(const std::vector<uint8_t>* v, size_t n) : d(n + 8), ptr(nullptr) {
    if (v) {
      if (v->size() != n) throw Error("identity flags: length mismatch");
      if (n) { check(sylow_hip_memcpy_h2d(d.as<void>(), v->data(), n, nullptr), "h2d"); check(sylow_hip_stream_sync(nullptr), "sync"); }
      ptr = d.as<uint8_t>();
    }
  }
};
inline void fetch_flags(std::vector<uint8_t>* out, const DeviceBuffer& d, size_t n) {
  if (!out) return;
  out->resize(n);
  if (n) { check(sylow_hip_memcpy_d2h(out->data(), d.as<void>(), n, nullptr), "d2h"); check(sylow_hip_stream_sync(nullptr), "sync"); }
}

inline G1Affine g1_generator() { return G1Affine{Fp{{1, 0, 0, 0}}, Fp{{2, 0, 0, 0}}}; }                 // g1.rs:54-60
inline G2Affine g2_generator() {                                                                       // g2.rs:47-77
  return G2Affine{Fp2{Fp{{0x46DEBD5CD992F6EDull, 0x674322D4F75EDADDull, 0x426A00665E5C4479ull, 0x1800DEEF121F1E76ull}},
                      Fp{{0x97E485B7AEF312C2ull, 0xF1AA493335A9E712ull, 0x7260BFB731FB5D25ull, 0x198E9393920D483Aull}}},
                  Fp2{Fp{{0x4CE6CC0166FA7DAAull, 0xE3D1E7690C43D37Bull, 0x4AAB71808DCB408Full, 0x12C85EA5DB8C6DEBull}},
                      Fp{{0x55ACDADCD122975Bull, 0xBC4B313370B38EF3ull, 0xEC9E99AD690C3395ull, 0x090689D0585FF075ull}}}};
}

// pairing(&G1Projective, &G2Projective) -> Gt (pairing.rs:870-893), elementwise over the batch
inline std::vector<Gt> pairing(const std::vector<G1Affine>& p, const std::vector<G2Affine>& q,
                               const std::vector<uint8_t>* p_inf = nullptr, const std::vector<uint8_t>* q_inf = nullptr) {
  if (p.size() != q.size()) throw Error("pairing: length mismatch");
  const size_t n = p.size();
  if ((p_inf && p_inf->size() != n) || (q_inf && q_inf->size() != n)) throw Error("identity flags: length mismatch");
  // host vectors in, host vector out: the chunked, double-buffered pipeline (copies of chunk k - 1 / k + 1 beside the kernels of chunk k)
  std::vector<Gt> out(n);
  check(sylow_hip_pairing_host(reinterpret_cast<const uint64_t*>(p.data()), p_inf ? p_inf->data() : nullptr, reinterpret_cast<const uint64_t*>(q.data()),
                               q_inf ? q_inf->data() : nullptr, reinterpret_cast<uint64_t*>(out.data()), n, 0), "sylow_hip_pairing_host");
  return out;
}
// the same through explicit upload -> sylow_hip_pairing_batch -> download on one stream (what the pipeline must equal bit for bit)
inline std::vector<Gt> pairing_unpipelined(const std::vector<G1Affine>& p, const std::vector<G2Affine>& q,
                                           const std::vector<uint8_t>* p_inf = nullptr, const std::vector<uint8_t>* q_inf = nullptr) {
  if (p.size() != q.size()) throw Error("pairing: length mismatch");
  const size_t n = p.size();
  auto dp = to_device_soa(p); auto dq = to_device_soa(q);
  DeviceBuffer dgt(n * sizeof(Gt) + 8);
  Flags dpi(p_inf, n), dqi(q_inf, n);
  check(sylow_hip_pairing_batch(dp.as<uint64_t>(), dpi.ptr, dq.as<uint64_t>(), dqi.ptr, dgt.as<uint64_t>(), n, nullptr), "sylow_hip_pairing_batch");
  return from_device_soa<Gt>(dgt, n);
}
// glued_pairing(&[G1Projective], &[G2Projective]) -> Gt (pairing.rs:1029-1037): ONE product.  Identity flags as in the reference:
// skip_infinity = false replays it (flags only shape Z of the G2 point, a G2 identity zeroes the product),
// true drops pairs with an identity on either side (EIP-197).
inline Gt glued_pairing(const std::vector<G1Affine>& g1s, const std::vector<G2Affine>& g2s,
                        const std::vector<uint8_t>* g1_inf = nullptr, const std::vector<uint8_t>* g2_inf = nullptr, bool skip_infinity = false) {
  const size_t k = g1s.size() < g2s.size() ? g1s.size() : g2s.size();        // zip truncates (pairing.rs:975)
  std::vector<G1Affine> a(g1s.begin(), g1s.begin() + k);
  std::vector<G2Affine> b(g2s.begin(), g2s.begin() + k);
  std::vector<uint8_t> ai, bi;
  if ((g1_inf && g1_inf->size() < k) || (g2_inf && g2_inf->size() < k)) throw Error("glued_pairing: identity flags shorter than the point list");
  if (g1_inf) ai.assign(g1_inf->begin(), g1_inf->begin() + k);
  if (g2_inf) bi.assign(g2_inf->begin(), g2_inf->begin() + k);
  auto dp = to_device_soa(a); auto dq = to_device_soa(b);
  Flags dpi(g1_inf ? &ai : nullptr, k), dqi(g2_inf ? &bi : nullptr, k);
  DeviceBuffer dgt(sizeof(Gt));
  // the whole batch as one product, spread over the GPU (chunked Miller loops, product tree, one final exponentiation)
  check(sylow_hip_pairing_product_batch(dp.as<uint64_t>(), dpi.ptr, dq.as<uint64_t>(), dqi.ptr, k, skip_infinity ? 1 : 0, dgt.as<uint64_t>(), nullptr, nullptr),
        "sylow_hip_pairing_product_batch");
  return from_device_soa<Gt>(dgt, 1)[0];
}
// Mul<&Fp> for G1 / G2 (group.rs:639-667), elementwise
// inf_out receives the identity flags of the results (k = 0, k = r, identity in -> identity out); p_inf marks identity inputs
inline std::vector<G1Affine> mul(const std::vector<G1Affine>& p, const std::vector<Fp>& k, std::vector<uint8_t>* inf_out = nullptr,
                                 const std::vector<uint8_t>* p_inf = nullptr) {
  if (p.size() != k.size()) throw Error("G1 * Fp: length mismatch");
  const size_t n = p.size();
  auto dp = to_device_soa(p); auto dk = to_device_soa(k);
  Flags dpi(p_inf, n);
  DeviceBuffer dout(n * sizeof(G1Affine) + 8), dinf(n + 8);
  check(sylow_hip_g1_scalar_mul_batch(dp.as<uint64_t>(), dpi.ptr, dk.as<uint64_t>(), dout.as<uint64_t>(), dinf.as<uint8_t>(), n, nullptr), "g1_scalar_mul");
  fetch_flags(inf_out, dinf, n);
  return from_device_soa<G1Affine>(dout, n);
}
// in_subgroup: every p[i] is in the r-torsion (what G2Projective::new guarantees upstream): the endomorphism-split product
inline std::vector<G2Affine> mul(const std::vector<G2Affine>& p, const std::vector<Fp>& k, std::vector<uint8_t>* inf_out = nullptr,
                                 const std::vector<uint8_t>* p_inf = nullptr, bool in_subgroup = false) {
  if (p.size() != k.size()) throw Error("G2 * Fp: length mismatch");
  const size_t n = p.size();
  auto dp = to_device_soa(p); auto dk = to_device_soa(k);
  Flags dpi(p_inf, n);
  DeviceBuffer dout(n * sizeof(G2Affine) + 8), dinf(n + 8);
  check((in_subgroup ? sylow_hip_g2_scalar_mul_subgroup_batch : sylow_hip_g2_scalar_mul_batch)(dp.as<uint64_t>(), dpi.ptr, dk.as<uint64_t>(), dout.as<uint64_t>(), dinf.as<uint8_t>(), n, nullptr), "g2_scalar_mul");
  fetch_flags(inf_out, dinf, n);
  return from_device_soa<G2Affine>(dout, n);
}
// Mul<&Fr> for &Gt (groups/gt.rs:161-187), elementwise: gt[i] "times" k[i]
inline std::vector<Gt> mul(const std::vector<Gt>& gt, const std::vector<Fp>& k) {
  if (gt.size() != k.size()) throw Error("Gt * Fr: length mismatch");
  const size_t n = gt.size();
  auto dg = to_device_soa(gt); auto dk = to_device_soa(k);
  DeviceBuffer dout(n * sizeof(Gt) + 8);
  check(sylow_hip_gt_pow_batch(dg.as<uint64_t>(), dk.as<uint64_t>(), dout.as<uint64_t>(), n, nullptr), "sylow_hip_gt_pow_batch");
  return from_device_soa<Gt>(dout, n);
}
// Fr arithmetic (fields/fp.rs:556-565), elementwise on canonical values carried in the Fp container
namespace fr {
inline std::vector<Fp> binop(int32_t (*fn)(const uint64_t*, const uint64_t*, uint64_t*, size_t, void*), const std::vector<Fp>& a, const std::vector<Fp>& b) {
  if (a.size() != b.size()) throw Error("Fr: length mismatch");
  auto da = to_device_soa(a); auto db = to_device_soa(b);
  DeviceBuffer dout(a.size() * sizeof(Fp) + 8);
  check(fn(da.as<uint64_t>(), db.as<uint64_t>(), dout.as<uint64_t>(), a.size(), nullptr), "fr binop");
  return from_device_soa<Fp>(dout, a.size());
}
inline std::vector<Fp> add(const std::vector<Fp>& a, const std::vector<Fp>& b) { return binop(sylow_hip_fr_add_batch, a, b); }
inline std::vector<Fp> sub(const std::vector<Fp>& a, const std::vector<Fp>& b) { return binop(sylow_hip_fr_sub_batch, a, b); }
inline std::vector<Fp> mul(const std::vector<Fp>& a, const std::vector<Fp>& b) { return binop(sylow_hip_fr_mul_batch, a, b); }
inline std::vector<Fp> inv(const std::vector<Fp>& a) {
  auto da = to_device_soa(a);
  DeviceBuffer dout(a.size() * sizeof(Fp) + 8);
  check(sylow_hip_fr_inv_batch(da.as<uint64_t>(), dout.as<uint64_t>(), a.size(), nullptr), "sylow_hip_fr_inv_batch");
  return from_device_soa<Fp>(dout, a.size());
}
// The same values as inv (inv(0) = 0) by Montgomery's trick (sylow_hip_fr_batch_inv): the elements of a chunk of 2048 share ONE inversion
inline std::vector<Fp> batch_inv(const std::vector<Fp>& a) {
  auto da = to_device_soa(a);
  DeviceBuffer dout(a.size() * sizeof(Fp) + 8);
  check(sylow_hip_fr_batch_inv(da.as<uint64_t>(), dout.as<uint64_t>(), a.size(), nullptr), "sylow_hip_fr_batch_inv");
  return from_device_soa<Fp>(dout, a.size());
}
// The transform on the domain of n = a.size() = 2^log_n points (sylow_hip_fr_ntt_batch_tuned), natural order in and out.  forward:
// out_i = sum_k a_k (g w_n^i)^k; inverse: out_k = n^-1 g^-k sum_i a_i w_n^(-ik); shift = the coset shift g (nullptr: 1); stages >= 1 pins the
// stages of a pass (the values do not depend on it).  Any 256-bit words in, taken mod r; canonical words out.
inline std::vector<std::vector<Fp>> ntt(const std::vector<std::vector<Fp>>& arrays, bool inverse = false, const Fp* shift = nullptr, int32_t stages = -1) {
  const size_t m = arrays.size(), n = m ? arrays[0].size() : 1;
  int32_t log_n = 0;
  while (((size_t)1 << log_n) < n) ++log_n;
  if (n != (size_t)1 << log_n) throw Error("fr::ntt: the length is a power of two");
  std::vector<uint64_t> flat(4 * n * m);
  for (size_t j = 0; j < m; ++j) {
    if (arrays[j].size() != n) throw Error("fr::ntt: arrays of one length");
    for (size_t k = 0; k < n; ++k) for (size_t w = 0; w < 4; ++w) flat[(j * 4 + w) * n + k] = arrays[j][k].w[w];
  }
  DeviceBuffer din(flat.size() * sizeof(uint64_t) + 8), dout(flat.size() * sizeof(uint64_t) + 8), dshift(sizeof(Fp));
  if (m) check(sylow_hip_memcpy_h2d(din.as<void>(), flat.data(), flat.size() * sizeof(uint64_t), nullptr), "h2d");
  if (shift) check(sylow_hip_memcpy_h2d(dshift.as<void>(), shift->w, sizeof(Fp), nullptr), "h2d");
  check(sylow_hip_fr_ntt_batch_tuned(din.as<uint64_t>(), log_n, m, inverse ? 1 : 0, shift ? dshift.as<uint64_t>() : nullptr, stages, dout.as<uint64_t>(), nullptr),
        "sylow_hip_fr_ntt_batch_tuned");
  if (m) check(sylow_hip_memcpy_d2h(flat.data(), dout.as<void>(), flat.size() * sizeof(uint64_t), nullptr), "d2h");
  check(sylow_hip_stream_sync(nullptr), "sync");
  std::vector<std::vector<Fp>> out(m, std::vector<Fp>(n));
  for (size_t j = 0; j < m; ++j) for (size_t k = 0; k < n; ++k) for (size_t w = 0; w < 4; ++w) out[j][k].w[w] = flat[(j * 4 + w) * n + k];
  return out;
}
inline std::vector<Fp> ntt(const std::vector<Fp>& a, bool inverse = false, const Fp* shift = nullptr, int32_t stages = -1) {
  return ntt(std::vector<std::vector<Fp>>{a}, inverse, shift, stages)[0];
}
}  // namespace fr
// The transform of fr::ntt with G1 POINTS as elements, on the domain of n = p.size() = 2^log_n points (sylow_hip_g1_ntt_batch_tuned), natural
// order in and out.  forward: out_i = sum_k w_n^(ik) P_k; inverse: out_k = n^-1 sum_i w_n^(-ik) P_i; no coset shift.  inf: the identity flags
// of p (nullptr: none; the pair (0, 1) is the identity with or without its flag); max_blocks >= 1 caps the blocks of a stage launch (the
// points do not depend on it).  Canonical affine words out, an identity as (0, 1) with its flag in inf_out.
inline std::vector<G1Affine> g1_ntt(const std::vector<G1Affine>& p, bool inverse = false, const std::vector<uint8_t>* inf = nullptr,
                                    std::vector<uint8_t>* inf_out = nullptr, int64_t max_blocks = -1) {
  const size_t n = p.size();
  int32_t log_n = 0;
  while (((size_t)1 << log_n) < n) ++log_n;
  if (!n || n != (size_t)1 << log_n) throw Error("g1_ntt: the length is a power of two");
  auto dp = to_device_soa(p);
  Flags f(inf, n);
  DeviceBuffer dout(n * sizeof(G1Affine) + 8), dinf(n + 8);
  check(sylow_hip_g1_ntt_batch_tuned(dp.as<uint64_t>(), f.ptr, log_n, 1, inverse ? 1 : 0, max_blocks, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr),
        "sylow_hip_g1_ntt_batch_tuned");
  fetch_flags(inf_out, dinf, n);
  return from_device_soa<G1Affine>(dout, n);
}
// sum_i k[j][i] * P[j][i] per job (examples/threshold_signing.rs:124-143); rows term-major: row i*n_jobs + j
inline std::vector<G1Affine> aggregate(const std::vector<G1Affine>& p, const std::vector<Fp>& k, size_t n_jobs, size_t n_terms) {
  if (p.size() != n_jobs * n_terms || k.size() != p.size()) throw Error("aggregate: shape mismatch");
  auto dp = to_device_soa(p); auto dk = to_device_soa(k);
  DeviceBuffer dout(n_jobs * sizeof(G1Affine) + 8), dinf(n_jobs + 8);
  check(sylow_hip_g1_lincomb_batch(dp.as<uint64_t>(), nullptr, dk.as<uint64_t>(), dout.as<uint64_t>(), dinf.as<uint8_t>(), n_jobs, n_terms, nullptr), "sylow_hip_g1_lincomb_batch");
  return from_device_soa<G1Affine>(dout, n_jobs);
}
// sum_i k[i] * P[i] as one point by the bucket method (sylow_hip_g1_msm); *infinity (if given) receives the identity flag.
// Same point as aggregate(p, k, 1, p.size()).
// window / min_n >= 0 pin the plan (sylow_hip_g1_msm_tuned); the point does not depend on them.
inline G1Affine msm(const std::vector<G1Affine>& p, const std::vector<Fp>& k, bool* infinity = nullptr, int32_t window = -1, int64_t min_n = -1) {
  if (k.size() != p.size()) throw Error("msm: shape mismatch");
  auto dp = to_device_soa(p); auto dk = to_device_soa(k);
  DeviceBuffer dout(sizeof(G1Affine) + 8), dinf(8);
  check(sylow_hip_g1_msm_tuned(dp.as<uint64_t>(), nullptr, dk.as<uint64_t>(), p.size(), window, min_n, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr),
        "sylow_hip_g1_msm_tuned");
  uint8_t flag = 0;
  check(sylow_hip_memcpy_d2h(&flag, dinf.as<void>(), 1, nullptr), "d2h");
  const G1Affine r = from_device_soa<G1Affine>(dout, 1)[0];       // synchronises the stream
  if (infinity) *infinity = flag != 0;
  return r;
}
// The G2 twins (public keys), under names of their own so that msm({}, {}) stays unambiguous: k is an Fp value and the products are exact on the whole twist, as sylow_hip_g2_scalar_mul_batch.
inline std::vector<G2Affine> g2_aggregate(const std::vector<G2Affine>& p, const std::vector<Fp>& k, size_t n_jobs, size_t n_terms) {
  if (p.size() != n_jobs * n_terms || k.size() != p.size()) throw Error("aggregate: shape mismatch");
  auto dp = to_device_soa(p); auto dk = to_device_soa(k);
  DeviceBuffer dout(n_jobs * sizeof(G2Affine) + 8), dinf(n_jobs + 8);
  check(sylow_hip_g2_lincomb_batch(dp.as<uint64_t>(), nullptr, dk.as<uint64_t>(), dout.as<uint64_t>(), dinf.as<uint8_t>(), n_jobs, n_terms, nullptr), "sylow_hip_g2_lincomb_batch");
  return from_device_soa<G2Affine>(dout, n_jobs);
}
// sum_i k[i] * Q[i] as one G2 point by the bucket method (sylow_hip_g2_msm_tuned); same point as g2_aggregate(p, k, 1, p.size())
inline G2Affine g2_msm(const std::vector<G2Affine>& p, const std::vector<Fp>& k, bool* infinity = nullptr, int32_t window = -1, int64_t min_n = -1) {
  if (k.size() != p.size()) throw Error("msm: shape mismatch");
  auto dp = to_device_soa(p); auto dk = to_device_soa(k);
  DeviceBuffer dout(sizeof(G2Affine) + 8), dinf(8);
  check(sylow_hip_g2_msm_tuned(dp.as<uint64_t>(), nullptr, dk.as<uint64_t>(), p.size(), window, min_n, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr),
        "sylow_hip_g2_msm_tuned");
  uint8_t flag = 0;
  check(sylow_hip_memcpy_d2h(&flag, dinf.as<void>(), 1, nullptr), "d2h");
  const G2Affine r = from_device_soa<G2Affine>(dout, 1)[0];       // synchronises the stream
  if (infinity) *infinity = flag != 0;
  return r;
}
// sum_i Q[i] as one G2 point (sylow_hip_g2_sum_batch): the `+` fold over public keys
inline G2Affine g2_sum(const std::vector<G2Affine>& q, bool* infinity = nullptr) {
  auto dq = to_device_soa(q);
  DeviceBuffer dout(sizeof(G2Affine) + 8), dinf(8);
  check(sylow_hip_g2_sum_batch(dq.as<uint64_t>(), nullptr, q.size(), dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr), "sylow_hip_g2_sum_batch");
  uint8_t flag = 0;
  check(sylow_hip_memcpy_d2h(&flag, dinf.as<void>(), 1, nullptr), "d2h");
  const G2Affine r = from_device_soa<G2Affine>(dout, 1)[0];       // synchronises the stream
  if (infinity) *infinity = flag != 0;
  return r;
}
struct Messages {                                    // concatenated bytes + offsets on the device
  DeviceBuffer bytes, offsets; size_t n;
  explicit Messages(const std::vector<std::vector<uint8_t>>& msgs) : bytes(total(msgs) + 8), offsets((msgs.size() + 1) * 8), n(msgs.size()) {
    std::vector<uint8_t> blob; std::vector<uint64_t> off(1, 0);
    for (auto& m : msgs) { blob.insert(blob.end(), m.begin(), m.end()); off.push_back(blob.size()); }
    if (!blob.empty()) check(sylow_hip_memcpy_h2d(bytes.as<void>(), blob.data(), blob.size(), nullptr), "h2d");
    check(sylow_hip_memcpy_h2d(offsets.as<void>(), off.data(), off.size() * 8, nullptr), "h2d");
    check(sylow_hip_stream_sync(nullptr), "sync");
  }
  static size_t total(const std::vector<std::vector<uint8_t>>& msgs) { size_t t = 0; for (auto& m : msgs) t += m.size(); return t; }
};
// sign(&Fp, &[u8]) -> Result<G1Projective, GroupError> (lib.rs:179-187), elementwise; sig_inf receives the identity flags of
// the signatures (k = 0 or a multiple of r signs to the identity)
inline std::vector<G1Affine> sign(const std::vector<Fp>& k, const std::vector<std::vector<uint8_t>>& msgs, std::vector<uint8_t>* sig_inf = nullptr) {
  if (k.size() != msgs.size()) throw Error("sign: length mismatch");
  Messages m(msgs);
  auto dk = to_device_soa(k);
  DeviceBuffer dsig(m.n * sizeof(G1Affine) + 8), dinf(m.n + 8);
  check(sylow_hip_bls_sign_batch(dk.as<uint64_t>(), m.bytes.as<uint8_t>(), m.offsets.as<uint64_t>(), dsig.as<uint64_t>(), dinf.as<uint8_t>(), m.n, nullptr), "sylow_hip_bls_sign_batch");
  fetch_flags(sig_inf, dinf, m.n);
  return from_device_soa<G1Affine>(dsig, m.n);
}
// verify(&G2Projective, &[u8], &G1Projective) -> Result<bool, GroupError> (lib.rs:223-236), elementwise.  An identity key or
// signature is a flag, not a coordinate pair: pairing() maps it to Gt::identity() (pairing.rs:876-886)
inline std::vector<uint8_t> verify(const std::vector<G2Affine>& pubkey, const std::vector<std::vector<uint8_t>>& msgs, const std::vector<G1Affine>& sig,
                                   const std::vector<uint8_t>* pk_inf = nullptr, const std::vector<uint8_t>* sig_inf = nullptr) {
  if (pubkey.size() != msgs.size() || sig.size() != msgs.size()) throw Error("verify: length mismatch");
  const size_t n = msgs.size();
  if ((pk_inf && pk_inf->size() != n) || (sig_inf && sig_inf->size() != n)) throw Error("identity flags: length mismatch");
  std::vector<uint8_t> blob; std::vector<uint64_t> off(1, 0);
  for (auto& m : msgs) { blob.insert(blob.end(), m.begin(), m.end()); off.push_back(blob.size()); }
  if (blob.empty()) blob.push_back(0);
  std::vector<uint8_t> ok(n);
  check(sylow_hip_bls_verify_host(reinterpret_cast<const uint64_t*>(pubkey.data()), pk_inf ? pk_inf->data() : nullptr, blob.data(), off.data(),
                                  reinterpret_cast<const uint64_t*>(sig.data()), sig_inf ? sig_inf->data() : nullptr, ok.data(), n, 0), "sylow_hip_bls_verify_host");
  return ok;
}
inline std::vector<uint8_t> verify_unpipelined(const std::vector<G2Affine>& pubkey, const std::vector<std::vector<uint8_t>>& msgs, const std::vector<G1Affine>& sig,
                                               const std::vector<uint8_t>* pk_inf = nullptr, const std::vector<uint8_t>* sig_inf = nullptr) {
  if (pubkey.size() != msgs.size() || sig.size() != msgs.size()) throw Error("verify: length mismatch");
  Messages m(msgs);
  auto dpk = to_device_soa(pubkey); auto dsig = to_device_soa(sig);
  Flags dpi(pk_inf, m.n), dsi(sig_inf, m.n);
  DeviceBuffer dok(m.n + 8);
  check(sylow_hip_bls_verify_batch(dpk.as<uint64_t>(), dpi.ptr, m.bytes.as<uint8_t>(), m.offsets.as<uint64_t>(), dsig.as<uint64_t>(), dsi.ptr, dok.as<uint8_t>(), m.n, nullptr), "sylow_hip_bls_verify_batch");
  std::vector<uint8_t> ok(m.n);
  if (m.n) { check(sylow_hip_memcpy_d2h(ok.data(), dok.as<void>(), m.n, nullptr), "d2h"); check(sylow_hip_stream_sync(nullptr), "sync"); }
  return ok;
}
// page-locked host storage for the pipeline's staging side (every copy asynchronous): a minimal allocator for std::vector
template <class T> struct PinnedAllocator {
  using value_type = T;
  PinnedAllocator() = default;
  template <class U> PinnedAllocator(const PinnedAllocator<U>&) {}
  T* allocate(size_t n) { void* p = nullptr; check(sylow_hip_host_malloc(&p, n * sizeof(T)), "sylow_hip_host_malloc"); return static_cast<T*>(p); }
  void deallocate(T* p, size_t) { sylow_hip_host_free(p); }
  template <class U> bool operator==(const PinnedAllocator<U>&) const { return true; }
  template <class U> bool operator!=(const PinnedAllocator<U>&) const { return false; }
};

// "are ALL of them valid?" as ONE boolean: the glued product of examples/verify_multiple_messages_same_signer.rs:41-60 (weights == nullptr)
// or the sound small-exponent test with the caller's random weights (sylow_hip_bls_batch_verify_weighted).  One key per message, or one key;
// c * n keys: n committees of c keys, term-major (key j belongs to message j mod n, sig[i] is committee i's aggregate signature; summed keys
// presume proofs of possession); n / c keys, at least two: keys reused with that period (signature i is under key i mod pubkey.size()).
inline bool aggregate_shape_ok(size_t n, size_t n_pk) {
  return n == 0 || n_pk == 1 || n_pk == n || (n_pk > n && n_pk % n == 0) || (n_pk >= 2 && n_pk < n && n % n_pk == 0);
}
inline bool verify_all(const std::vector<G2Affine>& pubkey, const std::vector<std::vector<uint8_t>>& msgs, const std::vector<G1Affine>& sig,
                       const std::vector<Fp>* weights = nullptr, Gt* product = nullptr) {
  if (sig.size() != msgs.size() || !aggregate_shape_ok(msgs.size(), pubkey.size())) throw Error("verify_all: length mismatch");
  if (weights && weights->size() != msgs.size()) throw Error("verify_all: one weight per signature");
  Messages m(msgs);
  auto dpk = to_device_soa(pubkey); auto dsig = to_device_soa(sig);
  DeviceBuffer dgt(sizeof(Gt) + 8), done(8);
  if (weights) {
    auto dw = to_device_soa(*weights);
    check(sylow_hip_bls_batch_verify_weighted(dpk.as<uint64_t>(), nullptr, pubkey.size(), m.bytes.as<uint8_t>(), m.offsets.as<uint64_t>(), dsig.as<uint64_t>(), nullptr,
                                              dw.as<uint64_t>(), m.n, nullptr, dgt.as<uint64_t>(), done.as<uint8_t>(), nullptr), "sylow_hip_bls_batch_verify_weighted");
  } else {
    check(sylow_hip_bls_aggregate_verify_batch(dpk.as<uint64_t>(), nullptr, pubkey.size(), m.bytes.as<uint8_t>(), m.offsets.as<uint64_t>(), dsig.as<uint64_t>(), nullptr,
                                               m.n, nullptr, dgt.as<uint64_t>(), done.as<uint8_t>(), nullptr), "sylow_hip_bls_aggregate_verify_batch");
  }
  uint8_t one = 0;
  check(sylow_hip_memcpy_d2h(&one, done.as<void>(), 1, nullptr), "d2h"); check(sylow_hip_stream_sync(nullptr), "sync");
  if (product) *product = from_device_soa<Gt>(dgt, 1)[0];
  return one != 0;
}
// Groth16 on BN254 under ONE verifying key (sylow_hip.h, "Groth16").  The key's points are never the identity, so it carries no flags.
struct Groth16VerifyingKey {
  G1Affine alpha;
  G2Affine beta, gamma, delta;
  std::vector<G1Affine> ic;                       // IC_0 .. IC_l
  size_t n_inputs() const { return ic.size() - 1; }
};
namespace detail {
// inputs[i][j] (proof-major on the host) -> the device's input-major [4][l * n]: input j of proof i at index j * n + i
inline DeviceBuffer groth16_inputs(const std::vector<std::vector<Fp>>& inputs, size_t l) {
  std::vector<Fp> flat(inputs.size() * l);
  for (size_t i = 0; i < inputs.size(); ++i) {
    if (inputs[i].size() != l) throw Error("groth16: every proof takes n_inputs public inputs");
    for (size_t j = 0; j < l; ++j) flat[j * inputs.size() + i] = inputs[i][j];
  }
  return to_device_soa(flat);
}
}  // namespace detail
// the device copies both Groth16 checks take
struct Groth16Device {
  DeviceBuffer alpha, beta, gamma, delta, ic, a, b, c, x;
  size_t n, l;
};
inline Groth16Device groth16_upload(const char* who, const Groth16VerifyingKey& vk, const std::vector<G1Affine>& a, const std::vector<G2Affine>& b,
                                    const std::vector<G1Affine>& c, const std::vector<std::vector<Fp>>& inputs) {
  if (vk.ic.empty()) throw Error(std::string(who) + ": the key holds at least IC_0");
  const size_t n = a.size(), l = vk.n_inputs();
  if (b.size() != n || c.size() != n || inputs.size() != n) throw Error(std::string(who) + ": length mismatch");
  return Groth16Device{to_device_soa(std::vector<G1Affine>{vk.alpha}), to_device_soa(std::vector<G2Affine>{vk.beta}), to_device_soa(std::vector<G2Affine>{vk.gamma}),
                       to_device_soa(std::vector<G2Affine>{vk.delta}), to_device_soa(vk.ic), to_device_soa(a), to_device_soa(b), to_device_soa(c),
                       detail::groth16_inputs(inputs, l), n, l};
}
// ok[i] = [ e(-A_i, B_i) e(alpha, beta) e(IC_0 + sum_j x_ij IC_j, gamma) e(C_i, delta) == 1 ]; inputs are any 256-bit words, taken mod r.
// Points are taken as given: B and the key's G2 points must lie in G2 proper.
inline std::vector<uint8_t> groth16_verify(const Groth16VerifyingKey& vk, const std::vector<G1Affine>& a, const std::vector<G2Affine>& b,
                                           const std::vector<G1Affine>& c, const std::vector<std::vector<Fp>>& inputs) {
  Groth16Device d = groth16_upload("groth16_verify", vk, a, b, c, inputs);
  std::vector<uint8_t> ok(d.n);
  DeviceBuffer dok(d.n + 8);
  check(sylow_hip_groth16_verify_batch(d.alpha.as<uint64_t>(), d.beta.as<uint64_t>(), d.gamma.as<uint64_t>(), d.delta.as<uint64_t>(), d.ic.as<uint64_t>(), d.l,
                                       d.a.as<uint64_t>(), nullptr, d.b.as<uint64_t>(), nullptr, d.c.as<uint64_t>(), nullptr, d.x.as<uint64_t>(), d.n, dok.as<uint8_t>(),
                                       nullptr), "sylow_hip_groth16_verify_batch");
  if (d.n) check(sylow_hip_memcpy_d2h(ok.data(), dok.as<void>(), d.n, nullptr), "d2h");
  check(sylow_hip_stream_sync(nullptr), "sync");
  return ok;
}
// "are ALL of them valid?" as ONE boolean, the sound small-exponent test (sylow_hip_groth16_batch_verify_weighted): one weight per proof, drawn
// AFTER the proofs are fixed; a batch with an invalid proof passes with probability at most 2^-(bits of the weights).  Like verify_all.
inline bool groth16_verify_all(const Groth16VerifyingKey& vk, const std::vector<G1Affine>& a, const std::vector<G2Affine>& b, const std::vector<G1Affine>& c,
                               const std::vector<std::vector<Fp>>& inputs, const std::vector<Fp>& weights, Gt* product = nullptr) {
  Groth16Device d = groth16_upload("groth16_verify_all", vk, a, b, c, inputs);
  if (weights.size() != d.n) throw Error("groth16_verify_all: one weight per proof");
  auto dw = to_device_soa(weights);
  DeviceBuffer dgt(sizeof(Gt) + 8), done(8);
  check(sylow_hip_groth16_batch_verify_weighted(d.alpha.as<uint64_t>(), d.beta.as<uint64_t>(), d.gamma.as<uint64_t>(), d.delta.as<uint64_t>(), d.ic.as<uint64_t>(), d.l,
                                                d.a.as<uint64_t>(), nullptr, d.b.as<uint64_t>(), nullptr, d.c.as<uint64_t>(), nullptr, d.x.as<uint64_t>(), dw.as<uint64_t>(),
                                                d.n, dgt.as<uint64_t>(), done.as<uint8_t>(), nullptr), "sylow_hip_groth16_batch_verify_weighted");
  uint8_t one = 0;
  check(sylow_hip_memcpy_d2h(&one, done.as<void>(), 1, nullptr), "d2h"); check(sylow_hip_stream_sync(nullptr), "sync");
  if (product) *product = from_device_soa<Gt>(dgt, 1)[0];
  return one != 0;
}
// vk_x_i = IC_0 + sum_j x_ij IC_j for every proof (sylow_hip_groth16_vk_x_batch); *infinity (if given) receives the identity flags
inline std::vector<G1Affine> groth16_vk_x(const std::vector<G1Affine>& ic, const std::vector<std::vector<Fp>>& inputs, std::vector<uint8_t>* infinity = nullptr) {
  if (ic.empty()) throw Error("groth16_vk_x: ic holds at least IC_0");
  const size_t n = inputs.size(), l = ic.size() - 1;
  auto dic = to_device_soa(ic);
  auto dx = detail::groth16_inputs(inputs, l);
  DeviceBuffer dout(n * sizeof(G1Affine) + 8), dinf(n + 8);
  check(sylow_hip_groth16_vk_x_batch(dic.as<uint64_t>(), l, dx.as<uint64_t>(), n, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr), "sylow_hip_groth16_vk_x_batch");
  if (infinity) {
    infinity->assign(n, 0);
    if (n) check(sylow_hip_memcpy_d2h(infinity->data(), dinf.as<void>(), n, nullptr), "d2h");
  }
  return from_device_soa<G1Affine>(dout, n);
}
// KZG openings on BN254 under ONE SRS (sylow_hip.h, "KZG"): F = C - y G1gen + z pi, ok = [ e(F, G2gen) e(-pi, tau_g2) == 1 ].  z and y are any
// 256-bit words, taken mod r (carried in the Fp container, as the Groth16 inputs).  Points are taken as given.
struct KzgOpenings {
  std::vector<G1Affine> c, pi;
  std::vector<Fp> z, y;
};
namespace detail {
struct KzgDevice {
  DeviceBuffer c, z, y, pi;
  size_t n;
};
inline KzgDevice kzg_upload(const char* who, const KzgOpenings& o) {
  const size_t n = o.c.size();
  if (o.pi.size() != n || o.z.size() != n || o.y.size() != n) throw Error(std::string(who) + ": length mismatch");
  return KzgDevice{to_device_soa(o.c), to_device_soa(o.z), to_device_soa(o.y), to_device_soa(o.pi), n};
}
}  // namespace detail
// F_i for every opening (sylow_hip_kzg_fold_batch); *infinity (if given) receives the identity flags
inline std::vector<G1Affine> kzg_fold(const KzgOpenings& o, std::vector<uint8_t>* infinity = nullptr) {
  detail::KzgDevice d = detail::kzg_upload("kzg_fold", o);
  DeviceBuffer dout(d.n * sizeof(G1Affine) + 8), dinf(d.n + 8);
  check(sylow_hip_kzg_fold_batch(d.c.as<uint64_t>(), nullptr, d.z.as<uint64_t>(), d.y.as<uint64_t>(), d.pi.as<uint64_t>(), nullptr, dout.as<uint64_t>(),
                                 dinf.as<uint8_t>(), d.n, nullptr), "sylow_hip_kzg_fold_batch");
  if (infinity) {
    infinity->assign(d.n, 0);
    if (d.n) check(sylow_hip_memcpy_d2h(infinity->data(), dinf.as<void>(), d.n, nullptr), "d2h");
  }
  return from_device_soa<G1Affine>(dout, d.n);
}
// The verifier's half of the SRS: tau_g2 = tau G2gen (G2 proper, not the identity) and its line table, built once and kept on the device.
class KzgVerifier {
 public:
  explicit KzgVerifier(const G2Affine& tau_g2) : tau_(to_device_soa(std::vector<G2Affine>{tau_g2})), table_((size_t)sylow_hip_g2_line_table_words() * sizeof(int32_t) + 8) {
    check(sylow_hip_g2_line_table(tau_.as<uint64_t>(), 1, 0, table_.as<int32_t>(), nullptr), "sylow_hip_g2_line_table");
    check(sylow_hip_stream_sync(nullptr), "sync");
  }
  // ok[i] for every opening (sylow_hip_kzg_verify_line_table_batch against the cached table)
  std::vector<uint8_t> verify(const KzgOpenings& o) const {
    detail::KzgDevice d = detail::kzg_upload("KzgVerifier::verify", o);
    std::vector<uint8_t> ok(d.n);
    DeviceBuffer dok(d.n + 8);
    check(sylow_hip_kzg_verify_line_table_batch(table_.as<int32_t>(), d.c.as<uint64_t>(), nullptr, d.z.as<uint64_t>(), d.y.as<uint64_t>(), d.pi.as<uint64_t>(), nullptr,
                                                dok.as<uint8_t>(), d.n, nullptr), "sylow_hip_kzg_verify_line_table_batch");
    if (d.n) check(sylow_hip_memcpy_d2h(ok.data(), dok.as<void>(), d.n, nullptr), "d2h");
    check(sylow_hip_stream_sync(nullptr), "sync");
    return ok;
  }
  // "are ALL of them valid?" as ONE boolean, the sound small-exponent test (sylow_hip_kzg_batch_verify_weighted): one weight per opening, drawn
  // AFTER the openings are fixed; a batch with an invalid opening passes with probability at most 2^-(bits of the weights).  Like verify_all.
  bool verify_all(const KzgOpenings& o, const std::vector<Fp>& weights, Gt* product = nullptr) const {
    detail::KzgDevice d = detail::kzg_upload("KzgVerifier::verify_all", o);
    if (weights.size() != d.n) throw Error("KzgVerifier::verify_all: one weight per opening");
    auto dw = to_device_soa(weights);
    DeviceBuffer dgt(sizeof(Gt) + 8), done(8);
    check(sylow_hip_kzg_batch_verify_weighted(tau_.as<uint64_t>(), d.c.as<uint64_t>(), nullptr, d.z.as<uint64_t>(), d.y.as<uint64_t>(), d.pi.as<uint64_t>(), nullptr,
                                              dw.as<uint64_t>(), d.n, dgt.as<uint64_t>(), done.as<uint8_t>(), nullptr), "sylow_hip_kzg_batch_verify_weighted");
    uint8_t one = 0;
    check(sylow_hip_memcpy_d2h(&one, done.as<void>(), 1, nullptr), "d2h"); check(sylow_hip_stream_sync(nullptr), "sync");
    if (product) *product = from_device_soa<Gt>(dgt, 1)[0];
    return one != 0;
  }
  // the same check with the table built inside the call (sylow_hip_kzg_verify_batch): what a one-shot caller without this holder would make
  std::vector<uint8_t> verify_uncached(const KzgOpenings& o) const {
    detail::KzgDevice d = detail::kzg_upload("KzgVerifier::verify_uncached", o);
    std::vector<uint8_t> ok(d.n);
    DeviceBuffer dok(d.n + 8);
    check(sylow_hip_kzg_verify_batch(tau_.as<uint64_t>(), d.c.as<uint64_t>(), nullptr, d.z.as<uint64_t>(), d.y.as<uint64_t>(), d.pi.as<uint64_t>(), nullptr,
                                     dok.as<uint8_t>(), d.n, nullptr), "sylow_hip_kzg_verify_batch");
    if (d.n) check(sylow_hip_memcpy_d2h(ok.data(), dok.as<void>(), d.n, nullptr), "d2h");
    check(sylow_hip_stream_sync(nullptr), "sync");
    return ok;
  }

 private:
  DeviceBuffer tau_, table_;
};
// The prover's half of the SRS (sylow_hip.h, "KZG, the prover's side"): srs_g1[k] = tau^k G1gen, kept on the device.  A polynomial is its
// coefficients, lowest degree first -- any 256-bit words, taken mod r -- padded with zeros by the caller to the length of the SRS.
class KzgProver {
 public:
  explicit KzgProver(const std::vector<G1Affine>& srs_g1) : len_(srs_g1.size()), srs_(to_device_soa(srs_g1)) {
    if (!len_) throw Error("KzgProver: the SRS holds at least G1gen");
  }
  size_t len() const { return len_; }
  // C_j = sum_k polys[j][k] srs_g1[k] (sylow_hip_kzg_commit_batch_tuned; window / min_len < 0 = the defaults, the points do not depend on them);
  // *infinity (if given) receives the identity flags (the zero polynomial)
  std::vector<G1Affine> commit(const std::vector<std::vector<Fp>>& polys, std::vector<uint8_t>* infinity = nullptr, int32_t window = -1, int64_t min_len = -1) const {
    const size_t m = polys.size();
    DeviceBuffer dc = upload("KzgProver::commit", polys);
    DeviceBuffer dout(m * sizeof(G1Affine) + 8), dinf(m + 8);
    check(sylow_hip_kzg_commit_batch_tuned(srs_.as<uint64_t>(), dc.as<uint64_t>(), len_, m, window, min_len, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr),
          "sylow_hip_kzg_commit_batch_tuned");
    fetch_flags(infinity, dinf, m);
    return from_device_soa<G1Affine>(dout, m);
  }
  // The same commitments from the VALUES evals[j][i] = f_j(w_n^i) on the domain of len() = 2^log_n points (sylow_hip_kzg_commit_evals_batch):
  // word for word commit(fr::ntt(evals, /*inverse=*/true))
  std::vector<G1Affine> commit_evals(const std::vector<std::vector<Fp>>& evals, std::vector<uint8_t>* infinity = nullptr) const {
    const size_t m = evals.size();
    int32_t log_n = 0;
    while (((size_t)1 << log_n) < len_) ++log_n;
    if (len_ != (size_t)1 << log_n) throw Error("KzgProver::commit_evals: the SRS holds a power of two of points");
    DeviceBuffer dc = upload("KzgProver::commit_evals", evals);
    DeviceBuffer dout(m * sizeof(G1Affine) + 8), dinf(m + 8);
    check(sylow_hip_kzg_commit_evals_batch(srs_.as<uint64_t>(), dc.as<uint64_t>(), log_n, m, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr),
          "sylow_hip_kzg_commit_evals_batch");
    fetch_flags(infinity, dinf, m);
    return from_device_soa<G1Affine>(dout, m);
  }
  // y_j = f_j(z_j) and pi_j = commit((f_j - y_j) / (X - z_j)) (sylow_hip_kzg_open_batch); a flagged pi_j is the proof for a constant polynomial
  std::vector<G1Affine> open(const std::vector<std::vector<Fp>>& polys, const std::vector<Fp>& z, std::vector<Fp>* y, std::vector<uint8_t>* infinity = nullptr) const {
    const size_t m = polys.size();
    if (z.size() != m) throw Error("KzgProver::open: one point per polynomial");
    DeviceBuffer dc = upload("KzgProver::open", polys);
    auto dz = to_device_soa(z);
    DeviceBuffer dy(m * sizeof(Fp) + 8), dpi(m * sizeof(G1Affine) + 8), dinf(m + 8);
    check(sylow_hip_kzg_open_batch(srs_.as<uint64_t>(), dc.as<uint64_t>(), len_, m, dz.as<uint64_t>(), dy.as<uint64_t>(), dpi.as<uint64_t>(), dinf.as<uint8_t>(), nullptr),
          "sylow_hip_kzg_open_batch");
    fetch_flags(infinity, dinf, m);
    if (y) *y = from_device_soa<Fp>(dy, m);
    return from_device_soa<G1Affine>(dpi, m);
  }
  // The Lagrange-basis SRS L_i(tau) G1gen of the domain of len() = 2^log_n points (sylow_hip_kzg_srs_lagrange): what KzgEvalProver takes.
  // Throws when tau lies in the domain (an identity comes back: some L_i(tau) = 0).
  std::vector<G1Affine> lagrange_srs() const {
    int32_t log_n = 0;
    while (((size_t)1 << log_n) < len_) ++log_n;
    if (len_ != (size_t)1 << log_n || log_n > 28) throw Error("KzgProver::lagrange_srs: the SRS holds a power of two of points, at most 2^28");
    DeviceBuffer dout(len_ * sizeof(G1Affine) + 8), dinf(len_ + 8);
    check(sylow_hip_kzg_srs_lagrange(srs_.as<uint64_t>(), log_n, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr), "sylow_hip_kzg_srs_lagrange");
    std::vector<uint8_t> inf;
    fetch_flags(&inf, dinf, len_);
    for (const uint8_t f : inf) if (f) throw Error("KzgProver::lagrange_srs: tau lies in the domain, the Lagrange-basis SRS is unusable");
    return from_device_soa<G1Affine>(dout, len_);
  }
  // The proofs of every f_j at ALL len() = 2^log_n points w_n^i of its domain at once, in n log n (sylow_hip_kzg_open_all_batch_tuned, the
  // Feist-Khovratovich construction): pi[j][i], word for word open(f_j, w_n^i); *y (if given) receives y[j][i] = f_j(w_n^i) = fr::ntt(polys)
  // and *infinity the identity flags per polynomial (every proof of a constant polynomial).  The table that depends on the SRS alone
  // (sylow_hip_kzg_open_all_prepare) is built on first use and kept on the device.  max_blocks >= 1 caps the blocks of a multiplying launch;
  // the values do not depend on it.
  std::vector<std::vector<G1Affine>> open_all(const std::vector<std::vector<Fp>>& polys, std::vector<std::vector<Fp>>* y = nullptr,
                                              std::vector<std::vector<uint8_t>>* infinity = nullptr, int64_t max_blocks = -1) const {
    const size_t m = polys.size(), n = len_;
    int32_t log_n = 0;
    while (((size_t)1 << log_n) < n) ++log_n;
    if (n != (size_t)1 << log_n || log_n > 27) throw Error("KzgProver::open_all: the SRS holds a power of two of points, at most 2^27");
    if (!all_xy_) {
      std::unique_ptr<DeviceBuffer> txy(new DeviceBuffer(2 * n * sizeof(G1Affine) + 8)), tinf(new DeviceBuffer(2 * n + 8));
      check(sylow_hip_kzg_open_all_prepare(srs_.as<uint64_t>(), log_n, txy->as<uint64_t>(), tinf->as<uint8_t>(), nullptr), "sylow_hip_kzg_open_all_prepare");
      all_xy_ = std::move(txy);
      all_inf_ = std::move(tinf);
    }
    DeviceBuffer dc = upload("KzgProver::open_all", polys);
    DeviceBuffer dy(4 * n * m * sizeof(uint64_t) + 8), dpi(8 * n * m * sizeof(uint64_t) + 8), dinf(n * m + 8);
    check(sylow_hip_kzg_open_all_batch_tuned(all_xy_->as<uint64_t>(), all_inf_->as<uint8_t>(), dc.as<uint64_t>(), log_n, m, max_blocks, dy.as<uint64_t>(),
                                             dpi.as<uint64_t>(), dinf.as<uint8_t>(), nullptr), "sylow_hip_kzg_open_all_batch_tuned");
    std::vector<uint64_t> fy(4 * n * m), fp(8 * n * m);
    std::vector<uint8_t> fi(n * m);
    if (m) {
      check(sylow_hip_memcpy_d2h(fy.data(), dy.as<void>(), fy.size() * sizeof(uint64_t), nullptr), "d2h");
      check(sylow_hip_memcpy_d2h(fp.data(), dpi.as<void>(), fp.size() * sizeof(uint64_t), nullptr), "d2h");
      check(sylow_hip_memcpy_d2h(fi.data(), dinf.as<void>(), fi.size(), nullptr), "d2h");
    }
    check(sylow_hip_stream_sync(nullptr), "sync");
    std::vector<std::vector<G1Affine>> pi(m, std::vector<G1Affine>(n));
    if (y) y->assign(m, std::vector<Fp>(n));
    if (infinity) infinity->assign(m, std::vector<uint8_t>(n));
    for (size_t j = 0; j < m; ++j)
      for (size_t k = 0; k < n; ++k) {
        for (size_t w = 0; w < 4; ++w) {
          pi[j][k].x.w[w] = fp[(j * 8 + w) * n + k];
          pi[j][k].y.w[w] = fp[(j * 8 + 4 + w) * n + k];
          if (y) (*y)[j][k].w[w] = fy[(j * 4 + w) * n + k];
        }
        if (infinity) (*infinity)[j][k] = fi[j * n + k];
      }
    return pi;
  }
  // q_j = (f_j - f_j(z_j)) / (X - z_j), canonical words, q_j[len - 1] = 0, and y_j (sylow_hip_kzg_quotient_batch)
  std::vector<std::vector<Fp>> quotient(const std::vector<std::vector<Fp>>& polys, const std::vector<Fp>& z, std::vector<Fp>* y = nullptr) const {
    const size_t m = polys.size();
    if (z.size() != m) throw Error("KzgProver::quotient: one point per polynomial");
    DeviceBuffer dc = upload("KzgProver::quotient", polys);
    auto dz = to_device_soa(z);
    DeviceBuffer dq(4 * len_ * m * sizeof(uint64_t) + 8), dy(m * sizeof(Fp) + 8);
    check(sylow_hip_kzg_quotient_batch(dc.as<uint64_t>(), len_, m, dz.as<uint64_t>(), dq.as<uint64_t>(), dy.as<uint64_t>(), nullptr), "sylow_hip_kzg_quotient_batch");
    std::vector<uint64_t> flat(4 * len_ * m);
    if (m) check(sylow_hip_memcpy_d2h(flat.data(), dq.as<void>(), flat.size() * sizeof(uint64_t), nullptr), "d2h");
    check(sylow_hip_stream_sync(nullptr), "sync");
    std::vector<std::vector<Fp>> q(m, std::vector<Fp>(len_));
    for (size_t j = 0; j < m; ++j) for (size_t k = 0; k < len_; ++k) for (size_t w = 0; w < 4; ++w) q[j][k].w[w] = flat[(j * 4 + w) * len_ + k];
    if (y) *y = from_device_soa<Fp>(dy, m);
    return q;
  }

 private:
  // the block layout of the prover's calls: word w of coefficient k of polynomial j at (j * 4 + w) * len + k
  DeviceBuffer upload(const char* who, const std::vector<std::vector<Fp>>& polys) const {
    const size_t m = polys.size();
    std::vector<uint64_t> flat(4 * len_ * m);
    for (size_t j = 0; j < m; ++j) {
      if (polys[j].size() != len_) throw Error(std::string(who) + ": every polynomial has one coefficient per SRS point (pad with zeros)");
      for (size_t k = 0; k < len_; ++k) for (size_t w = 0; w < 4; ++w) flat[(j * 4 + w) * len_ + k] = polys[j][k].w[w];
    }
    DeviceBuffer d(flat.size() * sizeof(uint64_t) + 8);
    if (m) { check(sylow_hip_memcpy_h2d(d.as<void>(), flat.data(), flat.size() * sizeof(uint64_t), nullptr), "h2d"); check(sylow_hip_stream_sync(nullptr), "sync"); }
    return d;
  }
  size_t len_;
  DeviceBuffer srs_;
  mutable std::unique_ptr<DeviceBuffer> all_xy_, all_inf_;      // open_all's table [8][2 len] + [2 len], built on first use
};
// The prover's half of the SRS for polynomials held in EVALUATION form (sylow_hip.h, "KZG, the prover's side, from evaluations"):
// srs_lagrange[i] = L_i(tau) G1gen for the Lagrange basis of the domain of n = 2^log_n points, kept on the device.  A polynomial is its
// values evals[i] = f(w_n^i), natural order -- any 256-bit words, taken mod r.  z may lie inside the domain.
class KzgEvalProver {
 public:
  explicit KzgEvalProver(const std::vector<G1Affine>& srs_lagrange) : n_(srs_lagrange.size()), log_n_(0), srs_(to_device_soa(srs_lagrange)) {
    while (((size_t)1 << log_n_) < n_) ++log_n_;
    if (!n_ || n_ != (size_t)1 << log_n_ || log_n_ > 28) throw Error("KzgEvalProver: the SRS holds a power of two of points, at most 2^28");
  }
  size_t len() const { return n_; }
  // C_j = sum_i evals[j][i] srs_lagrange[i] = f_j(tau) G1gen: sylow_hip_kzg_commit_batch over the values as they lie
  std::vector<G1Affine> commit(const std::vector<std::vector<Fp>>& evals, std::vector<uint8_t>* infinity = nullptr) const {
    const size_t m = evals.size();
    DeviceBuffer dc = upload("KzgEvalProver::commit", evals);
    DeviceBuffer dout(m * sizeof(G1Affine) + 8), dinf(m + 8);
    check(sylow_hip_kzg_commit_batch(srs_.as<uint64_t>(), dc.as<uint64_t>(), n_, m, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr), "sylow_hip_kzg_commit_batch");
    fetch_flags(infinity, dinf, m);
    return from_device_soa<G1Affine>(dout, m);
  }
  // y_j = f_j(z_j) by the barycentric formula (sylow_hip_kzg_quotient_evals_batch without a quotient buffer)
  std::vector<Fp> evaluate(const std::vector<std::vector<Fp>>& evals, const std::vector<Fp>& z) const {
    const size_t m = evals.size();
    if (z.size() != m) throw Error("KzgEvalProver::evaluate: one point per polynomial");
    DeviceBuffer dc = upload("KzgEvalProver::evaluate", evals);
    auto dz = to_device_soa(z);
    DeviceBuffer dy(m * sizeof(Fp) + 8);
    check(sylow_hip_kzg_quotient_evals_batch(dc.as<uint64_t>(), log_n_, m, dz.as<uint64_t>(), nullptr, dy.as<uint64_t>(), nullptr), "sylow_hip_kzg_quotient_evals_batch");
    return from_device_soa<Fp>(dy, m);
  }
  // the values on the domain of q_j = (f_j - y_j) / (X - z_j), canonical words, and y_j (sylow_hip_kzg_quotient_evals_batch)
  std::vector<std::vector<Fp>> quotient(const std::vector<std::vector<Fp>>& evals, const std::vector<Fp>& z, std::vector<Fp>* y = nullptr) const {
    const size_t m = evals.size();
    if (z.size() != m) throw Error("KzgEvalProver::quotient: one point per polynomial");
    DeviceBuffer dc = upload("KzgEvalProver::quotient", evals);
    auto dz = to_device_soa(z);
    DeviceBuffer dq(4 * n_ * m * sizeof(uint64_t) + 8), dy(m * sizeof(Fp) + 8);
    check(sylow_hip_kzg_quotient_evals_batch(dc.as<uint64_t>(), log_n_, m, dz.as<uint64_t>(), dq.as<uint64_t>(), dy.as<uint64_t>(), nullptr),
          "sylow_hip_kzg_quotient_evals_batch");
    std::vector<uint64_t> flat(4 * n_ * m);
    if (m) check(sylow_hip_memcpy_d2h(flat.data(), dq.as<void>(), flat.size() * sizeof(uint64_t), nullptr), "d2h");
    check(sylow_hip_stream_sync(nullptr), "sync");
    std::vector<std::vector<Fp>> q(m, std::vector<Fp>(n_));
    for (size_t j = 0; j < m; ++j) for (size_t k = 0; k < n_; ++k) for (size_t w = 0; w < 4; ++w) q[j][k].w[w] = flat[(j * 4 + w) * n_ + k];
    if (y) *y = from_device_soa<Fp>(dy, m);
    return q;
  }
  // y_j and pi_j = the commitment to the quotient's values (sylow_hip_kzg_open_evals_batch); a flagged pi_j is the proof for a constant polynomial
  std::vector<G1Affine> open(const std::vector<std::vector<Fp>>& evals, const std::vector<Fp>& z, std::vector<Fp>* y, std::vector<uint8_t>* infinity = nullptr) const {
    const size_t m = evals.size();
    if (z.size() != m) throw Error("KzgEvalProver::open: one point per polynomial");
    DeviceBuffer dc = upload("KzgEvalProver::open", evals);
    auto dz = to_device_soa(z);
    DeviceBuffer dy(m * sizeof(Fp) + 8), dpi(m * sizeof(G1Affine) + 8), dinf(m + 8);
    check(sylow_hip_kzg_open_evals_batch(srs_.as<uint64_t>(), dc.as<uint64_t>(), log_n_, m, dz.as<uint64_t>(), dy.as<uint64_t>(), dpi.as<uint64_t>(), dinf.as<uint8_t>(),
                                         nullptr), "sylow_hip_kzg_open_evals_batch");
    fetch_flags(infinity, dinf, m);
    if (y) *y = from_device_soa<Fp>(dy, m);
    return from_device_soa<G1Affine>(dpi, m);
  }

 private:
  // the block layout of the prover's calls: word w of value i of polynomial j at (j * 4 + w) * n + i
  DeviceBuffer upload(const char* who, const std::vector<std::vector<Fp>>& evals) const {
    const size_t m = evals.size();
    std::vector<uint64_t> flat(4 * n_ * m);
    for (size_t j = 0; j < m; ++j) {
      if (evals[j].size() != n_) throw Error(std::string(who) + ": every polynomial has one value per SRS point");
      for (size_t k = 0; k < n_; ++k) for (size_t w = 0; w < 4; ++w) flat[(j * 4 + w) * n_ + k] = evals[j][k].w[w];
    }
    DeviceBuffer d(flat.size() * sizeof(uint64_t) + 8);
    if (m) { check(sylow_hip_memcpy_h2d(d.as<void>(), flat.data(), flat.size() * sizeof(uint64_t), nullptr), "h2d"); check(sylow_hip_stream_sync(nullptr), "sync"); }
    return d;
  }
  size_t n_;
  int32_t log_n_;
  DeviceBuffer srs_;
};
// Many signers, ONE message (examples/threshold_signing.rs:92-121): e(sig, G2gen) e(-H(msg), sum_j pubkeys[j]) == identity -- one hash, one G2
// sum and two Miller loops whatever the number of keys.  `sig` is the signers' aggregate signature (sum() of the individual ones).
inline bool verify_one_message(const std::vector<G2Affine>& pubkeys, const std::vector<uint8_t>& msg, const G1Affine& sig, Gt* product = nullptr) {
  if (pubkeys.empty()) throw Error("verify_one_message: no public keys");
  return verify_all(pubkeys, std::vector<std::vector<uint8_t>>{msg}, std::vector<G1Affine>{sig}, nullptr, product);
}
// sum_i p[i] as ONE point (the `+` fold of examples/verify_multiple_messages_same_signer.rs:41-60); *is_identity receives the flag of the result
inline G1Affine sum(const std::vector<G1Affine>& p, bool* is_identity = nullptr, const std::vector<uint8_t>* p_inf = nullptr) {
  const size_t n = p.size();
  auto dp = to_device_soa(p);
  Flags dpi(p_inf, n);
  DeviceBuffer dout(sizeof(G1Affine) + 8), dinf(8);
  check(sylow_hip_g1_sum_batch(dp.as<uint64_t>(), dpi.ptr, n, dout.as<uint64_t>(), dinf.as<uint8_t>(), nullptr), "sylow_hip_g1_sum_batch");
  std::vector<uint8_t> f;
  fetch_flags(&f, dinf, 1);
  if (is_identity) *is_identity = f[0] != 0;
  return from_device_soa<G1Affine>(dout, 1)[0];
}
// Sub for &G1Projective (group.rs:614-624), elementwise on affine inputs
inline std::vector<G1Affine> sub(const std::vector<G1Affine>& a, const std::vector<G1Affine>& b, std::vector<uint8_t>* inf_out = nullptr) {
  if (a.size() != b.size()) throw Error("G1 - G1: length mismatch");
  const size_t n = a.size();
  auto da = to_device_soa(a); auto db = to_device_soa(b);
  DeviceBuffer dout(n * sizeof(G1Affine) + 8), dinf(n + 8);
  check(sylow_hip_g1_sub_batch(da.as<uint64_t>(), nullptr, db.as<uint64_t>(), nullptr, dout.as<uint64_t>(), dinf.as<uint8_t>(), n, nullptr), "sylow_hip_g1_sub_batch");
  fetch_flags(inf_out, dinf, n);
  return from_device_soa<G1Affine>(dout, n);
}

// ---- Groth16, the prover's side (sylow_hip.h, "Groth16, the prover's side") ----------------------------------------------------------------
// A sparse matrix over Fr in CSR: the entries of row i are col / val [row_ptr[i] .. row_ptr[i + 1])
struct CsrMatrix {
  std::vector<uint64_t> row_ptr{0}, col;
  std::vector<Fp> val;
  size_t rows() const { return row_ptr.size() - 1; }
  void add_row(const std::vector<std::pair<uint64_t, Fp>>& entries) {
    for (const auto& e : entries) { col.push_back(e.first); val.push_back(e.second); }
    row_ptr.push_back(col.size());
  }
};
namespace detail {
// m arrays of n elements <-> the block layout [m][4][n]: word w of element k of array j at (j * 4 + w) * n + k
inline DeviceBuffer fr_arrays_up(const char* who, const std::vector<std::vector<Fp>>& a, size_t n) {
  std::vector<uint64_t> flat(4 * n * a.size());
  for (size_t j = 0; j < a.size(); ++j) {
    if (a[j].size() != n) throw Error(std::string(who) + ": arrays of one length");
    for (size_t k = 0; k < n; ++k) for (size_t w = 0; w < 4; ++w) flat[(j * 4 + w) * n + k] = a[j][k].w[w];
  }
  DeviceBuffer d(flat.size() * sizeof(uint64_t) + 8);
  if (!flat.empty()) { check(sylow_hip_memcpy_h2d(d.as<void>(), flat.data(), flat.size() * sizeof(uint64_t), nullptr), "h2d"); check(sylow_hip_stream_sync(nullptr), "sync"); }
  return d;
}
inline std::vector<std::vector<Fp>> fr_arrays_down(const DeviceBuffer& d, size_t n, size_t m) {
  std::vector<uint64_t> flat(4 * n * m);
  if (!flat.empty()) check(sylow_hip_memcpy_d2h(flat.data(), d.as<void>(), flat.size() * sizeof(uint64_t), nullptr), "d2h");
  check(sylow_hip_stream_sync(nullptr), "sync");
  std::vector<std::vector<Fp>> out(m, std::vector<Fp>(n));
  for (size_t j = 0; j < m; ++j) for (size_t k = 0; k < n; ++k) for (size_t w = 0; w < 4; ++w) out[j][k].w[w] = flat[(j * 4 + w) * n + k];
  return out;
}
struct CsrDevice {
  DeviceBuffer row_ptr, col, val;
  size_t rows, nnz;
};
inline CsrDevice csr_up(const CsrMatrix& m) {
  if (m.row_ptr.empty() || m.col.size() != m.val.size()) throw Error("CsrMatrix: row_ptr holds rows + 1 offsets, col and val one entry each");
  DeviceBuffer rp(m.row_ptr.size() * 8 + 8), col(m.col.size() * 8 + 8);
  check(sylow_hip_memcpy_h2d(rp.as<void>(), m.row_ptr.data(), m.row_ptr.size() * 8, nullptr), "h2d");
  if (!m.col.empty()) check(sylow_hip_memcpy_h2d(col.as<void>(), m.col.data(), m.col.size() * 8, nullptr), "h2d");
  check(sylow_hip_stream_sync(nullptr), "sync");
  return CsrDevice{std::move(rp), std::move(col), to_device_soa(m.val), m.rows(), m.col.size()};
}
}  // namespace detail
namespace fr {
// out[j] = M w[j] for m vectors of one length, padded with zero rows to n_out (0: M.rows()) (sylow_hip_fr_spmv_batch_tuned; lanes_log >= 0 pins
// 2^lanes_log lanes per row, the values do not depend on it).  An entry whose column is past the vectors contributes zero.
inline std::vector<std::vector<Fp>> spmv(const CsrMatrix& mat, const std::vector<std::vector<Fp>>& w, size_t n_out = 0, int32_t lanes_log = -1) {
  const size_t m = w.size(), n_cols = m ? w[0].size() : 0;
  if (!n_out) n_out = mat.rows();
  detail::CsrDevice d = detail::csr_up(mat);
  DeviceBuffer dw = detail::fr_arrays_up("fr::spmv", w, n_cols), dout(4 * n_out * m * sizeof(uint64_t) + 8);
  check(sylow_hip_fr_spmv_batch_tuned(d.row_ptr.as<uint64_t>(), d.col.as<uint64_t>(), d.val.as<uint64_t>(), d.rows, d.nnz, dw.as<uint64_t>(), n_cols, m, n_out, lanes_log,
                                      dout.as<uint64_t>(), nullptr), "sylow_hip_fr_spmv_batch_tuned");
  return detail::fr_arrays_down(dout, n_out, m);
}
}  // namespace fr
// h[j] = the coefficients of the polynomial of degree < n that equals (a[j] b[j] - c[j]) / (X^n - 1) on the coset 5 <w_n>, for the values of three
// polynomials on the domain of n = 2^log_n points (sylow_hip_groth16_quotient_batch); h[j][n - 1] = 0 where a b = c on the whole domain
inline std::vector<std::vector<Fp>> groth16_quotient(const std::vector<std::vector<Fp>>& a, const std::vector<std::vector<Fp>>& b, const std::vector<std::vector<Fp>>& c) {
  const size_t m = a.size(), n = m ? a[0].size() : 1;
  int32_t log_n = 0;
  while (((size_t)1 << log_n) < n) ++log_n;
  if (n != (size_t)1 << log_n || b.size() != m || c.size() != m) throw Error("groth16_quotient: three batches of m arrays of 2^log_n values");
  DeviceBuffer da = detail::fr_arrays_up("groth16_quotient", a, n), db = detail::fr_arrays_up("groth16_quotient", b, n), dc = detail::fr_arrays_up("groth16_quotient", c, n);
  DeviceBuffer dh(4 * n * m * sizeof(uint64_t) + 8);
  check(sylow_hip_groth16_quotient_batch(da.as<uint64_t>(), db.as<uint64_t>(), dc.as<uint64_t>(), log_n, m, dh.as<uint64_t>(), nullptr), "sylow_hip_groth16_quotient_batch");
  return detail::fr_arrays_down(dh, n, m);
}
// An R1CS for the prover: variable 0 is the constant 1, variables 1 .. n_inputs are public, the domain has 2^log_n >= a.rows() points
struct Groth16Circuit {
  CsrMatrix a, b, c;
  size_t n_vars, n_inputs;
  int32_t log_n;
};
// A proving key, arkworks' names; *_inf are the queries' identity flags (empty: none flagged)
struct Groth16ProvingKey {
  G1Affine alpha_g1, beta_g1, delta_g1;
  G2Affine beta_g2, delta_g2;
  std::vector<G1Affine> a_query, b_g1_query;
  std::vector<G2Affine> b_g2_query;
  std::vector<G1Affine> h_query, l_query;                 // 2^log_n - 1 and n_vars - n_inputs - 1 points
  std::vector<uint8_t> a_query_inf, b_g1_query_inf, b_g2_query_inf, h_query_inf, l_query_inf;
};
struct Groth16Proofs {
  std::vector<G1Affine> a, c;
  std::vector<G2Affine> b;
  std::vector<uint8_t> a_inf, b_inf, c_inf;
};
// One proof per witness z[j] (n_vars values each) with the caller's randomness r[j], s[j] (sylow_hip_groth16_prove_batch): what groth16_verify
// takes with inputs z[j][1 .. n_inputs].  Neither z_0 = 1 nor the constraints are checked.
inline Groth16Proofs groth16_prove(const Groth16ProvingKey& pk, const Groth16Circuit& ct, const std::vector<std::vector<Fp>>& z, const std::vector<Fp>& r,
                                   const std::vector<Fp>& s) {
  const size_t m = z.size(), n = (size_t)1 << ct.log_n;
  if (r.size() != m || s.size() != m) throw Error("groth16_prove: one r and one s per witness");
  if (ct.n_inputs >= ct.n_vars || pk.a_query.size() != ct.n_vars || pk.b_g1_query.size() != ct.n_vars || pk.b_g2_query.size() != ct.n_vars ||
      pk.h_query.size() != n - 1 || pk.l_query.size() != ct.n_vars - ct.n_inputs - 1 || ct.b.rows() != ct.a.rows() || ct.c.rows() != ct.a.rows())
    throw Error("groth16_prove: the proving key does not fit the circuit");
  detail::CsrDevice da = detail::csr_up(ct.a), db = detail::csr_up(ct.b), dc = detail::csr_up(ct.c);
  auto one1 = [](const G1Affine& p) { return to_device_soa(std::vector<G1Affine>{p}); };
  auto one2 = [](const G2Affine& p) { return to_device_soa(std::vector<G2Affine>{p}); };
  DeviceBuffer alpha = one1(pk.alpha_g1), beta1 = one1(pk.beta_g1), delta1 = one1(pk.delta_g1), beta2 = one2(pk.beta_g2), delta2 = one2(pk.delta_g2);
  DeviceBuffer aq = to_device_soa(pk.a_query), b1q = to_device_soa(pk.b_g1_query), b2q = to_device_soa(pk.b_g2_query), hq = to_device_soa(pk.h_query), lq = to_device_soa(pk.l_query);
  auto flags = [](const std::vector<uint8_t>& f, size_t n) { return Flags(f.empty() ? nullptr : &f, n); };
  Flags aqi = flags(pk.a_query_inf, ct.n_vars), b1qi = flags(pk.b_g1_query_inf, ct.n_vars), b2qi = flags(pk.b_g2_query_inf, ct.n_vars), hqi = flags(pk.h_query_inf, n - 1),
        lqi = flags(pk.l_query_inf, pk.l_query.size());
  DeviceBuffer dz = detail::fr_arrays_up("groth16_prove", z, ct.n_vars);
  auto dr = to_device_soa(r); auto ds = to_device_soa(s);
  DeviceBuffer oa(m * sizeof(G1Affine) + 8), ob(m * sizeof(G2Affine) + 8), oc(m * sizeof(G1Affine) + 8), oai(m + 8), obi(m + 8), oci(m + 8);
  check(sylow_hip_groth16_prove_batch(da.row_ptr.as<uint64_t>(), da.col.as<uint64_t>(), da.val.as<uint64_t>(), da.nnz, db.row_ptr.as<uint64_t>(), db.col.as<uint64_t>(),
                                      db.val.as<uint64_t>(), db.nnz, dc.row_ptr.as<uint64_t>(), dc.col.as<uint64_t>(), dc.val.as<uint64_t>(), dc.nnz, da.rows, ct.n_vars,
                                      ct.n_inputs, ct.log_n, alpha.as<uint64_t>(), beta1.as<uint64_t>(), delta1.as<uint64_t>(), beta2.as<uint64_t>(), delta2.as<uint64_t>(),
                                      aq.as<uint64_t>(), aqi.ptr, b1q.as<uint64_t>(), b1qi.ptr, b2q.as<uint64_t>(), b2qi.ptr, hq.as<uint64_t>(), hqi.ptr, lq.as<uint64_t>(),
                                      lqi.ptr, dz.as<uint64_t>(), dr.as<uint64_t>(), ds.as<uint64_t>(), m, oa.as<uint64_t>(), oai.as<uint8_t>(), ob.as<uint64_t>(),
                                      obi.as<uint8_t>(), oc.as<uint64_t>(), oci.as<uint8_t>(), nullptr), "sylow_hip_groth16_prove_batch");
  Groth16Proofs out;
  fetch_flags(&out.a_inf, oai, m); fetch_flags(&out.b_inf, obi, m); fetch_flags(&out.c_inf, oci, m);
  out.a = from_device_soa<G1Affine>(oa, m); out.b = from_device_soa<G2Affine>(ob, m); out.c = from_device_soa<G1Affine>(oc, m);
  return out;
}

// ---- runtime knobs of the library (no reference counterpart: the reference is one element on one thread) -----------------------------------
// Route selectors and thresholds (SYLOW_HIP_OPT_*): process-wide, results identical under every setting; value < 0 restores the default.
inline void set_option(int32_t option, int64_t value) { check(sylow_hip_set_option(option, value), "sylow_hip_set_option"); }
inline int64_t get_option(int32_t option) {
  int64_t v = -1;
  check(sylow_hip_get_option(option, &v), "sylow_hip_get_option");
  return v;
}
// Live clock probe of the metric's kernels: arm() zeroes 256 device words and hands them to the library, read() returns the engine clock (MHz)
// the wavefronts launched since arm() ran at (0 if none ran) and disarms.
class ClockProbe {
 public:
  ClockProbe() : acc_(256 * sizeof(uint64_t)) {}
  ~ClockProbe() { sylow_hip_clock_probe(nullptr); }
  void arm() {
    const std::vector<uint64_t> zero(256, 0);
    check(sylow_hip_memcpy_h2d(acc_.as<void>(), zero.data(), zero.size() * 8, nullptr), "h2d"); check(sylow_hip_stream_sync(nullptr), "sync");
    check(sylow_hip_clock_probe(acc_.as<uint64_t>()), "sylow_hip_clock_probe");
  }
  double read_mhz(uint64_t* wavefronts = nullptr) {
    check(sylow_hip_stream_sync(nullptr), "sync");
    check(sylow_hip_clock_probe(nullptr), "sylow_hip_clock_probe");
    std::vector<uint64_t> w(256);
    check(sylow_hip_memcpy_d2h(w.data(), acc_.as<void>(), w.size() * 8, nullptr), "d2h"); check(sylow_hip_stream_sync(nullptr), "sync");
    int32_t khz = 0;
    check(sylow_hip_wall_clock_khz(&khz), "sylow_hip_wall_clock_khz");
    uint64_t clk = 0, wall = 0, waves = 0;
    for (int s = 0; s < 64; ++s) { clk += w[4 * s]; wall += w[4 * s + 1]; waves += w[4 * s + 2]; }
    if (wavefronts) *wavefronts = waves;
    return wall ? (double)clk / (double)wall * khz / 1e3 : 0.0;
  }
 private:
  DeviceBuffer acc_;
};

}  // namespace sylow
