// msm.hip -- sylow_hip_g1_msm / _tuned: the bucket method of msm_bucket.hpp with one lane per point, on E(Fp).  Every point has order r
// (cofactor 1), so the scalars are reduced mod r on top of Fp::new.  tools/msm_model.py is the host-side model (tests/test_msm_model.py).
#include "msm_bucket.hpp"

namespace msmh {
// the geometry policy of msm_bucket.hpp for G1: thread t is point t, and an F29 is the coordinate itself
struct G1Lane {
  typedef F29 F;
  typedef OpsF29I Ops;
  static constexpr int LANES = 1;
  static constexpr bool MOD_R = true;
  static constexpr size_t DEFAULT_MIN = (size_t)1 << 18;    // the smallest measured size the bucket route wins: 2^18 1.6 x, 2^17 0.28 x
  static constexpr int REDUCE_WAVES = 2;                    // k_msm_bucket_reduce under HEAVY_BOUNDS
  static constexpr const char* CHUNK_LAUNCH = "msm chunk launch";
  static int default_window(size_t n) { return msm::default_window(n); }
  template <class T> static BN_DEV T elem(T t) { return t; }
  template <class T> static BN_DEV int role(T) { return 0; }
  static BN_DEV F wrap(const F29& a) { return a; }
  static BN_DEV const F29& limbs(const F& a) { return a; }
  static BN_DEV G1W prepare(const u64* pxy, size_t n, size_t i, int) {
    return G1W{f29_from_fp_reduced(load_fp(pxy, n, i, 0)), f29_from_fp_reduced(load_fp(pxy, n, i, 4)), OpsF29::one()};
  }
  static BN_DEV void finish(u64* oxy, uint8_t* oinf, int, const G1W& acc) {
    Fp x, y; bool inf;
    g1w_to_affine(x, y, inf, acc);
    store_fp(oxy, 1, 0, 0, x); store_fp(oxy, 1, 0, 4, y);
    oinf[0] = inf ? 1 : 0;
  }
};
// small n (or a budget below one chunk of the bucket route): a scalar multiplication per lane, then the batch sum
int32_t composed(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  if (!n) {
    host::Lease ws;
    int32_t rc = ws.acquire(12 * sizeof(u64), (hipStream_t)stream);
    if (rc != SYLOW_HIP_OK) return rc;
    rc = g1h::sum_tree((uint64_t*)ws.p, 0, out_xy, out_inf, 1, 0, 0, stream);
    return host::finish(rc, ws);
  }
  host::Lease ws;
  int32_t rc = ws.acquire(n * (8 * sizeof(u64) + 1) + 12 * n * sizeof(u64) + 256, (hipStream_t)stream);
  if (rc != SYLOW_HIP_OK) return rc;
  uint64_t* acc = (uint64_t*)ws.p;
  uint64_t* xy = acc + 12 * n;
  uint8_t* inf = (uint8_t*)(xy + 8 * n);
  rc = sylow_hip_g1_scalar_mul_batch(p_xy, p_inf, k, xy, inf, n, stream);
  if (rc == SYLOW_HIP_OK) rc = g1h::sum(xy, inf, n, acc, out_xy, out_inf, 1, 0, 0, stream);
  return host::finish(rc, ws);
}
size_t g1_default_min() { return G1Lane::DEFAULT_MIN; }
size_t default_budget() { return msm::MSM_DEFAULT_BUDGET; }
bool window_ok(int32_t window) { return window < 0 || (window >= msm::MSM_C_MIN && window <= msm::MSM_C_MAX); }
}  // namespace msmh

extern "C" {
int32_t sylow_hip_g1_msm_tuned(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, int32_t window, int64_t min_n_arg,
                               uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  return msm::tuned<msmh::G1Lane>(p_xy, p_inf, k, n, window, min_n_arg, out_xy, out_inf, stream,
                                  [&] { return msmh::composed(p_xy, p_inf, k, n, out_xy, out_inf, stream); });
}
int32_t sylow_hip_g1_msm(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* k, size_t n, uint64_t* out_xy, uint8_t* out_inf, void* stream) {
  return sylow_hip_g1_msm_tuned(p_xy, p_inf, k, n, -1, -1, out_xy, out_inf, stream);
}
}  // extern "C"
