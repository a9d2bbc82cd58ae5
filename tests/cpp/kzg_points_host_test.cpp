// C++ test of the several-point KZG opening through the C ABI with raw device pointers (include/sylow_hip_kzg_points.h): three polynomials of
// 37 coefficients under an SRS made with a known tau are committed (sylow::KzgProver), opened at k = 4 points each with
// sylow_hip_kzg_open_points_batch -- ONE proof per polynomial -- and checked with sylow_hip_kzg_verify_points_batch under the G2 powers
// tau^i G2gen, i <= k.  Then one claimed value is altered (its row alone must fail), one row gets a repeated point (rejected), the quotient
// call must agree with the opening's values, and k = 0 and k = 65 are SYLOW_HIP_E_ARG.  Prints results for the pytest wrapper
// (tests/test_gpu_cpp_kzg_points.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"
#include "sylow_hip_kzg_points.h"

using namespace sylow;

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const size_t len = 37, m = 3, k = 4;
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    std::vector<Fp> pw(len, Fp{{1, 0, 0, 0}});
    for (size_t i = 1; i < len; ++i) pw[i] = fr::mul({pw[i - 1]}, {tau})[0];
    const std::vector<G1Affine> srs = mul(std::vector<G1Affine>(len, g1_generator()), pw);
    const std::vector<G1Affine> key_g1(srs.begin(), srs.begin() + k);
    const std::vector<G2Affine> key_g2 = mul(std::vector<G2Affine>(k + 1, g2_generator()), std::vector<Fp>(pw.begin(), pw.begin() + k + 1));
    // coefficients and points from a 64-bit LCG (any 256-bit words: some are >= r); coeffs [m][4][len] as the C ABI lays them out
    std::vector<std::vector<Fp>> polys(m, std::vector<Fp>(len));
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&s] { s = s * 6364136223846793005ull + 1442695040888963407ull; return s; };
    for (auto& f : polys) for (auto& c : f) for (int q = 0; q < 4; ++q) c.w[q] = next();
    std::vector<uint64_t> flat(4 * len * m);
    for (size_t j = 0; j < m; ++j) for (size_t e = 0; e < len; ++e) for (size_t w = 0; w < 4; ++w) flat[(j * 4 + w) * len + e] = polys[j][e].w[w];
    std::vector<Fp> z(m * k);                                      // (row j, point i) at j k + i
    for (auto& v : z) for (int q = 0; q < 4; ++q) v.w[q] = next();

    DeviceBuffer d_srs = to_device_soa(srs), d_k1 = to_device_soa(key_g1), d_k2 = to_device_soa(key_g2), d_z = to_device_soa(z), d_coeffs(flat.size() * 8);
    check(sylow_hip_memcpy_h2d(d_coeffs.as<void>(), flat.data(), flat.size() * 8, nullptr), "h2d");
    check(sylow_hip_stream_sync(nullptr), "sync");
    DeviceBuffer d_y(m * k * sizeof(Fp)), d_y2(m * k * sizeof(Fp)), d_pi(m * sizeof(G1Affine)), d_pi_inf(m), d_ok(m);
    check(sylow_hip_kzg_open_points_batch(d_srs.as<uint64_t>(), d_coeffs.as<uint64_t>(), len, m, d_z.as<uint64_t>(), k, d_y.as<uint64_t>(), d_pi.as<uint64_t>(),
                                          d_pi_inf.as<uint8_t>(), nullptr), "sylow_hip_kzg_open_points_batch");
    const std::vector<Fp> y = from_device_soa<Fp>(d_y, m * k);
    check(sylow_hip_kzg_quotient_points_batch(d_coeffs.as<uint64_t>(), len, m, d_z.as<uint64_t>(), k, nullptr, d_y2.as<uint64_t>(), nullptr),
          "sylow_hip_kzg_quotient_points_batch");
    const std::vector<Fp> y2 = from_device_soa<Fp>(d_y2, m * k);
    bool same = true;
    for (size_t i = 0; i < m * k; ++i) same = same && std::memcmp(y[i].w, y2[i].w, sizeof(y[i].w)) == 0;

    const KzgProver prover(srs);
    DeviceBuffer d_c = to_device_soa(prover.commit(polys));
    auto verify = [&](DeviceBuffer& zz, DeviceBuffer& yy, std::vector<uint8_t>* out) {
      check(sylow_hip_kzg_verify_points_batch(d_k1.as<uint64_t>(), d_k2.as<uint64_t>(), d_c.as<uint64_t>(), nullptr, zz.as<uint64_t>(), yy.as<uint64_t>(), k, m,
                                              d_pi.as<uint64_t>(), d_pi_inf.as<uint8_t>(), d_ok.as<uint8_t>(), nullptr), "sylow_hip_kzg_verify_points_batch");
      fetch_flags(out, d_ok, m);
    };
    std::vector<uint8_t> ok, bad, rep;
    verify(d_z, d_y, &ok);
    std::vector<Fp> y_bad = y;
    y_bad[1 * k + 2].w[0] ^= 1;                                    // one claimed value of the middle row
    DeviceBuffer d_y_bad = to_device_soa(y_bad);
    verify(d_z, d_y_bad, &bad);
    std::vector<Fp> z_rep = z, y_rep = y;
    z_rep[2 * k + 3] = z_rep[2 * k + 0];                           // the last row: its last point repeats its first, with the matching value
    y_rep[2 * k + 3] = y_rep[2 * k + 0];
    DeviceBuffer d_z_rep = to_device_soa(z_rep), d_y_rep = to_device_soa(y_rep);
    verify(d_z_rep, d_y_rep, &rep);
    const int32_t rc0 = sylow_hip_kzg_open_points_batch(d_srs.as<uint64_t>(), d_coeffs.as<uint64_t>(), len, m, d_z.as<uint64_t>(), 0, d_y.as<uint64_t>(),
                                                        d_pi.as<uint64_t>(), d_pi_inf.as<uint8_t>(), nullptr);
    const int32_t rc65 = sylow_hip_kzg_quotient_points_batch(d_coeffs.as<uint64_t>(), len, m, d_z.as<uint64_t>(), SYLOW_HIP_KZG_POINTS_MAX + 1, nullptr,
                                                             d_y2.as<uint64_t>(), nullptr);
    std::printf("POINTS %d%d%d %d%d%d %d%d%d %d %d%d\n", ok[0] ? 1 : 0, ok[1] ? 1 : 0, ok[2] ? 1 : 0, bad[0] ? 1 : 0, bad[1] ? 1 : 0, bad[2] ? 1 : 0, rep[0] ? 1 : 0,
                rep[1] ? 1 : 0, rep[2] ? 1 : 0, same ? 1 : 0, rc0 == SYLOW_HIP_E_ARG ? 1 : 0, rc65 == SYLOW_HIP_E_ARG ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
