// C++ test of the folded KZG openings through the C ABI with raw device pointers (include/sylow_hip.h, "KZG, folded openings"): five
// polynomials of 33 coefficients in the groups {3, 0, 2} under an SRS made with a known tau are committed (sylow::KzgProver), opened with
// sylow_hip_kzg_open_multi_batch and checked with sylow_hip_kzg_verify_multi_batch; the host's group_start array is overwritten right after
// every call returns.  The folded rows from sylow_hip_kzg_combine_openings_batch must pass sylow::KzgVerifier, a y_j + 1 must fail its group
// alone, the empty group's row is (identity, 0, identity), the linear combination must agree with the powers folded by fr::mul / fr::add, and
// a group_start that does not end at m is SYLOW_HIP_E_ARG.  Prints results for the pytest wrapper (tests/test_gpu_cpp_kzg_multi.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"

using namespace sylow;

static bool is_zero(const Fp& a) { return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) == 0; }

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const size_t len = 33, m = 5, G = 3;
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    std::vector<Fp> pw(len, Fp{{1, 0, 0, 0}});
    for (size_t k = 1; k < len; ++k) pw[k] = fr::mul({pw[k - 1]}, {tau})[0];
    const std::vector<G1Affine> srs = mul(std::vector<G1Affine>(len, g1_generator()), pw);
    const G2Affine tau_g2 = mul(std::vector<G2Affine>{g2_generator()}, std::vector<Fp>{tau})[0];
    // coefficients from a 64-bit LCG (any 256-bit words: some are >= r); coeffs [m][4][len] as the C ABI lays them out
    std::vector<std::vector<Fp>> polys(m, std::vector<Fp>(len));
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (auto& f : polys) for (auto& c : f) for (int q = 0; q < 4; ++q) { s = s * 6364136223846793005ull + 1442695040888963407ull; c.w[q] = s; }
    std::vector<uint64_t> flat(4 * len * m);
    for (size_t j = 0; j < m; ++j) for (size_t k = 0; k < len; ++k) for (size_t w = 0; w < 4; ++w) flat[(j * 4 + w) * len + k] = polys[j][k].w[w];
    const std::vector<Fp> z = {Fp{{s, s ^ 0x55, 7, 1}}, Fp{{3, 0, 0, 0}}, Fp{{s ^ 0xAA, 5, s, 2}}};
    const std::vector<Fp> gamma = {Fp{{s + 1, s ^ 0x77, 11, 3}}, Fp{{9, 0, 0, 0}}, Fp{{s + 2, 13, s, 4}}};
    uint64_t group_start[G + 1] = {0, 3, 3, 5};

    DeviceBuffer d_srs = to_device_soa(srs), d_z = to_device_soa(z), d_gamma = to_device_soa(gamma), d_coeffs(flat.size() * 8);
    check(sylow_hip_memcpy_h2d(d_coeffs.as<void>(), flat.data(), flat.size() * 8, nullptr), "h2d");
    check(sylow_hip_stream_sync(nullptr), "sync");
    DeviceBuffer d_y(m * sizeof(Fp)), d_pi(G * sizeof(G1Affine)), d_pi_inf(G), d_ok(G), d_cf(G * sizeof(G1Affine)), d_cf_inf(G), d_yf(G * sizeof(Fp));
    check(sylow_hip_kzg_open_multi_batch(d_srs.as<uint64_t>(), d_coeffs.as<uint64_t>(), len, m, group_start, G, d_z.as<uint64_t>(), d_gamma.as<uint64_t>(),
                                         d_y.as<uint64_t>(), d_pi.as<uint64_t>(), d_pi_inf.as<uint8_t>(), nullptr), "sylow_hip_kzg_open_multi_batch");
    std::memset(group_start, 0xFF, sizeof(group_start));          // read before the call returned: the stream may not even have started
    const std::vector<Fp> y = from_device_soa<Fp>(d_y, m);
    const std::vector<G1Affine> pi = from_device_soa<G1Affine>(d_pi, G);
    std::vector<uint8_t> pi_inf, cf_inf, ok, bad;
    fetch_flags(&pi_inf, d_pi_inf, G);

    const KzgProver prover(srs);
    const std::vector<G1Affine> c = prover.commit(polys);
    DeviceBuffer d_c = to_device_soa(c);
    const uint64_t gs[G + 1] = {0, 3, 3, 5};
    std::memcpy(group_start, gs, sizeof(gs));
    check(sylow_hip_kzg_verify_multi_batch(to_device_soa(std::vector<G2Affine>{tau_g2}).as<uint64_t>(), d_c.as<uint64_t>(), nullptr, d_y.as<uint64_t>(), m, group_start, G,
                                           d_z.as<uint64_t>(), d_gamma.as<uint64_t>(), d_pi.as<uint64_t>(), d_pi_inf.as<uint8_t>(), d_ok.as<uint8_t>(), nullptr),
          "sylow_hip_kzg_verify_multi_batch");
    std::memset(group_start, 0xFF, sizeof(group_start));
    fetch_flags(&ok, d_ok, G);
    // one claimed value of the last group altered
    std::vector<Fp> y_bad = y;
    y_bad[4].w[0] ^= 1;
    DeviceBuffer d_y_bad = to_device_soa(y_bad);
    check(sylow_hip_kzg_verify_multi_batch(to_device_soa(std::vector<G2Affine>{tau_g2}).as<uint64_t>(), d_c.as<uint64_t>(), nullptr, d_y_bad.as<uint64_t>(), m, gs, G,
                                           d_z.as<uint64_t>(), d_gamma.as<uint64_t>(), d_pi.as<uint64_t>(), d_pi_inf.as<uint8_t>(), d_ok.as<uint8_t>(), nullptr),
          "sylow_hip_kzg_verify_multi_batch");
    fetch_flags(&bad, d_ok, G);
    // the folded rows on their own, through the cached-table verifier
    check(sylow_hip_kzg_combine_openings_batch(d_c.as<uint64_t>(), nullptr, d_y.as<uint64_t>(), m, gs, G, d_gamma.as<uint64_t>(), d_cf.as<uint64_t>(),
                                               d_cf_inf.as<uint8_t>(), d_yf.as<uint64_t>(), nullptr), "sylow_hip_kzg_combine_openings_batch");
    const std::vector<G1Affine> cf = from_device_soa<G1Affine>(d_cf, G);
    const std::vector<Fp> yf = from_device_soa<Fp>(d_yf, G);
    fetch_flags(&cf_inf, d_cf_inf, G);
    const KzgVerifier verifier(tau_g2);
    const std::vector<uint8_t> rows = verifier.verify(KzgOpenings{{cf[0], cf[2]}, {pi[0], pi[2]}, {z[0], z[2]}, {yf[0], yf[2]}});
    const bool empty = cf_inf[1] && pi_inf[1] && is_zero(yf[1]) && is_zero(cf[1].x) && cf[1].y.w[0] == 1 && !cf_inf[0] && !cf_inf[2] && !pi_inf[0] && !pi_inf[2];
    // the linear combination against Horner with fr::mul and fr::add on the first group: F = f_0 + gamma (f_1 + gamma f_2)
    DeviceBuffer d_pow(m * sizeof(Fp)), d_f(4 * len * G * 8);
    check(sylow_hip_fr_group_powers_batch(d_gamma.as<uint64_t>(), gs, G, m, d_pow.as<uint64_t>(), nullptr), "sylow_hip_fr_group_powers_batch");
    check(sylow_hip_fr_lincomb_batch(d_coeffs.as<uint64_t>(), len, m, d_pow.as<uint64_t>(), gs, G, d_f.as<uint64_t>(), nullptr), "sylow_hip_fr_lincomb_batch");
    std::vector<uint64_t> fw(4 * len * G);
    check(sylow_hip_memcpy_d2h(fw.data(), d_f.as<void>(), fw.size() * 8, nullptr), "d2h");
    check(sylow_hip_stream_sync(nullptr), "sync");
    const std::vector<Fp> g0(len, gamma[0]);
    const std::vector<Fp> horner = fr::add(polys[0], fr::mul(g0, fr::add(polys[1], fr::mul(g0, polys[2]))));
    bool lin = true;
    for (size_t k = 0; k < len; ++k) for (size_t w = 0; w < 4; ++w) lin = lin && fw[w * len + k] == horner[k].w[w] && fw[(4 + w) * len + k] == 0;
    // a group_start that does not end at m: refused, nothing enqueued
    const uint64_t wrong[G + 1] = {0, 3, 3, 4};
    const int32_t rc = sylow_hip_fr_lincomb_batch(d_coeffs.as<uint64_t>(), len, m, d_pow.as<uint64_t>(), wrong, G, d_f.as<uint64_t>(), nullptr);
    std::printf("MULTI %d%d%d %d%d%d %d%d %d%d%d\n", ok[0] ? 1 : 0, ok[1] ? 1 : 0, ok[2] ? 1 : 0, bad[0] ? 1 : 0, bad[1] ? 1 : 0, bad[2] ? 1 : 0, rows[0] ? 1 : 0,
                rows[1] ? 1 : 0, empty ? 1 : 0, lin ? 1 : 0, rc == SYLOW_HIP_E_ARG ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
