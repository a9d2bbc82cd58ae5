// C++ host-layer test of sylow::KzgProver (include/sylow_hip.hpp): commit to and open one polynomial of 65 coefficients under an SRS made
// with a known tau, then verify the opening with sylow::KzgVerifier; y + 1 must fail.  Prints results for the pytest wrapper
// (tests/test_gpu_cpp_kzg_prove.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"

using namespace sylow;

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const size_t len = 65;
    // tau^k for k < len in Fr on the device, then the SRS as generator multiples
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    std::vector<Fp> pw(len, Fp{{1, 0, 0, 0}});
    for (size_t k = 1; k < len; ++k) pw[k] = fr::mul({pw[k - 1]}, {tau})[0];
    const std::vector<G1Affine> srs = mul(std::vector<G1Affine>(len, g1_generator()), pw);
    const G2Affine tau_g2 = mul(std::vector<G2Affine>{g2_generator()}, std::vector<Fp>{tau})[0];
    // coefficients from a 64-bit LCG (any 256-bit words: some are >= r)
    std::vector<Fp> f(len);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (auto& c : f) for (int q = 0; q < 4; ++q) { s = s * 6364136223846793005ull + 1442695040888963407ull; c.w[q] = s; }
    const Fp z{{s, s ^ 0x55, 7, 1}};
    const KzgProver prover(srs);
    std::vector<uint8_t> c_inf, pi_inf;
    const std::vector<G1Affine> c = prover.commit({f}, &c_inf);
    const std::vector<G1Affine> c_bucket = prover.commit({f}, nullptr, -1, /*min_len=*/0);
    std::vector<Fp> y;
    const std::vector<G1Affine> pi = prover.open({f}, {z}, &y, &pi_inf);
    std::vector<Fp> y2;
    const auto q = prover.quotient({f}, {z}, &y2);
    const bool shape = c.size() == 1 && pi.size() == 1 && y.size() == 1 && !c_inf[0] && !pi_inf[0] && std::memcmp(&c[0], &c_bucket[0], sizeof(G1Affine)) == 0 &&
                       std::memcmp(&y[0], &y2[0], sizeof(Fp)) == 0 && q.size() == 1 && q[0].size() == len && (q[0][len - 1].w[0] | q[0][len - 1].w[1] | q[0][len - 1].w[2] | q[0][len - 1].w[3]) == 0;
    const KzgVerifier verifier(tau_g2);
    const std::vector<uint8_t> ok = verifier.verify(KzgOpenings{c, pi, {z}, y});
    Fp y_bad = y[0];
    y_bad.w[0] ^= 1;
    const std::vector<uint8_t> bad = verifier.verify(KzgOpenings{c, pi, {z}, {y_bad}});
    std::printf("PROVE %d%d%d\n", shape ? 1 : 0, ok[0] ? 1 : 0, bad[0] ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
