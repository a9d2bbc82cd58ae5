// C++ host-layer test of sylow::KzgEvalProver (include/sylow_hip.hpp): open one polynomial given by its 64 values on the domain <w_64>
// under a Lagrange-basis SRS made with a known tau -- L_i(tau) = (tau^n - 1) w^i / (n (tau - w^i)), the w^i as the transform of X, the
// inverses through fr::batch_inv -- then verify the opening with sylow::KzgVerifier; y + 1 must fail.  A second opening at z = w^5, inside
// the domain, must return y = the fifth value and verify.  Prints results for the pytest wrapper (tests/test_gpu_cpp_kzg_evals.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"

using namespace sylow;

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const size_t n = 64;
    const Fp one{{1, 0, 0, 0}}, zero{{0, 0, 0, 0}};
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    // w^i: the values of the polynomial X on the domain
    std::vector<Fp> x(n, zero);
    x[1] = one;
    const std::vector<Fp> w = fr::ntt(x);
    Fp tau_n = tau;
    for (int s = 0; s < 6; ++s) tau_n = fr::mul({tau_n}, {tau_n})[0];
    const Fp c = fr::mul(fr::sub({tau_n}, {one}), fr::inv({Fp{{n, 0, 0, 0}}}))[0];       // (tau^n - 1) / n
    const std::vector<Fp> lag = fr::mul(fr::mul(std::vector<Fp>(n, c), w), fr::batch_inv(fr::sub(std::vector<Fp>(n, tau), w)));
    const std::vector<G1Affine> srs = mul(std::vector<G1Affine>(n, g1_generator()), lag);
    const G2Affine tau_g2 = mul(std::vector<G2Affine>{g2_generator()}, std::vector<Fp>{tau})[0];
    // values from a 64-bit LCG (any 256-bit words: some are >= r)
    std::vector<Fp> f(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (auto& v : f) for (int q = 0; q < 4; ++q) { s = s * 6364136223846793005ull + 1442695040888963407ull; v.w[q] = s; }
    const std::vector<Fp> z = {Fp{{s, s ^ 0x55, 7, 1}}, w[5]};
    const KzgEvalProver prover(srs);
    std::vector<uint8_t> c_inf, pi_inf;
    const std::vector<G1Affine> cm = prover.commit({f, f}, &c_inf);
    std::vector<Fp> y, y2;
    const std::vector<G1Affine> pi = prover.open({f, f}, z, &y, &pi_inf);
    const auto q = prover.quotient({f, f}, z, &y2);
    const std::vector<Fp> y3 = prover.evaluate({f, f}, z);
    const std::vector<Fp> f5 = fr::add({f[5]}, {zero});                                // the fifth value mod r
    const bool shape = cm.size() == 2 && pi.size() == 2 && y.size() == 2 && !c_inf[0] && !pi_inf[0] && !pi_inf[1] && q.size() == 2 && q[1].size() == n &&
                       std::memcmp(y.data(), y2.data(), 2 * sizeof(Fp)) == 0 && std::memcmp(y.data(), y3.data(), 2 * sizeof(Fp)) == 0 &&
                       std::memcmp(&y[1], &f5[0], sizeof(Fp)) == 0 && std::memcmp(&cm[0], &cm[1], sizeof(G1Affine)) == 0;
    const KzgVerifier verifier(tau_g2);
    const std::vector<uint8_t> ok = verifier.verify(KzgOpenings{cm, pi, z, y});
    std::vector<Fp> y_bad = y;
    y_bad[0].w[0] ^= 1;
    y_bad[1].w[0] ^= 1;
    const std::vector<uint8_t> bad = verifier.verify(KzgOpenings{cm, pi, z, y_bad});
    std::printf("EVALS %d%d%d%d%d\n", shape ? 1 : 0, ok[0] ? 1 : 0, ok[1] ? 1 : 0, bad[0] ? 1 : 0, bad[1] ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
