// C++ host-layer test of sylow::KzgProver::open_all (include/sylow_hip.hpp) at log_n = 4 under the monomial SRS of a known tau: the 16 proofs
// of each of three polynomials -- a random one, a constant and X^15 -- are word for word KzgProver::open of the polynomial repeated 16 times
// at z_i = w^i (w^i from fr::ntt of a delta), the values are fr::ntt of the coefficients, every proof of the constant is flagged, the grid
// capped at one block gives the same words, and all 16 rows (C, w^i, y_i, pi_i) of the random polynomial pass KzgVerifier::verify while
// none does with y_i + 1.  Prints results for the pytest wrapper (tests/test_gpu_cpp_kzg_open_all.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"

using namespace sylow;

static bool same(const std::vector<G1Affine>& a, const std::vector<G1Affine>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(G1Affine)) == 0;
}
static bool same(const std::vector<Fp>& a, const std::vector<Fp>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(Fp)) == 0; }

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const size_t n = 16;
    const Fp zero{{0, 0, 0, 0}}, one{{1, 0, 0, 0}};
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    std::vector<Fp> tp(n, one);
    for (size_t k = 1; k < n; ++k) tp[k] = fr::mul({tp[k - 1]}, {tau})[0];
    const std::vector<G1Affine> mono = mul(std::vector<G1Affine>(n, g1_generator()), tp);
    const KzgProver prover(mono);
    std::vector<Fp> f(n), constant(n, zero), top(n, zero), d(n, zero);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto& c : f) { for (int q = 0; q < 4; ++q) { x = x * 6364136223846793005ull + 1442695040888963407ull; c.w[q] = x; } }   // any words: taken mod r
    constant[0] = Fp{{9, 0, 0, 0}};
    top[n - 1] = one;
    d[1] = one;
    const std::vector<Fp> w = fr::ntt(d);                                         // w^i
    const std::vector<std::vector<Fp>> polys{f, constant, top};
    std::vector<std::vector<Fp>> y;
    std::vector<std::vector<uint8_t>> inf, inf1;
    const std::vector<std::vector<G1Affine>> pi = prover.open_all(polys, &y, &inf);
    bool routes = pi.size() == 3 && y.size() == 3 && inf.size() == 3, values = true, flags = true;
    for (size_t j = 0; routes && j < 3; ++j) {
      std::vector<Fp> wy;
      std::vector<uint8_t> winf;
      const std::vector<G1Affine> want = prover.open(std::vector<std::vector<Fp>>(n, polys[j]), w, &wy, &winf);
      routes = routes && same(pi[j], want) && inf[j] == winf;
      values = values && same(y[j], wy) && same(y[j], fr::ntt(polys[j]));
      for (size_t i = 0; i < n; ++i) flags = flags && inf[j][i] == (j == 1 ? 1 : 0);
    }
    const std::vector<std::vector<G1Affine>> capped = prover.open_all(polys, nullptr, &inf1, 1);
    bool pinned = capped.size() == 3 && inf1 == inf;
    for (size_t j = 0; pinned && j < 3; ++j) pinned = same(capped[j], pi[j]);
    // through the verifier: tau G2gen, the commitment repeated
    const KzgVerifier verifier(mul(std::vector<G2Affine>{g2_generator()}, {tau})[0]);
    const std::vector<G1Affine> c(n, prover.commit({f})[0]);
    std::vector<Fp> bad = y[0];
    for (auto& v : bad) v = fr::add({v}, {one})[0];
    bool good = true, none = true;
    for (const uint8_t ok : verifier.verify(KzgOpenings{c, pi[0], w, y[0]})) good = good && ok;
    for (const uint8_t ok : verifier.verify(KzgOpenings{c, pi[0], w, bad})) none = none && !ok;
    std::printf("OPENALL %d%d%d%d%d\n", routes ? 1 : 0, values ? 1 : 0, flags ? 1 : 0, pinned ? 1 : 0, good && none ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
