// C++ host-layer test of sylow::g1_ntt and sylow::KzgProver::lagrange_srs (include/sylow_hip.hpp) at log_n = 4: the round trip of 16 points
// through the transform and back, both ways and with the grid capped at one block; a delta at 1 transforms to w^i P (out_0 = P,
// out_{i+1} = w out_i with w = fr::ntt of the same delta, out_8 = -P); and the Lagrange SRS of a known tau sums to G1gen (sum_i L_i = 1) and
// transforms forward to the monomial SRS.  Prints results for the pytest wrapper (tests/test_gpu_cpp_g1_ntt.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"

using namespace sylow;

static bool same(const std::vector<G1Affine>& a, const std::vector<G1Affine>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(G1Affine)) == 0;
}
static bool none(const std::vector<uint8_t>& f) { for (const uint8_t v : f) if (v) return false; return true; }

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const size_t n = 16;
    std::vector<Fp> s(n);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto& c : s) { for (int q = 0; q < 4; ++q) { x = x * 6364136223846793005ull + 1442695040888963407ull; c.w[q] = x; } c.w[3] >>= 4; }
    const std::vector<G1Affine> gens(n, g1_generator());
    const std::vector<G1Affine> p = mul(gens, s);
    std::vector<uint8_t> f1, f2, f3;
    const std::vector<G1Affine> fwd = g1_ntt(p, false, nullptr, &f1);
    const bool round = same(g1_ntt(fwd, true, &f1, &f2), p) && none(f1) && none(f2) && same(g1_ntt(g1_ntt(p, true), false), p) &&
                       same(g1_ntt(p, false, nullptr, &f3, 1), fwd) && !same(fwd, p);
    // a delta at 1: identities everywhere else, flagged, whatever their words hold
    std::vector<G1Affine> delta(n, p[3]);
    std::vector<uint8_t> dflags(n, 1), of;
    delta[1] = p[0];
    dflags[1] = 0;
    const std::vector<G1Affine> pw = g1_ntt(delta, false, &dflags, &of);
    std::vector<Fp> d(n, Fp{{0, 0, 0, 0}});
    d[1] = Fp{{1, 0, 0, 0}};
    const std::vector<Fp> w = fr::ntt(d);                                         // w^i
    const std::vector<G1Affine> want = mul(std::vector<G1Affine>(n, p[0]), w);
    const bool probe = same(pw, want) && none(of) && std::memcmp(&pw[0], &p[0], sizeof(G1Affine)) == 0 &&
                       std::memcmp(&pw[n / 2].x, &p[0].x, sizeof(Fp)) == 0 && std::memcmp(&pw[n / 2].y, &p[0].y, sizeof(Fp)) != 0;
    // the Lagrange SRS of tau: its points sum to G1gen and its forward transform is the monomial SRS
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    std::vector<Fp> tp(n, Fp{{1, 0, 0, 0}});
    for (size_t k = 1; k < n; ++k) tp[k] = fr::mul({tp[k - 1]}, {tau})[0];
    const std::vector<G1Affine> mono = mul(gens, tp);
    const KzgProver prover(mono);
    const std::vector<G1Affine> lag = prover.lagrange_srs();
    const G1Affine total = sum(lag);
    const G1Affine g = g1_generator();
    const bool srs = same(g1_ntt(lag), mono) && std::memcmp(&total, &g, sizeof(G1Affine)) == 0 && same(lag, g1_ntt(mono, true));
    std::printf("G1NTT %d%d%d\n", round ? 1 : 0, probe ? 1 : 0, srs ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
