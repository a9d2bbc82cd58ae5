// C++ host-layer test of sylow::fr::ntt and sylow::KzgProver::commit_evals (include/sylow_hip.hpp): the round trip of 64 values (any 256-bit
// words) through the transform and back, with and without a coset shift and with the stages pinned; a delta at 1 transforms to the powers of
// the root; and commit_evals against commit of the interpolated coefficients under an SRS made with a known tau.  Prints results for the
// pytest wrapper (tests/test_gpu_cpp_ntt.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"

using namespace sylow;

static bool same(const std::vector<Fp>& a, const std::vector<Fp>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(Fp)) == 0; }

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const size_t n = 64;
    std::vector<Fp> a(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (auto& c : a) for (int q = 0; q < 4; ++q) { s = s * 6364136223846793005ull + 1442695040888963407ull; c.w[q] = s; }
    const std::vector<Fp> canonical = fr::add(a, std::vector<Fp>(n, Fp{{0, 0, 0, 0}}));          // a mod r
    const std::vector<Fp> ev = fr::ntt(a);
    const Fp g{{5, 0, 0, 0}};
    const bool round = same(fr::ntt(ev, true), canonical) && same(fr::ntt(fr::ntt(a, false, &g), true, &g), canonical) && same(fr::ntt(a, false, nullptr, 2), ev);
    // delta at 1 -> w^i: out[i + 1] = out[i] * out[1], out[n / 2] = r - 1
    std::vector<Fp> delta(n, Fp{{0, 0, 0, 0}});
    delta[1] = Fp{{1, 0, 0, 0}};
    const std::vector<Fp> pw = fr::ntt(delta);
    const std::vector<Fp> next = fr::mul(pw, std::vector<Fp>(n, pw[1]));
    bool root = pw[0].w[0] == 1 && pw[n / 2].w[0] == 0x43e1f593f0000000ull && pw[n / 2].w[3] == 0x30644e72e131a029ull;
    for (size_t i = 0; i + 1 < n; ++i) root = root && std::memcmp(&next[i], &pw[i + 1], sizeof(Fp)) == 0;
    // commit_evals(ev) == commit(a) under srs_k = tau^k G1gen
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    std::vector<Fp> tp(n, Fp{{1, 0, 0, 0}});
    for (size_t k = 1; k < n; ++k) tp[k] = fr::mul({tp[k - 1]}, {tau})[0];
    const KzgProver prover(mul(std::vector<G1Affine>(n, g1_generator()), tp));
    std::vector<uint8_t> inf_e, inf_c;
    const std::vector<G1Affine> ce = prover.commit_evals({ev, std::vector<Fp>(n, Fp{{0, 0, 0, 0}})}, &inf_e);
    const std::vector<G1Affine> cc = prover.commit({a}, &inf_c);
    const bool commit = ce.size() == 2 && std::memcmp(&ce[0], &cc[0], sizeof(G1Affine)) == 0 && !inf_e[0] && inf_e[1] == 1 && !inf_c[0];
    std::printf("NTT %d%d%d\n", round ? 1 : 0, root ? 1 : 0, commit ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
