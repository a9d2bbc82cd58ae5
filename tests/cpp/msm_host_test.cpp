// C++ host-layer test of sylow::msm (include/sylow_hip.hpp) against sylow::aggregate with one job, on the same points and scalars.
// Prints results for the pytest wrapper (tests/test_gpu_cpp_msm.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"

using namespace sylow;

static bool same(const G1Affine& a, const G1Affine& b) { return std::memcmp(&a, &b, sizeof(G1Affine)) == 0; }

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    // msm on both routes == aggregate(.., 1, n): points j * G (j = 1..n), scalars from a 64-bit LCG (some words >= p)
    const size_t n = 20000;
    std::vector<Fp> a(n), k(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (size_t j = 0; j < n; ++j) {
      a[j] = Fp{{j + 1, 0, 0, 0}};
      for (int q = 0; q < 4; ++q) { s = s * 6364136223846793005ull + 1442695040888963407ull; k[j].w[q] = s; }
    }
    auto pts = mul(std::vector<G1Affine>(n, g1_generator()), a);
    const G1Affine agg = aggregate(pts, k, 1, n)[0];
    bool inf = true;
    const G1Affine m_default = msm(pts, k, &inf);
    const G1Affine m_bucket = msm(pts, k, nullptr, -1, /*min_n=*/0);
    std::printf("MSM %d%d%d\n", same(m_default, agg) ? 1 : 0, same(m_bucket, agg) ? 1 : 0, inf ? 1 : 0);
    // P + (-P) with one scalar: the identity; no points at all: the identity
    bool inf2 = false, inf3 = false;
    G1Affine neg = pts[0];
    const Fp p_mod = Fp{{0x3C208C16D87CFD47ull, 0x97816A916871CA8Dull, 0xB85045B68181585Dull, 0x30644E72E131A029ull}};
    unsigned __int128 borrow = 0;
    for (int q = 0; q < 4; ++q) {
      const unsigned __int128 d = (unsigned __int128)p_mod.w[q] - pts[0].y.w[q] - borrow;
      neg.y.w[q] = (uint64_t)d;
      borrow = (d >> 64) ? 1 : 0;
    }
    msm({pts[0], neg}, {k[0], k[0]}, &inf2);
    msm({}, {}, &inf3);
    std::printf("IDENT %d%d\n", inf2 ? 1 : 0, inf3 ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
