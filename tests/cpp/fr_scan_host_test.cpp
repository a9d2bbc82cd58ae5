// C++ test of the scans over Fr and of PLONK's permutation grand product through the C ABI with raw device pointers
// (include/sylow_hip_fr_scan.h), at log_n = 3, W = 2.  The identity columns against words baked in from tests/fr_scan_model.py
// (tests/test_gpu_cpp_fr_scan.py checks the tables against the model on the CPU); sigma gathered on the host through the mapping
// p -> 3 p mod 16; wires constant on its cycles; z against the baked words, z_n = 1 and status 0, on the default form and the tuned one; one
// changed wire: status 2; the running product of 1 .. 8 is the factorials and the ratio scan of (k + 1) / k telescopes; W = 33, op = 2 and
// totals_tile = 0 are SYLOW_HIP_E_ARG.  Prints results for the pytest wrapper.
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"
#include "sylow_hip_fr_scan.h"

using namespace sylow;

static const uint64_t IDENT[16][4] = {
    {0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x948dad4ac1bd5e80ull, 0x52627366f8170a0aull, 0xec9b9e2f96afef36ull, 0x2b337de1c8c14f22ull},
    {0x231204708f703636ull, 0x5cea24f6fd736becull, 0x048b6e193fd84104ull, 0x30644e72e131a029ull},
    {0xb8d01be8e846a566ull, 0x07c2d99b3852513aull, 0xbd157ac850893a6full, 0x1d59376149b959ccull},
    {0x43e1f593f0000000ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0xaf5448492e42a181ull, 0xd5d174e181a26686ull, 0xcbb4a786ead16926ull, 0x0530d09118705106ull},
    {0x20cff123608fc9cbull, 0xcb49c3517c4604a5ull, 0xb3c4d79d41a91758ull, 0x0000000000000000ull},
    {0x8b11d9ab07b95a9bull, 0x20710ead41671f56ull, 0xfb3acaee30f81deeull, 0x130b17119778465cull},
    {0x0000000000000005ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0xd73c8c2608b2d87cull, 0xfb1c9fe0f18d6fefull, 0xbdc90013eb6a4a9aull, 0x16703b9d67000b07ull},
    {0x9fd23fe30d310f0aull, 0x2fc317b10c5b5957ull, 0x35780fa43933e3a1ull, 0x30644e72e131a026ull},
    {0xd06aaad0b9613afbull, 0xae32872eac6f4471ull, 0x887a94c60e2a1b13ull, 0x0191298dcd09e082ull},
    {0x43e1f593effffffcull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0x6ca5696de74d2785ull, 0x2d174867882c00a1ull, 0xfa8745a296170dc2ull, 0x19f412d57a319521ull},
    {0xa40fb5b0e2cef0f7ull, 0xf870d0976d5e1739ull, 0x82d83612484d74bbull, 0x0000000000000003ull},
    {0x73774ac3369ec506ull, 0x7a016119cd4a2c1full, 0x2fd5b0f073573d49ull, 0x2ed324e51427bfa7ull}
};
static const uint64_t Z[8][4] = {
    {0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x5dcf415303956090ull, 0x5834aff833d31cf3ull, 0x963b66eb540affabull, 0x220714bfd69925edull},
    {0x975da1fdf6ea5feaull, 0x5cb79424f42b1bebull, 0xc98ad0626bc0c617ull, 0x23e637674825aeb8ull},
    {0xc41314ead58b92c5ull, 0x30346c0b6548581dull, 0xbb52d20e7226ce3bull, 0x269f4186cc0017d7ull},
    {0xc41314ead58b92c5ull, 0x30346c0b6548581dull, 0xbb52d20e7226ce3bull, 0x269f4186cc0017d7ull},
    {0x555630eb9804de48ull, 0x07d0353bc90d955bull, 0xf25d22e6c7c90b1full, 0x2361f5dfab08c53cull},
    {0x3dee7ae63196fb2eull, 0x292a8d5ce455404eull, 0x061ac63f70ddb7c3ull, 0x24c25c575032dd3full}
};

static void up(DeviceBuffer& d, const std::vector<uint64_t>& v) { check(sylow_hip_memcpy_h2d(d.as<void>(), v.data(), v.size() * 8, nullptr), "h2d"); }
static std::vector<uint64_t> down(DeviceBuffer& d, size_t words) {
  std::vector<uint64_t> v(words);
  check(sylow_hip_memcpy_d2h(v.data(), d.as<void>(), words * 8, nullptr), "d2h");
  check(sylow_hip_stream_sync(nullptr), "sync");
  return v;
}
// soa [rows][4][n] against want [rows * n][4]
template <size_t N> static bool same(const std::vector<uint64_t>& soa, const uint64_t (&want)[N][4], size_t n) {
  bool ok = soa.size() == 4 * N;
  for (size_t i = 0; ok && i < N; ++i)
    for (size_t w = 0; w < 4; ++w) ok = ok && soa[(i / n * 4 + w) * n + i % n] == want[i][w];
  return ok;
}
static bool is_small(const std::vector<uint64_t>& soa, size_t stride, size_t i, uint64_t v) {
  return soa[i] == v && !soa[stride + i] && !soa[2 * stride + i] && !soa[3 * stride + i];
}

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const int32_t log_n = 3, W = 2;
    const size_t n = 8, m = 1;
    // ---- the identity columns, and sigma through the mapping
    const std::vector<uint64_t> shifts = {1, 5, 0, 0, 0, 0, 0, 0};          // [4][W]
    DeviceBuffer d_sh(4 * W * 8), d_id(W * 4 * n * 8), d_sg(W * 4 * n * 8);
    up(d_sh, shifts);
    check(sylow_hip_plonk_identity_batch(d_sh.as<uint64_t>(), log_n, W, d_id.as<uint64_t>(), nullptr), "sylow_hip_plonk_identity_batch");
    const std::vector<uint64_t> ident = down(d_id, W * 4 * n);
    const bool ident_ok = same(ident, IDENT, n);
    std::vector<uint64_t> sigma(W * 4 * n), wires(W * 4 * n, 0);
    const uint64_t cycle_of[16] = {0, 1, 2, 1, 3, 4, 2, 4, 5, 1, 6, 1, 3, 4, 6, 4};      // the cycles of p -> 3 p mod 16, numbered by their least position
    for (size_t p = 0; p < 16; ++p) {
      const size_t q = p * 3 % 16;
      for (size_t w = 0; w < 4; ++w) sigma[(p / n * 4 + w) * n + p % n] = ident[(q / n * 4 + w) * n + q % n];
      wires[(p / n * 4) * n + p % n] = 1000 + 17 * cycle_of[p];
    }
    const std::vector<uint64_t> beta = {0x1234567, 0, 0, 0}, gamma = {0x89ABCDEF, 0, 0, 0};
    DeviceBuffer d_w(W * 4 * n * 8), d_b(32), d_g(32), d_z(4 * n * 8), d_t(32), d_st(1);
    up(d_sg, sigma); up(d_w, wires); up(d_b, beta); up(d_g, gamma);
    bool z_ok = true;
    std::vector<uint8_t> st;
    for (int tuned = 0; tuned < 2; ++tuned) {
      const int32_t rc = tuned ? sylow_hip_plonk_permutation_batch_tuned(d_w.as<uint64_t>(), d_sg.as<uint64_t>(), d_sh.as<uint64_t>(), d_b.as<uint64_t>(), d_g.as<uint64_t>(),
                                                                         log_n, W, m, 1, 1, d_z.as<uint64_t>(), d_t.as<uint64_t>(), d_st.as<uint8_t>(), nullptr)
                               : sylow_hip_plonk_permutation_batch(d_w.as<uint64_t>(), d_sg.as<uint64_t>(), d_sh.as<uint64_t>(), d_b.as<uint64_t>(), d_g.as<uint64_t>(), log_n,
                                                                   W, m, d_z.as<uint64_t>(), d_t.as<uint64_t>(), d_st.as<uint8_t>(), nullptr);
      check(rc, "sylow_hip_plonk_permutation_batch");
      fetch_flags(&st, d_st, 1);
      z_ok = z_ok && same(down(d_z, 4 * n), Z, n) && is_small(down(d_t, 4), 1, 0, 1) && st[0] == 0;
    }
    // one changed wire on a cycle of length 4: z does not close
    wires[3] += 1;
    up(d_w, wires);
    check(sylow_hip_plonk_permutation_batch(d_w.as<uint64_t>(), d_sg.as<uint64_t>(), d_sh.as<uint64_t>(), d_b.as<uint64_t>(), d_g.as<uint64_t>(), log_n, W, m,
                                            d_z.as<uint64_t>(), nullptr, d_st.as<uint8_t>(), nullptr), "sylow_hip_plonk_permutation_batch");
    fetch_flags(&st, d_st, 1);
    const bool broken = st[0] == 2 && is_small(down(d_z, 4 * n), n, 0, 1);
    // ---- the scans: the running product of 1 .. 8, and the ratio (k + 1) / k, whose exclusive product telescopes to k
    std::vector<uint64_t> a(4 * n, 0), nu(4 * n, 0);
    for (size_t k = 0; k < n; ++k) { a[k] = k + 1; nu[k] = k + 2; }
    DeviceBuffer d_a(4 * n * 8), d_nu(4 * n * 8), d_o(4 * n * 8);
    up(d_a, a); up(d_nu, nu);
    check(sylow_hip_fr_scan_batch(d_a.as<uint64_t>(), n, 1, 1, 0, d_o.as<uint64_t>(), d_t.as<uint64_t>(), nullptr), "sylow_hip_fr_scan_batch");
    std::vector<uint64_t> o = down(d_o, 4 * n);
    bool scan_ok = is_small(down(d_t, 4), 1, 0, 40320);
    uint64_t f = 1;
    for (size_t k = 0; k < n; ++k) { f *= k + 1; scan_ok = scan_ok && is_small(o, n, k, f); }
    check(sylow_hip_fr_scan_batch_tuned(d_a.as<uint64_t>(), n, 1, 0, 1, 1, 2, d_o.as<uint64_t>(), nullptr, nullptr), "sylow_hip_fr_scan_batch_tuned");
    o = down(d_o, 4 * n);
    for (size_t k = 0; k < n; ++k) scan_ok = scan_ok && is_small(o, n, k, k * (k + 1) / 2);
    check(sylow_hip_fr_ratio_scan_batch(d_nu.as<uint64_t>(), d_a.as<uint64_t>(), n, 1, 1, d_o.as<uint64_t>(), d_t.as<uint64_t>(), d_st.as<uint8_t>(), nullptr),
          "sylow_hip_fr_ratio_scan_batch");
    o = down(d_o, 4 * n);
    fetch_flags(&st, d_st, 1);
    bool ratio_ok = st[0] == 0 && is_small(down(d_t, 4), 1, 0, n + 1);
    for (size_t k = 0; k < n; ++k) ratio_ok = ratio_ok && is_small(o, n, k, k + 1);
    // ---- refused
    const bool e_arg =
        sylow_hip_plonk_identity_batch(d_sh.as<uint64_t>(), log_n, 33, d_id.as<uint64_t>(), nullptr) == SYLOW_HIP_E_ARG &&
        sylow_hip_fr_scan_batch(d_a.as<uint64_t>(), n, 1, 2, 0, d_o.as<uint64_t>(), nullptr, nullptr) == SYLOW_HIP_E_ARG &&
        sylow_hip_fr_scan_batch_tuned(d_a.as<uint64_t>(), n, 1, 1, 0, -1, 0, d_o.as<uint64_t>(), nullptr, nullptr) == SYLOW_HIP_E_ARG &&
        sylow_hip_fr_ratio_scan_batch(nullptr, d_a.as<uint64_t>(), n, 1, 1, d_a.as<uint64_t>(), nullptr, d_st.as<uint8_t>(), nullptr) == SYLOW_HIP_E_ARG;
    printf("FRSCAN %d %d %d %d %d %d\n", ident_ok, z_ok, broken, scan_ok, ratio_ok, e_arg);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
