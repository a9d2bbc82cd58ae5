// C++ host-layer test of sylow::fr::spmv, sylow::groth16_quotient and sylow::groth16_prove (include/sylow_hip.hpp) on a circuit of 3 constraints
// over 5 variables (n = 4, one public input) under a key of random generator multiples: the sparse product against fr::mul / fr::add, the
// quotient's top coefficient for a b = c, and A, B, C of two witnesses against the same sums composed from sylow::msm, g2_msm, mul, sum and sub.
// The key comes from no setup, so the proofs are compared with the formulas, not verified.  Prints results for the pytest wrapper
// (tests/test_gpu_cpp_groth16_prove.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"

using namespace sylow;

static uint64_t lcg = 0x9E3779B97F4A7C15ull;
static Fp word() {
  Fp c;
  for (int q = 0; q < 4; ++q) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; c.w[q] = lcg; }
  return c;
}
static std::vector<Fp> words(size_t n) {
  std::vector<Fp> v(n);
  for (auto& c : v) c = word();
  return v;
}
template <class T> static bool same(const T& a, const T& b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }
static std::vector<Fp> canonical(const std::vector<Fp>& a) { return fr::add(a, std::vector<Fp>(a.size(), Fp{{0, 0, 0, 0}})); }

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const size_t n = 4, n_vars = 5, l = 1, m = 2;
    Groth16Circuit ct;
    ct.n_vars = n_vars; ct.n_inputs = l; ct.log_n = 2;
    for (CsrMatrix* mat : {&ct.a, &ct.b, &ct.c})
      for (size_t i = 0; i < 3; ++i) mat->add_row({{i, word()}, {(i + 2) % n_vars, word()}, {4, word()}});
    std::vector<std::vector<Fp>> z = {words(n_vars), words(n_vars)};
    const std::vector<Fp> r = words(m), s = words(m), rc = canonical(r), sc = canonical(s), rs = fr::mul(r, s);
    // the sparse product: row 1 of A z_0 by hand, and the padding row
    const auto az = fr::spmv(ct.a, z, n), bz = fr::spmv(ct.b, z, n), cz = fr::spmv(ct.c, z, n);
    const std::vector<Fp> t = fr::mul({ct.a.val[3], ct.a.val[4], ct.a.val[5]}, {z[0][1], z[0][3], z[0][4]});
    const Fp row1 = fr::add(fr::add({t[0]}, {t[1]}), {t[2]})[0];
    const bool spmv_ok = same(az[0][1], row1) && same(az[0][3], Fp{{0, 0, 0, 0}}) && same(fr::spmv(ct.a, z, n, 3)[1][2], az[1][2]);
    // the quotient: exact for a b = c, so its top coefficient is zero; and the quotient of the circuit's three products
    const auto ab = std::vector<std::vector<Fp>>{fr::mul(az[0], bz[0]), fr::mul(az[1], bz[1])};
    const auto hx = groth16_quotient(az, bz, ab);
    const bool quot_ok = same(hx[0][n - 1], Fp{{0, 0, 0, 0}}) && same(hx[1][n - 1], Fp{{0, 0, 0, 0}}) && !same(hx[0][0], Fp{{0, 0, 0, 0}});
    const auto h = groth16_quotient(az, bz, cz);
    // a key of random generator multiples
    auto g1s = [](size_t k) { return mul(std::vector<G1Affine>(k, g1_generator()), canonical(words(k))); };
    auto g2s = [](size_t k) { return mul(std::vector<G2Affine>(k, g2_generator()), canonical(words(k))); };
    Groth16ProvingKey pk;
    pk.alpha_g1 = g1s(1)[0]; pk.beta_g1 = g1s(1)[0]; pk.delta_g1 = g1s(1)[0]; pk.beta_g2 = g2s(1)[0]; pk.delta_g2 = g2s(1)[0];
    pk.a_query = g1s(n_vars); pk.b_g1_query = g1s(n_vars); pk.b_g2_query = g2s(n_vars); pk.h_query = g1s(n - 1); pk.l_query = g1s(n_vars - l - 1);
    const Groth16Proofs pr = groth16_prove(pk, ct, z, r, s);
    bool a_ok = pr.a.size() == m, b_ok = pr.b.size() == m, c_ok = pr.c.size() == m;
    for (size_t j = 0; j < m && a_ok && b_ok && c_ok; ++j) {
      const std::vector<Fp> zc = canonical(z[j]);
      const G1Affine a = sum({pk.alpha_g1, msm(pk.a_query, zc), mul({pk.delta_g1}, {rc[j]})[0]});
      const G1Affine b1 = sum({pk.beta_g1, msm(pk.b_g1_query, zc), mul({pk.delta_g1}, {sc[j]})[0]});
      const G2Affine b = g2_sum({pk.beta_g2, g2_msm(pk.b_g2_query, zc), mul({pk.delta_g2}, {sc[j]})[0]});
      const G1Affine pos = sum({msm(pk.l_query, std::vector<Fp>(zc.begin() + l + 1, zc.end())), msm(pk.h_query, std::vector<Fp>(h[j].begin(), h[j].end() - 1)),
                                mul({a}, {sc[j]})[0], mul({b1}, {rc[j]})[0]});
      const G1Affine c = sub({pos}, {mul({pk.delta_g1}, {rs[j]})[0]})[0];
      a_ok = same(pr.a[j], a) && !pr.a_inf[j];
      b_ok = same(pr.b[j], b) && !pr.b_inf[j];
      c_ok = same(pr.c[j], c) && !pr.c_inf[j];
    }
    std::printf("G16 %d%d%d%d%d\n", spmv_ok ? 1 : 0, quot_ok ? 1 : 0, a_ok ? 1 : 0, b_ok ? 1 : 0, c_ok ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
