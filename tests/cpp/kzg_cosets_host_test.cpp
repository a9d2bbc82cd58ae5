// C++ test of the KZG proofs on every coset of the domain through the C ABI with raw device pointers (include/sylow_hip_kzg_cosets.h), at
// log_c = 3, log_l = 2: two polynomials of 32 coefficients under an SRS made with a known tau are committed (sylow::KzgProver), the table is
// built with sylow_hip_kzg_open_cosets_prepare, the 8 proofs of each come from sylow_hip_kzg_open_cosets_batch -- ONE proof per cell of 4
// values -- and the 16 rows (C, coset, cell, proof) are checked with sylow_hip_kzg_verify_cosets_batch under tau^4 G2gen.  Then one cell value
// is altered (its row alone must fail), one row names another coset (it alone fails), one names coset c (out of range), the tuned call with
// one block and four planes must give the same words, and log_c + log_l = 28 and planes_log = 3 are SYLOW_HIP_E_ARG.  Prints results for the
// pytest wrapper (tests/test_gpu_cpp_kzg_cosets.py).
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"
#include "sylow_hip_kzg_cosets.h"

using namespace sylow;

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const int32_t log_c = 3, log_l = 2;
    const size_t c = 8, l = 4, n = 32, m = 2, rows = m * c;
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    std::vector<Fp> pw(n, Fp{{1, 0, 0, 0}});
    for (size_t i = 1; i < n; ++i) pw[i] = fr::mul({pw[i - 1]}, {tau})[0];
    const std::vector<G1Affine> srs = mul(std::vector<G1Affine>(n, g1_generator()), pw);
    const std::vector<G1Affine> key_g1(srs.begin(), srs.begin() + l);
    const std::vector<G2Affine> key_g2 = mul(std::vector<G2Affine>{g2_generator()}, {pw[l]});              // tau^l G2gen
    // coefficients from a 64-bit LCG (any 256-bit words: some are >= r); coeffs [m][4][n] as the C ABI lays them out
    std::vector<std::vector<Fp>> polys(m, std::vector<Fp>(n));
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&s] { s = s * 6364136223846793005ull + 1442695040888963407ull; return s; };
    for (auto& f : polys) for (auto& v : f) for (int q = 0; q < 4; ++q) v.w[q] = next();
    std::vector<uint64_t> flat(4 * n * m);
    for (size_t j = 0; j < m; ++j) for (size_t e = 0; e < n; ++e) for (size_t w = 0; w < 4; ++w) flat[(j * 4 + w) * n + e] = polys[j][e].w[w];

    DeviceBuffer d_srs = to_device_soa(srs), d_k1 = to_device_soa(key_g1), d_k2 = to_device_soa(key_g2), d_coeffs(flat.size() * 8);
    check(sylow_hip_memcpy_h2d(d_coeffs.as<void>(), flat.data(), flat.size() * 8, nullptr), "h2d");
    DeviceBuffer d_txy(l * 2 * c * sizeof(G1Affine)), d_tinf(l * 2 * c), d_y(m * n * sizeof(Fp)), d_pi(m * c * sizeof(G1Affine)), d_pi_inf(m * c);
    DeviceBuffer d_pi2(m * c * sizeof(G1Affine)), d_pi2_inf(m * c);
    check(sylow_hip_kzg_open_cosets_prepare(d_srs.as<uint64_t>(), log_c, log_l, d_txy.as<uint64_t>(), d_tinf.as<uint8_t>(), nullptr), "sylow_hip_kzg_open_cosets_prepare");
    check(sylow_hip_kzg_open_cosets_batch(d_txy.as<uint64_t>(), d_tinf.as<uint8_t>(), d_coeffs.as<uint64_t>(), log_c, log_l, m, d_y.as<uint64_t>(), d_pi.as<uint64_t>(),
                                          d_pi_inf.as<uint8_t>(), nullptr), "sylow_hip_kzg_open_cosets_batch");
    check(sylow_hip_kzg_open_cosets_batch_tuned(d_txy.as<uint64_t>(), nullptr, d_coeffs.as<uint64_t>(), log_c, log_l, m, 1, 2, nullptr, d_pi2.as<uint64_t>(),
                                                d_pi2_inf.as<uint8_t>(), nullptr), "sylow_hip_kzg_open_cosets_batch_tuned");
    std::vector<uint64_t> y(4 * n * m), pi(8 * c * m), pi2(8 * c * m);
    check(sylow_hip_memcpy_d2h(y.data(), d_y.as<void>(), y.size() * 8, nullptr), "d2h");
    check(sylow_hip_memcpy_d2h(pi.data(), d_pi.as<void>(), pi.size() * 8, nullptr), "d2h");
    check(sylow_hip_memcpy_d2h(pi2.data(), d_pi2.as<void>(), pi2.size() * 8, nullptr), "d2h");
    check(sylow_hip_stream_sync(nullptr), "sync");
    std::vector<uint8_t> pf, pf2;
    fetch_flags(&pf, d_pi_inf, m * c);
    fetch_flags(&pf2, d_pi2_inf, m * c);
    bool pinned = pi == pi2 && pf == pf2, proper = true;
    for (const uint8_t f : pf) proper = proper && !f;

    // the rows: row j c + i is (C_j, coset i, the values y_j[i + c t], proof i of polynomial j); vals [rows][4][l], points [8][rows]
    const KzgProver prover(srs);
    const std::vector<G1Affine> commits = prover.commit(polys);
    std::vector<G1Affine> cs(rows);
    std::vector<uint64_t> idx(rows), vals(4 * l * rows), pis(8 * rows);
    for (size_t j = 0; j < m; ++j)
      for (size_t i = 0; i < c; ++i) {
        const size_t r = j * c + i;
        cs[r] = commits[j];
        idx[r] = i;
        for (size_t w = 0; w < 4; ++w) for (size_t t = 0; t < l; ++t) vals[(r * 4 + w) * l + t] = y[(j * 4 + w) * n + i + c * t];
        for (size_t w = 0; w < 8; ++w) pis[w * rows + r] = pi[(j * 8 + w) * c + i];
      }
    DeviceBuffer d_c = to_device_soa(cs), d_idx(rows * 8), d_vals(vals.size() * 8), d_pis(pis.size() * 8), d_ok(rows);
    check(sylow_hip_memcpy_h2d(d_pis.as<void>(), pis.data(), pis.size() * 8, nullptr), "h2d");
    auto verify = [&](const std::vector<uint64_t>& ix, const std::vector<uint64_t>& vv, std::vector<uint8_t>* out) {
      check(sylow_hip_memcpy_h2d(d_idx.as<void>(), ix.data(), ix.size() * 8, nullptr), "h2d");
      check(sylow_hip_memcpy_h2d(d_vals.as<void>(), vv.data(), vv.size() * 8, nullptr), "h2d");
      check(sylow_hip_kzg_verify_cosets_batch(d_k1.as<uint64_t>(), d_k2.as<uint64_t>(), d_c.as<uint64_t>(), nullptr, d_idx.as<uint64_t>(), d_vals.as<uint64_t>(), log_c,
                                              log_l, rows, d_pis.as<uint64_t>(), nullptr, d_ok.as<uint8_t>(), nullptr), "sylow_hip_kzg_verify_cosets_batch");
      fetch_flags(out, d_ok, rows);
    };
    auto only = [&](const std::vector<uint8_t>& ok, size_t bad) {          // every row holds but `bad` (rows: none)
      bool good = ok.size() == rows;
      for (size_t r = 0; good && r < rows; ++r) good = (ok[r] != 0) == (r != bad);
      return good;
    };
    std::vector<uint8_t> ok, altered, moved, outside;
    verify(idx, vals, &ok);
    std::vector<uint64_t> vals_bad = vals, idx_moved = idx, idx_out = idx;
    vals_bad[(5 * 4 + 0) * l + 2] ^= 1;                              // value 2 of row 5
    idx_moved[9] = 2;                                                // row 9 holds coset 1 of the second polynomial
    idx_out[3] = c + 3;                                              // the words of coset 3, an index that names no coset
    verify(idx, vals_bad, &altered);
    verify(idx_moved, vals, &moved);
    verify(idx_out, vals, &outside);
    const int32_t rc28 = sylow_hip_kzg_open_cosets_batch(d_txy.as<uint64_t>(), nullptr, d_coeffs.as<uint64_t>(), 14, 14, m, nullptr, d_pi2.as<uint64_t>(),
                                                         d_pi2_inf.as<uint8_t>(), nullptr);
    const int32_t rcpl = sylow_hip_kzg_open_cosets_batch_tuned(d_txy.as<uint64_t>(), nullptr, d_coeffs.as<uint64_t>(), log_c, log_l, m, -1, log_l + 1, nullptr,
                                                               d_pi2.as<uint64_t>(), d_pi2_inf.as<uint8_t>(), nullptr);
    std::printf("COSETS %d%d %d %d%d%d %d%d\n", pinned ? 1 : 0, proper ? 1 : 0, only(ok, rows) ? 1 : 0, only(altered, 5) ? 1 : 0, only(moved, 9) ? 1 : 0,
                only(outside, 3) ? 1 : 0, rc28 == SYLOW_HIP_E_ARG ? 1 : 0, rcpl == SYLOW_HIP_E_ARG ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
