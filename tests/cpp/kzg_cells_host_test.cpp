// C++ test of the check of many cells of many blobs as one boolean through the C ABI with raw device pointers
// (include/sylow_hip_kzg_cells.h), at log_c = 2, log_l = 2.  First the Fr half on seven rows of small integers against words baked in from
// tests/kzg_cells_model.py (tests/test_gpu_cpp_kzg_cells.py checks the tables against the model on the CPU): the default form and both
// pinned routes.  Then two polynomials of 16 coefficients under an SRS made with a known tau are committed and opened on every coset, and
// the eight rows go through sylow_hip_kzg_cells_verify_weighted under tau^4 G2gen: accepted; one value altered: rejected, and accepted
// again with that row's weight 0; a row that names no cell: the range flag clear; the reduction's row (F, 0, 0, P) through
// sylow_hip_kzg_verify_batch; log_c + log_l = 28 and route = 2 are SYLOW_HIP_E_ARG.  Prints results for the pytest wrapper.
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"
#include "sylow_hip_kzg_cells.h"
#include "sylow_hip_kzg_cosets.h"

using namespace sylow;

static const uint64_t W[2][4] = {
    {0x00000000003d092eull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x00000000005b8db4ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}
};
static const uint64_t A[4][4] = {
    {0x0000008a4bad7d0full, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x69d083e9a2c3fe8aull, 0x1794173dd2b8c9c8ull, 0x8a5275bc02939e2bull, 0x2bcf5cf4eeff79faull},
    {0xaaeedcb7d7f799dcull, 0xbc737388c8f53f0eull, 0x522274671383b20cull, 0x1ca4dab78f9ca2feull},
    {0x1d8539f9e48b5c18ull, 0xe7a95b6ca6e21afeull, 0x3acaa5cc3d86d3b8ull, 0x12bcfcb28973782aull}
};
static const uint64_t RZ[7][4] = {
    {0x00000000000f4254ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x6ebf2b1231594d44ull, 0x536f1eef86adb5e1ull, 0xeb9a5048da52f786ull, 0x30644e72e11c31fcull},
    {0x1b15477e06cc2723ull, 0xa8ffb677ad7b0005ull, 0x7d487e4ab4d90d8dull, 0x30644e72e1117aecull},
    {0x7c7691aa13c0feffull, 0x29a39a48a5712668ull, 0xa9599969f22234c8ull, 0x00000000002adc4dull},
    {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}
};

template <size_t N> static bool same(const std::vector<uint64_t>& soa, const uint64_t (&want)[N][4]) {      // soa: [4][N]
  bool ok = soa.size() == 4 * N;
  for (size_t i = 0; ok && i < N; ++i) for (size_t w = 0; w < 4; ++w) ok = ok && soa[w * N + i] == want[i][w];
  return ok;
}
static void up(DeviceBuffer& d, const std::vector<uint64_t>& v) { check(sylow_hip_memcpy_h2d(d.as<void>(), v.data(), v.size() * 8, nullptr), "h2d"); }
static std::vector<uint64_t> down(DeviceBuffer& d, size_t words) {
  std::vector<uint64_t> v(words);
  check(sylow_hip_memcpy_d2h(v.data(), d.as<void>(), words * 8, nullptr), "d2h");
  check(sylow_hip_stream_sync(nullptr), "sync");
  return v;
}

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const int32_t log_c = 2, log_l = 2;
    const size_t c = 4, l = 4, n = 16;
    // ---- the Fr half: rows k < 7 of (idx, com, vals[j] = 7919 (k + 1)(j + 1) + j^2 + 1, weight 1000003 (k + 1) + 17), the last weight 0;
    // row 4 names commitment 2 of 2 and row 5 cell 4 of 4: dropped, and the flag is clear
    const size_t fr_rows = 7, fr_com = 2;
    const std::vector<uint64_t> f_idx = {0, 1, 1, 3, 2, 4, 1}, f_cm = {0, 1, 0, 1, 2, 0, 1};
    std::vector<uint64_t> f_vals(4 * l * fr_rows, 0), f_wt(4 * fr_rows, 0);
    for (size_t k = 0; k < fr_rows; ++k) {
      for (size_t j = 0; j < l; ++j) f_vals[(k * 4 + 0) * l + j] = 7919 * (k + 1) * (j + 1) + j * j + 1;
      f_wt[k] = k == 6 ? 0 : 1000003 * (k + 1) + 17;
    }
    DeviceBuffer d_fi(fr_rows * 8), d_fc(fr_rows * 8), d_fv(f_vals.size() * 8), d_fw(f_wt.size() * 8);
    DeviceBuffer d_w(4 * fr_com * 8), d_a(4 * l * 8), d_r(4 * fr_rows * 8), d_rz(4 * fr_rows * 8), d_flag(1);
    up(d_fi, f_idx); up(d_fc, f_cm); up(d_fv, f_vals); up(d_fw, f_wt);
    bool fold_ok = true;
    for (int route = -1; route <= 1; ++route) {
      const int32_t rc = route < 0 ? sylow_hip_kzg_cells_fold_batch(d_fi.as<uint64_t>(), d_fc.as<uint64_t>(), d_fv.as<uint64_t>(), d_fw.as<uint64_t>(), log_c, log_l, fr_rows,
                                                                    fr_com, d_w.as<uint64_t>(), d_a.as<uint64_t>(), d_r.as<uint64_t>(), d_rz.as<uint64_t>(),
                                                                    d_flag.as<uint8_t>(), nullptr)
                                   : sylow_hip_kzg_cells_fold_batch_tuned(d_fi.as<uint64_t>(), d_fc.as<uint64_t>(), d_fv.as<uint64_t>(), d_fw.as<uint64_t>(), log_c, log_l,
                                                                          fr_rows, fr_com, route, 1, d_w.as<uint64_t>(), d_a.as<uint64_t>(), d_r.as<uint64_t>(),
                                                                          d_rz.as<uint64_t>(), d_flag.as<uint8_t>(), nullptr);
      check(rc, "sylow_hip_kzg_cells_fold_batch");
      const std::vector<uint64_t> r = down(d_r, 4 * fr_rows);
      bool weights = true;
      for (size_t k = 0; k < fr_rows; ++k) weights = weights && r[k] == (k < 4 ? f_wt[k] : 0) && !r[fr_rows + k] && !r[2 * fr_rows + k] && !r[3 * fr_rows + k];
      std::vector<uint8_t> flag;
      fetch_flags(&flag, d_flag, 1);
      fold_ok = fold_ok && weights && same(down(d_w, 4 * fr_com), W) && same(down(d_a, 4 * l), A) && same(down(d_rz, 4 * fr_rows), RZ) && flag[0] == 0;
    }

    // ---- the whole check on real openings
    const size_t m = 2, rows = m * c;
    const Fp tau{{0x0123456789ABCDEFull, 0x0FEDCBA987654321ull, 0x1122334455667788ull, 0x0099AABBCCDDEEFFull}};
    std::vector<Fp> pw(n, Fp{{1, 0, 0, 0}});
    for (size_t i = 1; i < n; ++i) pw[i] = fr::mul({pw[i - 1]}, {tau})[0];
    const std::vector<G1Affine> srs = mul(std::vector<G1Affine>(n, g1_generator()), pw);
    const std::vector<G1Affine> key_g1(srs.begin(), srs.begin() + l);
    const std::vector<G2Affine> key_g2 = mul(std::vector<G2Affine>{g2_generator()}, {pw[l]});              // tau^l G2gen
    std::vector<std::vector<Fp>> polys(m, std::vector<Fp>(n));
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&s] { s = s * 6364136223846793005ull + 1442695040888963407ull; return s; };
    for (auto& f : polys) for (auto& v : f) for (int q = 0; q < 4; ++q) v.w[q] = next();
    std::vector<uint64_t> flat(4 * n * m);
    for (size_t j = 0; j < m; ++j) for (size_t e = 0; e < n; ++e) for (size_t w = 0; w < 4; ++w) flat[(j * 4 + w) * n + e] = polys[j][e].w[w];
    DeviceBuffer d_srs = to_device_soa(srs), d_k1 = to_device_soa(key_g1), d_k2 = to_device_soa(key_g2), d_coeffs(flat.size() * 8);
    up(d_coeffs, flat);
    DeviceBuffer d_txy(l * 2 * c * sizeof(G1Affine)), d_tinf(l * 2 * c), d_y(m * n * sizeof(Fp)), d_pi(m * c * sizeof(G1Affine)), d_pi_inf(m * c);
    check(sylow_hip_kzg_open_cosets_prepare(d_srs.as<uint64_t>(), log_c, log_l, d_txy.as<uint64_t>(), d_tinf.as<uint8_t>(), nullptr), "sylow_hip_kzg_open_cosets_prepare");
    check(sylow_hip_kzg_open_cosets_batch(d_txy.as<uint64_t>(), d_tinf.as<uint8_t>(), d_coeffs.as<uint64_t>(), log_c, log_l, m, d_y.as<uint64_t>(), d_pi.as<uint64_t>(),
                                          d_pi_inf.as<uint8_t>(), nullptr), "sylow_hip_kzg_open_cosets_batch");
    const std::vector<uint64_t> y = down(d_y, 4 * n * m), pi = down(d_pi, 8 * c * m);
    const KzgProver prover(srs);
    DeviceBuffer d_c = to_device_soa(prover.commit(polys));                                                 // [8][m]: ONE commitment per blob
    // row j c + i is (commitment j, cell i, the values y_j[i + c t], proof i of polynomial j); weights of 128 bits
    std::vector<uint64_t> idx(rows), cm(rows), vals(4 * l * rows), pis(8 * rows), wt(4 * rows, 0);
    for (size_t j = 0; j < m; ++j)
      for (size_t i = 0; i < c; ++i) {
        const size_t r = j * c + i;
        idx[r] = i;
        cm[r] = j;
        for (size_t w = 0; w < 4; ++w) for (size_t t = 0; t < l; ++t) vals[(r * 4 + w) * l + t] = y[(j * 4 + w) * n + i + c * t];
        for (size_t w = 0; w < 8; ++w) pis[w * rows + r] = pi[(j * 8 + w) * c + i];
        wt[r] = next() | 1;
        wt[rows + r] = next();
      }
    DeviceBuffer d_idx(rows * 8), d_cm(rows * 8), d_vals(vals.size() * 8), d_pis(pis.size() * 8), d_wt(wt.size() * 8), d_gt(48 * 8), d_one(1), d_rng(1);
    up(d_cm, cm); up(d_pis, pis);
    auto verify = [&](const std::vector<uint64_t>& ix, const std::vector<uint64_t>& vv, const std::vector<uint64_t>& ww, bool* in_range) {
      up(d_idx, ix); up(d_vals, vv); up(d_wt, ww);
      check(sylow_hip_kzg_cells_verify_weighted(d_k1.as<uint64_t>(), d_k2.as<uint64_t>(), d_c.as<uint64_t>(), nullptr, d_idx.as<uint64_t>(), d_cm.as<uint64_t>(),
                                                d_vals.as<uint64_t>(), d_pis.as<uint64_t>(), nullptr, d_wt.as<uint64_t>(), log_c, log_l, rows, m, d_gt.as<uint64_t>(),
                                                d_one.as<uint8_t>(), d_rng.as<uint8_t>(), nullptr), "sylow_hip_kzg_cells_verify_weighted");
      std::vector<uint8_t> one, rng;
      fetch_flags(&one, d_one, 1);
      fetch_flags(&rng, d_rng, 1);
      if (in_range) *in_range = rng[0] != 0;
      return one[0] != 0;
    };
    bool rng_ok = false, rng_alt = false, rng_out = false;
    const bool accepted = verify(idx, vals, wt, &rng_ok);
    std::vector<uint64_t> vals_bad = vals, wt_masked = wt, idx_out = idx;
    vals_bad[(5 * 4 + 0) * l + 2] ^= 1;                              // value 2 of row 5
    wt_masked[5] = wt_masked[rows + 5] = 0;
    idx_out[3] = c + 3;
    const bool altered = verify(idx, vals_bad, wt, &rng_alt), masked = verify(idx, vals_bad, wt_masked, nullptr), outside = verify(idx_out, vals, wt, &rng_out);
    // the reduction's one row under the single-point verifier
    up(d_idx, idx); up(d_vals, vals); up(d_wt, wt);
    DeviceBuffer d_f(64), d_finf(1), d_p(64), d_pinf(1), d_zero(32), d_ok(1);
    up(d_zero, std::vector<uint64_t>(4, 0));
    check(sylow_hip_kzg_cells_reduce_batch(d_k1.as<uint64_t>(), d_c.as<uint64_t>(), nullptr, d_idx.as<uint64_t>(), d_cm.as<uint64_t>(), d_vals.as<uint64_t>(),
                                           d_pis.as<uint64_t>(), nullptr, d_wt.as<uint64_t>(), log_c, log_l, rows, m, d_f.as<uint64_t>(), d_finf.as<uint8_t>(),
                                           d_p.as<uint64_t>(), d_pinf.as<uint8_t>(), d_rng.as<uint8_t>(), nullptr), "sylow_hip_kzg_cells_reduce_batch");
    check(sylow_hip_kzg_verify_batch(d_k2.as<uint64_t>(), d_f.as<uint64_t>(), d_finf.as<uint8_t>(), d_zero.as<uint64_t>(), d_zero.as<uint64_t>(), d_p.as<uint64_t>(),
                                     d_pinf.as<uint8_t>(), d_ok.as<uint8_t>(), 1, nullptr), "sylow_hip_kzg_verify_batch");
    std::vector<uint8_t> row_ok;
    fetch_flags(&row_ok, d_ok, 1);
    const int32_t rc28 = sylow_hip_kzg_cells_verify_weighted(d_k1.as<uint64_t>(), d_k2.as<uint64_t>(), d_c.as<uint64_t>(), nullptr, d_idx.as<uint64_t>(), d_cm.as<uint64_t>(),
                                                             d_vals.as<uint64_t>(), d_pis.as<uint64_t>(), nullptr, d_wt.as<uint64_t>(), 14, 14, rows, m, d_gt.as<uint64_t>(),
                                                             d_one.as<uint8_t>(), nullptr, nullptr);
    const int32_t rcrt = sylow_hip_kzg_cells_fold_batch_tuned(d_fi.as<uint64_t>(), d_fc.as<uint64_t>(), d_fv.as<uint64_t>(), d_fw.as<uint64_t>(), log_c, log_l, fr_rows, fr_com,
                                                              2, -1, d_w.as<uint64_t>(), d_a.as<uint64_t>(), d_r.as<uint64_t>(), d_rz.as<uint64_t>(), d_flag.as<uint8_t>(),
                                                              nullptr);
    std::printf("CELLS %d %d%d %d%d%d %d%d %d %d%d\n", fold_ok ? 1 : 0, accepted ? 1 : 0, rng_ok ? 1 : 0, altered ? 1 : 0, rng_alt ? 1 : 0, masked ? 1 : 0,
                outside ? 1 : 0, rng_out ? 1 : 0, row_ok[0] ? 1 : 0, rc28 == SYLOW_HIP_E_ARG ? 1 : 0, rcrt == SYLOW_HIP_E_ARG ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
