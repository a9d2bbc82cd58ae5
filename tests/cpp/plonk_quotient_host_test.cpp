// C++ test of PLONK's quotient polynomial through the C ABI with raw device pointers (include/sylow_plonk.h), at log_n = 3, W = 2, E = 4: the
// prover's rounds over the library's own calls.  sigma gathered on the host from the identity columns through the mapping p -> 3 p mod 16;
// wires constant on its cycles; the selectors q_0 = i + 1, q_1 = 2 i + 3, q_M = i + 2 and the q_C that makes the gate hold, baked in; z from
// sylow_hip_plonk_permutation_batch; the coefficients from sylow_hip_fr_ntt_batch; then the table (its tail against baked words), t against
// baked words with status 0 on the default form and the tuned one, the same t through the fused kernel alone between two transforms, one
// changed wire: status 1, and the refused arguments.  The baked words are tests/plonk_quotient_model.py's
// (tests/test_gpu_cpp_plonk_quotient.py re-derives them on the CPU).  Prints results for the pytest wrapper.
#include <cstdio>
#include <cstring>

#include "sylow_hip.hpp"
#include "sylow_plonk.h"

using namespace sylow;

static const uint64_t QC[8][4] = {
    {0x43e1f593efded2d2ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0x43e1f593efd08b9full, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0x43e1f593efba4991ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0x43e1f593efb0e367ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0x43e1f593ef9a9d3bull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0x43e1f593ef85dbcdull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0x43e1f593ef748ac9ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
    {0x43e1f593ef62f3a5ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}
};
static const uint64_t ZINV[4][4] = {
    {0x75e479197177d233ull, 0xf7088036234cd1a0ull, 0xf7866dee87985c50ull, 0x0e11ae2d82f979fcull},
    {0xabca8a48c698f119ull, 0x0b56fa843968d63cull, 0xce55855b34f833fcull, 0x275afc499ab94191ull},
    {0x5d70d530665de9b1ull, 0x1aa2d637872c6707ull, 0x768388f14edd8b5bull, 0x1e0a9bf6e72dbb5bull},
    {0x090e9170467852a9ull, 0x2a28913b6b5eea60ull, 0xd8cb9d4cb669d4eaull, 0x17cbaed417a9d14bull}
};
// the coefficients 0 .. D - n = 13 of t; the other 18 are 0
static const uint64_t T[14][4] = {
    {0x01f42de5b2c189c2ull, 0x6f5b97ec021953c6ull, 0x82646c8261feaa08ull, 0x301e033ca9c45594ull},
    {0x9583e623e9bcbaa6ull, 0x3b86ca3a69be4e9bull, 0x59b66dcb670891f1ull, 0x2a09ea9c569176e2ull},
    {0x31eb4855c0c9f606ull, 0x0800eb353e8f559cull, 0x0780158bb50872d1ull, 0x0d4a76d4c32c7a80ull},
    {0x33747e2255c7a51dull, 0xafbdcf0d1df7f997ull, 0x024c769d468ff884ull, 0x2bcd92d3b0ff910eull},
    {0xf3d3cac8fb9179a0ull, 0x16c62b7d76655367ull, 0xbfc99f7828c6daacull, 0x106059b22e95fd99ull},
    {0x7420ef0cf49e4f6cull, 0x5956170eababa4afull, 0x473f1b988ac40844ull, 0x0913ff9a7aad262full},
    {0x74c09dacd1d6fe51ull, 0x5af705c1cd50fc39ull, 0xd044069e00b4cacdull, 0x1a049ef8f7807da9ull},
    {0xee25a58b31463948ull, 0x08fff5feb70162d0ull, 0x8bba3d1b91bfd499ull, 0x0b655ca342ae67d2ull},
    {0xb55f5238bb03bb24ull, 0x8e6453c41b068273ull, 0x27120b7b47d193f1ull, 0x18554eba3505c2b5ull},
    {0x020f349b5651a97bull, 0x7837c510f28b24c4ull, 0x9c8373e0f61b0ef7ull, 0x063f1c2708295ddcull},
    {0x63837be15a5f4560ull, 0x05f4505fa1a4fbd9ull, 0xc6dca69586850bcfull, 0x06cde162fc1adef3ull},
    {0x73ae9cec359a8358ull, 0x93fd8140bfd30306ull, 0x38e6bcedfb25a5c8ull, 0x2d1d5e591779f757ull},
    {0x0811c6433a07fc40ull, 0x34c325e0572dc281ull, 0xa5920d7f74424ccaull, 0x27b2a60ffc14c994ull},
    {0xbe59ab97f9df6923ull, 0xaad8ffbbdf4ae64dull, 0x5c7e991644b44308ull, 0x15dbb685ea0b3a70ull}
};

static void up(DeviceBuffer& d, const std::vector<uint64_t>& v) { check(sylow_hip_memcpy_h2d(d.as<void>(), v.data(), v.size() * 8, nullptr), "h2d"); }
static std::vector<uint64_t> down(DeviceBuffer& d, size_t words, size_t first = 0) {
  std::vector<uint64_t> v(words);
  check(sylow_hip_memcpy_d2h(v.data(), d.as<uint64_t>() + first, words * 8, nullptr), "d2h");
  check(sylow_hip_stream_sync(nullptr), "sync");
  return v;
}
// soa [4][stride]: element i against want[i] for i < N, and zeros from N up to stride
template <size_t N> static bool same(const std::vector<uint64_t>& soa, const uint64_t (&want)[N][4], size_t stride) {
  bool ok = soa.size() == 4 * stride;
  for (size_t i = 0; ok && i < stride; ++i)
    for (size_t w = 0; w < 4; ++w) ok = ok && soa[w * stride + i] == (i < N ? want[i][w] : 0);
  return ok;
}

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const int32_t log_n = 3, log_e = 2, W = 2;
    const size_t n = 8, N = 32, E = 4, m = 1, rows = 2 * W + 3, table_words = 4 * N * rows + 4 * E;
    uint64_t* const null = nullptr;
    // ---- the circuit: identity columns, sigma through the mapping, the selectors
    const std::vector<uint64_t> shifts = {1, 5, 0, 0, 0, 0, 0, 0};          // [4][W]
    DeviceBuffer d_sh(4 * W * 8), d_id(W * 4 * n * 8), d_sg(W * 4 * n * 8), d_sel((W + 2) * 4 * n * 8);
    up(d_sh, shifts);
    check(sylow_hip_plonk_identity_batch(d_sh.as<uint64_t>(), log_n, W, d_id.as<uint64_t>(), nullptr), "sylow_hip_plonk_identity_batch");
    const std::vector<uint64_t> ident = down(d_id, W * 4 * n);
    std::vector<uint64_t> sigma(W * 4 * n), wires(W * 4 * n, 0), sel((W + 2) * 4 * n, 0);
    const uint64_t cycle_of[16] = {0, 1, 2, 1, 3, 4, 2, 4, 5, 1, 6, 1, 3, 4, 6, 4};      // the cycles of p -> 3 p mod 16, numbered by their least position
    for (size_t p = 0; p < 16; ++p) {
      const size_t q = p * 3 % 16;
      for (size_t w = 0; w < 4; ++w) sigma[(p / n * 4 + w) * n + p % n] = ident[(q / n * 4 + w) * n + q % n];
      wires[(p / n * 4) * n + p % n] = 1000 + 17 * cycle_of[p];
    }
    for (size_t i = 0; i < n; ++i) {
      sel[(0 * 4) * n + i] = i + 1;                                          // q_0
      sel[(1 * 4) * n + i] = 2 * i + 3;                                      // q_1
      sel[(2 * 4) * n + i] = i + 2;                                          // q_M
      for (size_t w = 0; w < 4; ++w) sel[(3 * 4 + w) * n + i] = QC[i][w];    // q_C = -(q_M w_0 w_1 + q_0 w_0 + q_1 w_1)
    }
    up(d_sg, sigma); up(d_sel, sel);
    DeviceBuffer d_table(table_words * 8);
    check(sylow_plonk_quotient_prepare(d_sel.as<uint64_t>(), d_sg.as<uint64_t>(), log_n, log_e, W, d_table.as<uint64_t>(), nullptr), "sylow_plonk_quotient_prepare");
    const bool table_ok = same(down(d_table, 4 * E, 4 * N * rows), ZINV, E);
    // ---- round 2: z; then the coefficients of the wires and of z
    const std::vector<uint64_t> beta = {0x1234567, 0, 0, 0}, gamma = {0x89ABCDEF, 0, 0, 0}, alpha = {0x13579BDF, 0, 0, 0};
    DeviceBuffer d_w(W * 4 * n * 8), d_b(32), d_g(32), d_a(32), d_z(4 * n * 8), d_wc(W * 4 * n * 8), d_zc(4 * n * 8), d_t(4 * N * 8), d_st(1);
    up(d_w, wires); up(d_b, beta); up(d_g, gamma); up(d_a, alpha);
    check(sylow_hip_plonk_permutation_batch(d_w.as<uint64_t>(), d_sg.as<uint64_t>(), d_sh.as<uint64_t>(), d_b.as<uint64_t>(), d_g.as<uint64_t>(), log_n, W, m,
                                            d_z.as<uint64_t>(), nullptr, d_st.as<uint8_t>(), nullptr), "sylow_hip_plonk_permutation_batch");
    std::vector<uint8_t> st;
    fetch_flags(&st, d_st, 1);
    const bool z_ok = st[0] == 0;
    check(sylow_hip_fr_ntt_batch(d_w.as<uint64_t>(), log_n, W, 1, nullptr, d_wc.as<uint64_t>(), nullptr), "sylow_hip_fr_ntt_batch");
    check(sylow_hip_fr_ntt_batch(d_z.as<uint64_t>(), log_n, 1, 1, nullptr, d_zc.as<uint64_t>(), nullptr), "sylow_hip_fr_ntt_batch");
    // ---- round 3: t, on the default form and the tuned one
    bool t_ok = true;
    for (int tuned = 0; tuned < 2; ++tuned) {
      const int32_t rc = tuned ? sylow_plonk_quotient_batch_tuned(d_table.as<uint64_t>(), d_wc.as<uint64_t>(), n, d_zc.as<uint64_t>(), n, null, d_sh.as<uint64_t>(),
                                                                  d_b.as<uint64_t>(), d_g.as<uint64_t>(), d_a.as<uint64_t>(), log_n, log_e, W, m, 1, d_t.as<uint64_t>(),
                                                                  d_st.as<uint8_t>(), nullptr)
                               : sylow_plonk_quotient_batch(d_table.as<uint64_t>(), d_wc.as<uint64_t>(), n, d_zc.as<uint64_t>(), n, null, d_sh.as<uint64_t>(),
                                                            d_b.as<uint64_t>(), d_g.as<uint64_t>(), d_a.as<uint64_t>(), log_n, log_e, W, m, d_t.as<uint64_t>(),
                                                            d_st.as<uint8_t>(), nullptr);
      check(rc, "sylow_plonk_quotient_batch");
      fetch_flags(&st, d_st, 1);
      t_ok = t_ok && same(down(d_t, 4 * N), T, N) && st[0] == 0;
    }
    // ---- the same t through the fused kernel alone: the columns padded and taken onto K, t_ext, and back
    std::vector<uint64_t> padded((W + 1) * 4 * N, 0);
    const std::vector<uint64_t> wc = down(d_wc, W * 4 * n), zc = down(d_zc, 4 * n);
    for (size_t c = 0; c < (size_t)W + 1; ++c)
      for (size_t w = 0; w < 4; ++w)
        for (size_t i = 0; i < n; ++i) padded[(c * 4 + w) * N + i] = c < (size_t)W ? wc[(c * 4 + w) * n + i] : zc[w * n + i];
    const std::vector<uint64_t> five = {5, 0, 0, 0};
    DeviceBuffer d_pad((W + 1) * 4 * N * 8), d_ext((W + 1) * 4 * N * 8), d_five(32), d_text(4 * N * 8);
    up(d_pad, padded); up(d_five, five);
    check(sylow_hip_fr_ntt_batch(d_pad.as<uint64_t>(), log_n + log_e, W + 1, 0, d_five.as<uint64_t>(), d_ext.as<uint64_t>(), nullptr), "sylow_hip_fr_ntt_batch");
    check(sylow_plonk_quotient_evals_batch(d_table.as<uint64_t>(), d_ext.as<uint64_t>(), d_ext.as<uint64_t>() + W * 4 * N, null, d_sh.as<uint64_t>(), d_b.as<uint64_t>(),
                                           d_g.as<uint64_t>(), d_a.as<uint64_t>(), log_n, log_e, W, m, d_text.as<uint64_t>(), nullptr),
          "sylow_plonk_quotient_evals_batch");
    check(sylow_hip_fr_ntt_batch(d_text.as<uint64_t>(), log_n + log_e, 1, 1, d_five.as<uint64_t>(), d_t.as<uint64_t>(), nullptr), "sylow_hip_fr_ntt_batch");
    const bool evals_ok = same(down(d_t, 4 * N), T, N);
    // ---- one changed wire under the same z: X^n - 1 does not divide
    wires[3] += 1;
    up(d_w, wires);
    check(sylow_hip_fr_ntt_batch(d_w.as<uint64_t>(), log_n, W, 1, nullptr, d_wc.as<uint64_t>(), nullptr), "sylow_hip_fr_ntt_batch");
    check(sylow_plonk_quotient_batch(d_table.as<uint64_t>(), d_wc.as<uint64_t>(), n, d_zc.as<uint64_t>(), n, null, d_sh.as<uint64_t>(), d_b.as<uint64_t>(),
                                     d_g.as<uint64_t>(), d_a.as<uint64_t>(), log_n, log_e, W, m, d_t.as<uint64_t>(), d_st.as<uint8_t>(), nullptr),
          "sylow_plonk_quotient_batch");
    fetch_flags(&st, d_st, 1);
    const bool broken = st[0] == 1;
    // ---- refused: W = 1, log_n + log_e = 29, len_z = 27 (D - n = N), max_blocks = 0, t_out over the wires
    auto full = [&](int32_t lg, int32_t le, int32_t w, size_t len_z, uint64_t* t_out) {
      return sylow_plonk_quotient_batch(d_table.as<uint64_t>(), d_wc.as<uint64_t>(), n, d_zc.as<uint64_t>(), len_z, null, d_sh.as<uint64_t>(), d_b.as<uint64_t>(),
                                        d_g.as<uint64_t>(), d_a.as<uint64_t>(), lg, le, w, m, t_out, d_st.as<uint8_t>(), nullptr);
    };
    const bool e_arg =
        full(log_n, log_e, 1, n, d_t.as<uint64_t>()) == SYLOW_HIP_E_ARG && full(27, 2, W, n, d_t.as<uint64_t>()) == SYLOW_HIP_E_ARG &&
        full(log_n, log_e, W, 27, d_t.as<uint64_t>()) == SYLOW_HIP_E_ARG && full(log_n, log_e, W, n, d_wc.as<uint64_t>()) == SYLOW_HIP_E_ARG &&
        sylow_plonk_quotient_evals_batch_tuned(d_table.as<uint64_t>(), d_ext.as<uint64_t>(), d_ext.as<uint64_t>() + W * 4 * N, null, d_sh.as<uint64_t>(), d_b.as<uint64_t>(),
                                               d_g.as<uint64_t>(), d_a.as<uint64_t>(), log_n, log_e, W, m, 0, d_text.as<uint64_t>(), nullptr) == SYLOW_HIP_E_ARG &&
        sylow_plonk_quotient_prepare(d_sel.as<uint64_t>(), d_sg.as<uint64_t>(), log_n, log_e, 33, d_table.as<uint64_t>(), nullptr) == SYLOW_HIP_E_ARG;
    printf("PLONKQ %d %d %d %d %d %d\n", table_ok, z_ok, t_ok, evals_ok, broken, e_arg);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
