// C++ test of the recovery of a KZG polynomial from half of its cells through the C ABI with raw device pointers
// (include/sylow_hip_kzg_recover.h), at log_c = 2, log_l = 2, m = 2, against values baked in from tests/kzg_recover_model.py.
// The blobs are f_j[k] = (j + 1) 1000003 + 7919 k^2 + 1 for k < 8 and 0 above; Y holds their 16 values each.  Row 0 misses cell 1, row 1
// misses cells 0 and 3 (exactly half); the words of missing cells are all-ones.  Checked: the vanishing values (ZD, ZC), the recovered
// coefficients and status 0, y_out = Y with the missing cells restored; then Y[0][4] + 1 in row 0 (status 2, coefficients BAD) and
// Y[1][5] + 1 in row 1 (status 0, the other polynomial OTHER); a third mask of three missing cells (status 1, zero row); and
// (log_c, log_l) = (13, 0) and (0, 0) are SYLOW_HIP_E_ARG.  Prints results for the pytest wrapper (tests/test_gpu_cpp_kzg_recover.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "sylow_hip.hpp"
#include "sylow_hip_kzg_recover.h"

using namespace sylow;

static const uint64_t Y[32][4] = {
    {0x00000000008AFCD4ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x0EC8238D4996FAF4ull, 0x9B00BFAD94404CF9ull, 0xEC29271F81054983ull, 0x2470E75044D805C7ull},
    {0x62E9173E121549D2ull, 0x3066F102DE7C5E39ull, 0xDC4AD29DFDCCB0A0ull, 0x1D8BB51F1431B990ull},
    {0xB3E925808011210Dull, 0x906D8BC8884C200Dull, 0x0E9F8F9F83F23EF1ull, 0x0177F0B5A1807FDEull},
    {0x0C88AAFFFC62EA38ull, 0xD81CB4673D360040ull, 0xC1373043B326770Dull, 0x000000000002B71Cull},
    {0xA58CC53603F9EDF5ull, 0x954A8AFD30A4C231ull, 0x062F4341DAAB3426ull, 0x15D2A83EB235E659ull},
    {0x116C099C40CC81E0ull, 0x79FDF970DE0C85F3ull, 0x70BEDF4665F31424ull, 0x10403FA4063BD1B5ull},
    {0xB7D0BCFB004FC8F0ull, 0xF520F2B16969E98Cull, 0xDC37AF1B62A5373Bull, 0x18136CC627D99257ull},
    {0x43E1F593EFFC9DDDull, 0x2833E84879B97091ull, 0xB85045B68181585Dull, 0x30644E72E131A029ull},
    {0xFCD55E6B9408EB49ull, 0x96322582248EA6C1ull, 0x955D13DB2C32C2E5ull, 0x013AD3AEA012BD33ull},
    {0xFA0A3455D6B2798Full, 0xA806601415A912D7ull, 0x5E73D39FEA0195D8ull, 0x12D89953CD0554D2ull},
    {0xE079EE49F4C2C0E7ull, 0x186DC4209F27ACBAull, 0x69D5B7DA70D021FCull, 0x28FD51C29A2AD3F9ull},
    {0x37594A93F39748F9ull, 0x501733E13C837051ull, 0xF7191572CE5AE14Full, 0x30644E72E12EE90Cull},
    {0xEBA0FB1AD963D3F0ull, 0x02CC487039B040AFull, 0xDE22063B78467CC9ull, 0x254A39A82B124C80ull},
    {0x196495F7B663FF01ull, 0xFDFC86092140EA1Eull, 0xC52305E8B541561Cull, 0x20240ECEDAF0603Aull},
    {0x2688C3409058BF1Eull, 0x3989A5EA32E41553ull, 0x26BC9BCCAE740BF2ull, 0x1E3FEDA75F0EA4A2ull},
    {0x0000000001050EECull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x69645AAB25414102ull, 0x1EE0803E9F04D3F6ull, 0x8CA37EA4024994ACull, 0x22B7158845D0DC3Bull},
    {0x62E9173E121549D2ull, 0x3066F102DE7C5E39ull, 0xDC4AD29DFDCCB0A0ull, 0x1D8BB51F1431B990ull},
    {0x8934DACFCE9C3BE2ull, 0x8E0D4B7D068D5222ull, 0xE6CFF43962A3AD2Aull, 0x2B0109F530909154ull},
    {0x0C88AAFFFC62EA38ull, 0xD81CB4673D360040ull, 0xC1373043B326770Dull, 0x000000000002B71Cull},
    {0xFCCE5DCD5887DAC6ull, 0x005B1C0E857B12F3ull, 0x0945C88B8A230941ull, 0x1EE383CC6AA6B0BBull},
    {0x116C099C40CC81E0ull, 0x79FDF970DE0C85F3ull, 0x70BEDF4665F31424ull, 0x10403FA4063BD1B5ull},
    {0x26EC5B457C31797Full, 0xB8630EC72947D73Aull, 0x192FB4FECC18E985ull, 0x2645ABBF338F9E22ull},
    {0x43E1F593EFFC9DDDull, 0x2833E84879B97091ull, 0xB85045B68181585Dull, 0x30644E72E131A029ull},
    {0xD19BB5B50845BF41ull, 0xFB23F1B4DE6A29A5ull, 0x10B553AE444068F8ull, 0x236CE328758E5193ull},
    {0xFA0A3455D6B2798Full, 0xA806601415A912D7ull, 0x5E73D39FEA0195D8ull, 0x12D89953CD0554D2ull},
    {0x893855B2A053589Cull, 0xAD5D330F4A515BF8ull, 0x66BF3290C1584CE1ull, 0x1FEC7634E1BA0997ull},
    {0x37594A93F39748F9ull, 0x501733E13C837051ull, 0xF7191572CE5AE14Full, 0x30644E72E12EE90Cull},
    {0x5A373B5F7AF73DA2ull, 0x2D60710435287F2Cull, 0xBE41E7581B1666EDull, 0x2C256EDB7D33DB33ull},
    {0x196495F7B663FF01ull, 0xFDFC86092140EA1Eull, 0xC52305E8B541561Cull, 0x20240ECEDAF0603Aull},
    {0xCBEC8C22B4CCFD96ull, 0xB5A9E559281F8E55ull, 0x864244482D2FC0C9ull, 0x1FF9BF6F5E15CE2Eull},
};
static const uint64_t ZD[8][4] = {
    {0x20CFF123608FC9CCull, 0xCB49C3517C4604A5ull, 0xB3C4D79D41A91758ull, 0x0000000000000000ull},
    {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x20CFF123608FC9CAull, 0xCB49C3517C4604A5ull, 0xB3C4D79D41A91758ull, 0x0000000000000000ull},
    {0x419FE246C11F9396ull, 0x969386A2F88C094Aull, 0x6789AF3A83522EB1ull, 0x0000000000000001ull},
    {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
    {0x419FE246C11F9394ull, 0x969386A2F88C094Aull, 0x6789AF3A83522EB1ull, 0x0000000000000001ull},
    {0x419FE246C11F9398ull, 0x969386A2F88C094Aull, 0x6789AF3A83522EB1ull, 0x0000000000000001ull},
    {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
};
static const uint64_t ZC[8][4] = {
    {0x20CFF123608FCC3Cull, 0xCB49C3517C4604A5ull, 0xB3C4D79D41A91758ull, 0x0000000000000000ull},
    {0x49062F5891842131ull, 0xA467D1A98F0E1E11ull, 0x8882B66675586FEDull, 0x30644E72E1319E73ull},
    {0x20CFF123608FC75Aull, 0xCB49C3517C4604A5ull, 0xB3C4D79D41A91758ull, 0x0000000000000000ull},
    {0x3C7BA8821F9B7266ull, 0x1A5F9D41E3375BCAull, 0x97573E8A8F7B1721ull, 0x00000000000001B7ull},
    {0x49062F58918A14A1ull, 0xA467D1A98F0E1E11ull, 0x8882B66675586FEDull, 0x30644E72E1319E73ull},
    {0x3C7BA8821F957A14ull, 0x1A5F9D41E3375BCAull, 0x97573E8A8F7B1721ull, 0x00000000000001B7ull},
    {0x3C7BA8821FA16AB8ull, 0x1A5F9D41E3375BCAull, 0x97573E8A8F7B1721ull, 0x00000000000001B7ull},
    {0x49062F58917E2DC1ull, 0xA467D1A98F0E1E11ull, 0x8882B66675586FEDull, 0x30644E72E1319E73ull},
};
// the coefficients of step 5 for row 0 with Y[0][4] + 1: the upper half is not zero
static const uint64_t BAD[16][4] = {
    {0x78603A6A400645A8ull, 0xAC6BD4F8344F8610ull, 0x07F5DE183CD645C4ull, 0x1E3EB107CCBF041Aull},
    {0xA3057C7732185DD0ull, 0xD6C196473632BC6Eull, 0x79505EE7747AE78Cull, 0x0C19139CB84C680Aull},
    {0xCB81BB29B018BA9Dull, 0x7BC813504569EA80ull, 0xB05A679E44AB1298ull, 0x12259D6B14729C0Full},
    {0xA0DC791CBE075C0Full, 0x517252014386B422ull, 0x3EFFE6CF0D0670D0ull, 0x244B3AD628E5381Full},
    {0x1B65B6E172113135ull, 0x832D6B3F6A82427Full, 0x81463CFFB1512D51ull, 0x2A57C4A4850B6C24ull},
    {0x6E8737A0E22440D5ull, 0x5289A9977B9CA6EFull, 0x29AAC685B925FA25ull, 0x1E3EB107CCBF041Aull},
    {0x287C3EB27E139BE0ull, 0xA5067D090F372E12ull, 0x370A08B6D0302B0Bull, 0x060C89CE5C263405ull},
    {0xD55ABDF30E0334CAull, 0xD5AA3EB0FE1CC9A1ull, 0x8EA57F30C85B5E37ull, 0x12259D6B14729C0Full},
    {0xA3057C773208FC9Dull, 0xD6C196473632BC6Eull, 0x79505EE7747AE78Cull, 0x0C19139CB84C680Aull},
    {0xCB81BB29B008FC9Dull, 0x7BC813504569EA80ull, 0xB05A679E44AB1298ull, 0x12259D6B14729C0Full},
    {0xA0DC791CBDF70364ull, 0x517252014386B422ull, 0x3EFFE6CF0D0670D0ull, 0x244B3AD628E5381Full},
    {0x78603A6A3FF70364ull, 0xAC6BD4F8344F8610ull, 0x07F5DE183CD645C4ull, 0x1E3EB107CCBF041Aull},
    {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0},
};
// the polynomial of degree below 8 through the held values of row 1 with Y[1][5] + 1
static const uint64_t OTHER[16][4] = {
    {0x460AF8EE64307DC1ull, 0xAD832C8E6C6578DDull, 0xF2A0BDCEE8F5CF19ull, 0x183227397098D014ull},
    {0x8A99512A4DD7AC52ull, 0x3B384FB742ED3766ull, 0xF636DDA3EB382E43ull, 0x03A0B2AF37483C2Dull},
    {0xFAA4368B715F80C0ull, 0xF551A3B2647B878Cull, 0x634A348C9D477B4Bull, 0x152AAA451A9BBD28ull},
    {0xB7980D4EE642DC36ull, 0xCEF5D5C40131C890ull, 0x24EAAC7698B98245ull, 0x30333640EB7ABE21ull},
    {0x460AF8EE64326CB1ull, 0xAD832C8E6C6578DDull, 0xF2A0BDCEE8F5CF19ull, 0x183227397098D014ull},
    {0x8A99512A4DDA92BAull, 0x3B384FB742ED3766ull, 0xF636DDA3EB382E43ull, 0x03A0B2AF37483C2Dull},
    {0xFAA4368B71635EA0ull, 0xF551A3B2647B878Cull, 0x634A348C9D477B4Bull, 0x152AAA451A9BBD28ull},
    {0xB7980D4EE647B18Eull, 0xCEF5D5C40131C890ull, 0x24EAAC7698B98245ull, 0x30333640EB7ABE21ull},
    {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0},
};

int main() {
  try {
    check(sylow_hip_init(0), "sylow_hip_init");
    const int32_t log_c = 2, log_l = 2;
    const size_t c = 4, n = 16, m = 2;
    const uint8_t present[m][c] = {{1, 0, 1, 1}, {0, 1, 1, 0}};
    // y [m][4][n] as the C ABI lays it out: word w of element e of row j at (j 4 + w) n + e; missing cells hold all-ones words
    auto lay = [&](std::vector<uint64_t>* out, const uint8_t (*mask)[c]) {
      out->assign(4 * n * m, 0);
      for (size_t j = 0; j < m; ++j) for (size_t e = 0; e < n; ++e) for (size_t w = 0; w < 4; ++w)
        (*out)[(j * 4 + w) * n + e] = mask[j][e % c] ? Y[j * n + e][w] : ~(uint64_t)0;
    };
    std::vector<uint64_t> y, coeffs(4 * n * m), yo(4 * n * m), zd(4 * c * m), zc(4 * c * m);
    lay(&y, present);
    DeviceBuffer d_y(y.size() * 8), d_p(m * c), d_c(coeffs.size() * 8), d_yo(yo.size() * 8), d_s(m), d_zd(zd.size() * 8), d_zc(zc.size() * 8), d_vs(m);
    check(sylow_hip_memcpy_h2d(d_p.as<void>(), present, m * c, nullptr), "h2d");
    std::vector<uint8_t> st, vst;
    auto recover = [&](bool with_y) {
      check(sylow_hip_memcpy_h2d(d_y.as<void>(), y.data(), y.size() * 8, nullptr), "h2d");
      check(sylow_hip_kzg_recover_batch(d_y.as<uint64_t>(), d_p.as<uint8_t>(), log_c, log_l, m, d_c.as<uint64_t>(), with_y ? d_yo.as<uint64_t>() : nullptr,
                                        d_s.as<uint8_t>(), nullptr), "sylow_hip_kzg_recover_batch");
      check(sylow_hip_memcpy_d2h(coeffs.data(), d_c.as<void>(), coeffs.size() * 8, nullptr), "d2h");
      if (with_y) check(sylow_hip_memcpy_d2h(yo.data(), d_yo.as<void>(), yo.size() * 8, nullptr), "d2h");
      check(sylow_hip_stream_sync(nullptr), "sync");
      fetch_flags(&st, d_s, m);
    };
    auto row_is = [&](size_t j, const uint64_t (*want)[4]) {          // coefficients of row j against 16 baked values
      bool same = true;
      for (size_t e = 0; e < n; ++e) for (size_t w = 0; w < 4; ++w) same = same && coeffs[(j * 4 + w) * n + e] == want[e][w];
      return same;
    };
    auto row_is_blob = [&](size_t j) {
      bool same = true;
      for (size_t e = 0; e < n; ++e) for (size_t w = 0; w < 4; ++w)
        same = same && coeffs[(j * 4 + w) * n + e] == (w == 0 && e < n / 2 ? (j + 1) * 1000003ull + 7919ull * e * e + 1 : 0);
      return same;
    };

    check(sylow_hip_kzg_recover_vanish_batch(d_p.as<uint8_t>(), log_c, log_l, m, d_zd.as<uint64_t>(), d_zc.as<uint64_t>(), d_vs.as<uint8_t>(), nullptr),
          "sylow_hip_kzg_recover_vanish_batch");
    check(sylow_hip_memcpy_d2h(zd.data(), d_zd.as<void>(), zd.size() * 8, nullptr), "d2h");
    check(sylow_hip_memcpy_d2h(zc.data(), d_zc.as<void>(), zc.size() * 8, nullptr), "d2h");
    check(sylow_hip_stream_sync(nullptr), "sync");
    fetch_flags(&vst, d_vs, m);
    bool vanish = vst.size() == m && !vst[0] && !vst[1];
    for (size_t j = 0; j < m; ++j) for (size_t k = 0; k < c; ++k) for (size_t w = 0; w < 4; ++w)
      vanish = vanish && zd[(j * 4 + w) * c + k] == ZD[j * c + k][w] && zc[(j * 4 + w) * c + k] == ZC[j * c + k][w];

    recover(true);
    bool restored = true;
    for (size_t j = 0; j < m; ++j) for (size_t e = 0; e < n; ++e) for (size_t w = 0; w < 4; ++w) restored = restored && yo[(j * 4 + w) * n + e] == Y[j * n + e][w];
    const bool recovered = row_is_blob(0) && row_is_blob(1) && st[0] == 0 && st[1] == 0;

    y[(0 * 4 + 0) * n + 4] += 1;                                     // value 1 of cell 0 of row 0: detected, one cell short of half is missing
    y[(1 * 4 + 0) * n + 5] += 1;                                     // value 1 of cell 1 of row 1: exactly half is held, so it is another blob
    recover(false);
    const bool detected = st[0] == 2 && row_is(0, BAD), other = st[1] == 0 && row_is(1, OTHER) && !row_is_blob(1);

    const uint8_t few[m][c] = {{0, 0, 1, 0}, {1, 1, 1, 1}};           // row 0 holds one cell of four
    check(sylow_hip_memcpy_h2d(d_p.as<void>(), few, m * c, nullptr), "h2d");
    lay(&y, few);
    recover(true);
    bool refused = st[0] == 1 && st[1] == 0 && row_is_blob(1);
    for (size_t e = 0; e < n; ++e) for (size_t w = 0; w < 4; ++w) refused = refused && coeffs[w * n + e] == 0 && yo[w * n + e] == 0;

    const int32_t rc13 = sylow_hip_kzg_recover_batch(d_y.as<uint64_t>(), d_p.as<uint8_t>(), 13, 0, m, d_c.as<uint64_t>(), nullptr, d_s.as<uint8_t>(), nullptr);
    const int32_t rc00 = sylow_hip_kzg_recover_vanish_batch(d_p.as<uint8_t>(), 0, 0, m, d_zd.as<uint64_t>(), d_zc.as<uint64_t>(), d_vs.as<uint8_t>(), nullptr);
    std::printf("RECOVER %d %d%d %d%d %d %d%d\n", vanish ? 1 : 0, recovered ? 1 : 0, restored ? 1 : 0, detected ? 1 : 0, other ? 1 : 0, refused ? 1 : 0,
                rc13 == SYLOW_HIP_E_ARG ? 1 : 0, rc00 == SYLOW_HIP_E_ARG ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
