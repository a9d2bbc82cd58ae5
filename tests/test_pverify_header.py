"""CPU: include/sylow_pverify.h, the header of the batched PLONK verifier.  It compiles as plain C99, the library exports exactly the five
sylow_pverify_* names it declares, the ninth binding table of sylow_amd/_lib.py has exactly those keys and one ctypes argument per parameter,
the nine tables are disjoint, and every prototype carries a `@shape` line that sylow_amd/_shapes.py parses and the Engine's table holds.
Its entry points are sylow_pverify_*: the sets of sylow_hip_*, sylow_plonk_* and sylow_popen_* names are closed by the tests of the eight
other headers, and this header adds none."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_pverify.h")
NAMES = ["sylow_pverify_scalars_batch", "sylow_pverify_scalars_batch_tuned", "sylow_pverify_fold_batch", "sylow_pverify_verify_batch",
         "sylow_pverify_batch_verify_weighted"]
OTHER_HEADERS = ("sylow_hip.h", "sylow_hip_kzg_points.h", "sylow_hip_kzg_cosets.h", "sylow_hip_kzg_recover.h", "sylow_hip_kzg_cells.h", "sylow_hip_fr_scan.h",
                 "sylow_plonk.h", "sylow_popen.h")


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_pverify.h"\n'
                   "int main(void) { return SYLOW_HIP_PLONK_WIRES_MAX == 32 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_the_header_says_why_it_has_a_prefix_of_its_own_and_when_the_challenges_are_drawn():
    text = " ".join(re.sub(r"\n \*", " ", open(HEADER).read()).split())          # the comment's line breaks do not matter
    assert '#include "sylow_popen.h"' in open(HEADER).read()
    assert "NO sylow_hip_*, NO sylow_plonk_* AND NO sylow_popen_* symbol is added" in text and "sylow_pverify_" in text
    assert "SOUNDNESS: THE LIBRARY DRAWS NO CHALLENGE" in text and "ARE THOSE OF THE TRANSCRIPT" in text
    assert "u IS DRAWN AFTER W_zeta AND W_omega ARE FIXED" in text and "THE WEIGHTS ARE DRAWN AFTER ALL PROOFS ARE FIXED" in text
    assert "SLOT 2 W (p) IS NOT READ" in text and "FORCED TO 0" in text and "T = 3 W + E + 5" in text
    assert "BIT-IDENTICAL TO sylow_hip_g1_lincomb_batch" in text and "NO PAIRING, GROUP-LAW OR MSM KERNEL IS NEW" in text


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES) and all(n.startswith("sylow_pverify_") for n in protos)
    assert set(_lib.SIGNATURES_PVERIFY) == set(protos)
    tables = [_lib.SIGNATURES, _lib.SIGNATURES_KZG_POINTS, _lib.SIGNATURES_KZG_COSETS, _lib.SIGNATURES_KZG_RECOVER, _lib.SIGNATURES_KZG_CELLS, _lib.SIGNATURES_FR_SCAN,
              _lib.SIGNATURES_PLONK, _lib.SIGNATURES_POPEN, _lib.SIGNATURES_PVERIFY]
    assert sum(len(t) for t in tables) == len(set().union(*tables)), "the nine tables are disjoint"
    others = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in OTHER_HEADERS]
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert params[-1] == "stream" and len(params) == len(_lib.SIGNATURES_PVERIFY[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_PVERIFY[name]
        assert not any(name in text for text in others), "the other headers do not declare them"
    exported = subprocess.run(["nm", "-D", "--defined-only", sylow_amd._lib.LIB_PATH], capture_output=True, text=True, check=True, timeout=120).stdout
    assert set(re.findall(r"\b(sylow_pverify_\w+)\b", exported)) == set(NAMES), "the sylow_pverify_* exports are exactly the declared names"
    assert set(re.findall(r"\b(sylow_popen_\w+)\b", exported)) == set(_lib.SIGNATURES_POPEN), "and this header added no sylow_popen_* export"
    assert set(re.findall(r"\b(sylow_plonk_\w+)\b", exported)) == set(_lib.SIGNATURES_PLONK), "no sylow_plonk_* export"
    assert set(re.findall(r"\b(sylow_hip_\w+)\b", exported)) == set().union(*tables[:6]), "and no sylow_hip_* export"
    assert len(_lib.SIGNATURES_POPEN) == 6 and len(_lib.SIGNATURES_PLONK) == 5, "the two closed PLONK tables are as they were"


def test_every_prototype_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert HEADER == _shapes.HEADER_PVERIFY and set(shapes) == set(protos)
    for other in (_shapes.HEADER, _shapes.HEADER_KZG_POINTS, _shapes.HEADER_KZG_COSETS, _shapes.HEADER_KZG_RECOVER, _shapes.HEADER_KZG_CELLS, _shapes.HEADER_FR_SCAN,
                  _shapes.HEADER_PLONK, _shapes.HEADER_POPEN):
        assert not set(shapes) & set(_shapes.parse(other))
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, (names, sh) in shapes.items():
        assert names == protos[name]
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        pointers = {p.replace("*", " ").split()[-1] for p in proto.split(",") if "*" in p} - {"stream"}
        assert set(sh) == pointers, (name, set(sh) ^ pointers)           # every pointer has an extent
        assert _shapes.table()[name][1].keys() == sh.keys()              # and the Engine checks it on every call
        assert not any("-" in s.expr or "/" in s.expr for s in sh.values())
    optional = {n: sorted(p for p, s in sh.items() if s.optional) for n, (_, sh) in shapes.items()}
    pts = ["proof_inf", "pub", "vk_inf"]
    assert optional == {"sylow_pverify_scalars_batch": ["pub"], "sylow_pverify_scalars_batch_tuned": ["pub"], "sylow_pverify_fold_batch": pts,
                        "sylow_pverify_verify_batch": pts, "sylow_pverify_batch_verify_weighted": ["gt_out", "is_one"] + pts}
    v = {"log_n": 3, "log_e": 2, "W": 3, "m": 2, "n_pub": 3}
    T, P, K = 3 * 3 + 4 + 5, 3 + 4 + 3, 2 * 3 + 2
    for name in NAMES:
        sh = shapes[name][1]
        assert sh["evals"].nbytes(v) == 32 * 7 * 2 == 448 and sh["pub"].nbytes(v) == 32 * 3 * 2 and sh["shifts"].nbytes(v) == 96 and sh["status"].nbytes(v) == 2
        assert all(sh[k].nbytes(v) == 64 for k in ("beta", "gamma", "alpha", "zeta", "v", "u"))
        assert sh["pub"].nbytes(dict(v, n_pub=0)) == 0, "NULL pub is accepted with n_pub = 0"
    for name in NAMES[:2]:
        sh = shapes[name][1]
        assert sh["k_out"].nbytes(v) == 32 * T * 2 == 1152 and sh["y_out"].nbytes(v) == 64
        assert sh["k_out"].nbytes(dict(v, log_e=0, W=2)) == 32 * 12 * 2
    for name in NAMES[2:]:
        sh = shapes[name][1]
        assert sh["vk_xy"].nbytes(v) == 64 * K == 512 and sh["vk_inf"].nbytes(v) == K and sh["proof_xy"].nbytes(v) == 64 * P * 2 == 1280 and sh["proof_inf"].nbytes(v) == 20
    sh = shapes["sylow_pverify_fold_batch"][1]
    assert sh["c_xy"].nbytes(v) == 128 and sh["pi_xy"].nbytes(v) == 128 and sh["c_inf"].nbytes(v) == 2 and sh["pi_inf"].nbytes(v) == 2 and sh["y_out"].nbytes(v) == 64
    sh = shapes["sylow_pverify_verify_batch"][1]
    assert sh["tau_g2_xy"].nbytes(v) == 128 and sh["ok"].nbytes(v) == 2
    sh = shapes["sylow_pverify_batch_verify_weighted"][1]
    assert sh["tau_g2_xy"].nbytes(v) == 128 and sh["weights"].nbytes(v) == 64 and sh["gt_out"].nbytes(v) == 384 and sh["is_one"].nbytes(v) == 1


def test_the_bounds_and_the_helpers_are_the_shared_ones():
    plan = open(os.path.join(ROOT, "sylow_amd", "csrc", "plonk_verify_plan.hpp")).read()
    assert '#include "plonk_open_plan.hpp"' in plan and "using plonk_open_plan::dims_ok;" in plan and "using plonk_open_plan::STATUS_ZETA_IN_DOMAIN;" in plan
    unit = open(os.path.join(ROOT, "sylow_amd", "csrc", "plonk_verify.hip")).read()
    for shared in ("bn254_fr_block.hpp", "bn254_fr_roots.hpp", "plonk_verify_plan.hpp"):
        assert f'#include "{shared}"' in unit, "the shared helpers, no private copies"
    for private in ("BN_DEV Fp fr_pow", "BN_DEV Fp fr_one", "BN_DEV Fp lds_get", "BN_DEV Fp elem("):
        assert private not in unit, "no second copy of an Fr device helper"
    assert "sylow_hip_fr_batch_inv(" in unit and "fr_inv_lone" not in unit and "fr_inv(" not in unit, "the denominators share inversions; no power per term"
    for call in ("sylow_hip_g1_lincomb_batch(", "sylow_hip_kzg_verify_batch(", "sylow_hip_g1_msm(", "sylow_hip_g1_add_batch(", "sylow_hip_g1_generator_mul_batch(",
                 "sylow_hip_pairing_product_batch("):
        assert call in unit, call
