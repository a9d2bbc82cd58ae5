"""CPU: include/sylow_popen.h, the header of PLONK's closing rounds.  It compiles as plain C99, the library exports exactly the six
sylow_popen_* names it declares, the eighth binding table of sylow_amd/_lib.py has exactly those keys and one ctypes argument per parameter,
the eight tables are disjoint, and every prototype carries a `@shape` line that sylow_amd/_shapes.py parses and the Engine's table holds.
Its entry points are sylow_popen_*: the sets of sylow_hip_* and of sylow_plonk_* names are closed by the tests of the seven other headers,
and this header adds none."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_popen.h")
NAMES = ["sylow_popen_prepare", "sylow_popen_evaluate_batch", "sylow_popen_evaluate_batch_tuned", "sylow_popen_linearise_batch",
         "sylow_popen_linearise_batch_tuned", "sylow_popen_open_batch"]
OTHER_HEADERS = ("sylow_hip.h", "sylow_hip_kzg_points.h", "sylow_hip_kzg_cosets.h", "sylow_hip_kzg_recover.h", "sylow_hip_kzg_cells.h", "sylow_hip_fr_scan.h",
                 "sylow_plonk.h")


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_popen.h"\n'
                   "int main(void) { return SYLOW_HIP_PLONK_WIRES_MAX == 32 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_the_header_says_why_it_has_a_prefix_of_its_own_and_when_the_challenges_are_drawn():
    text = " ".join(re.sub(r"\n \*", " ", open(HEADER).read()).split())          # the comment's line breaks do not matter
    assert '#include "sylow_plonk.h"' in open(HEADER).read()
    assert "NO sylow_hip_* AND NO sylow_plonk_* symbol is added" in text and "sylow_popen_" in text and "THE LIBRARY DRAWS NO CHALLENGE" in text
    assert "zeta MUST BE DRAWN AFTER THE COMMITMENTS TO THE CHUNKS OF t ARE FIXED" in text and "v AFTER THE EVALUATIONS ARE FIXED" in text
    assert "TAKES v BESIDE zeta" in text, "the full route's ordering caveat"
    assert "sylow_popen.h" in open(os.path.join(ROOT, "include", "sylow_plonk.h")).read(), "the prover surface's header points here"


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES) and all(n.startswith("sylow_popen_") for n in protos)
    assert set(_lib.SIGNATURES_POPEN) == set(protos)
    tables = [_lib.SIGNATURES, _lib.SIGNATURES_KZG_POINTS, _lib.SIGNATURES_KZG_COSETS, _lib.SIGNATURES_KZG_RECOVER, _lib.SIGNATURES_KZG_CELLS, _lib.SIGNATURES_FR_SCAN,
              _lib.SIGNATURES_PLONK, _lib.SIGNATURES_POPEN]
    assert sum(len(t) for t in tables) == len(set().union(*tables)), "the eight tables are disjoint"
    others = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in OTHER_HEADERS]
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert params[-1] == "stream" and len(params) == len(_lib.SIGNATURES_POPEN[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_POPEN[name]
        assert not any(name in text for text in others), "the other headers do not declare them"
    exported = subprocess.run(["nm", "-D", "--defined-only", sylow_amd._lib.LIB_PATH], capture_output=True, text=True, check=True, timeout=120).stdout
    assert set(re.findall(r"\b(sylow_popen_\w+)\b", exported)) == set(NAMES), "the sylow_popen_* exports are exactly the declared names"
    assert set(re.findall(r"\b(sylow_plonk_\w+)\b", exported)) == set(_lib.SIGNATURES_PLONK), "and this header added no sylow_plonk_* export"
    assert set(re.findall(r"\b(sylow_hip_\w+)\b", exported)) == set().union(*tables[:6]), "and no sylow_hip_* export"


def test_every_prototype_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert HEADER == _shapes.HEADER_POPEN and set(shapes) == set(protos)
    for other in (_shapes.HEADER, _shapes.HEADER_KZG_POINTS, _shapes.HEADER_KZG_COSETS, _shapes.HEADER_KZG_RECOVER, _shapes.HEADER_KZG_CELLS, _shapes.HEADER_FR_SCAN,
                  _shapes.HEADER_PLONK):
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
    assert optional == {"sylow_popen_prepare": [], "sylow_popen_evaluate_batch": ["pi"], "sylow_popen_evaluate_batch_tuned": ["pi"],
                        "sylow_popen_linearise_batch": ["f_out", "r_out", "v", "wires"], "sylow_popen_linearise_batch_tuned": ["f_out", "r_out", "v", "wires"],
                        "sylow_popen_open_batch": ["pi"]}
    v = {"log_n": 3, "log_e": 2, "W": 3, "m": 2, "len_w": 10, "len_z": 11, "len_out": 12, "len_f": 16}
    ctable, evals = 8 * 8 * 32, 32 * (2 * 3 + 1) * 2
    sh = shapes["sylow_popen_prepare"][1]
    assert sh["selectors"].nbytes(v) == 5 * 8 * 32 and sh["sigma"].nbytes(v) == 3 * 8 * 32 and sh["ctable"].nbytes(v) == ctable
    for name in ("sylow_popen_evaluate_batch", "sylow_popen_evaluate_batch_tuned"):
        sh = shapes[name][1]
        assert sh["ctable"].nbytes(v) == ctable and sh["wires"].nbytes(v) == 2 * 3 * 10 * 32 and sh["z"].nbytes(v) == 2 * 11 * 32 and sh["pi"].nbytes(v) == 2 * 8 * 32
        assert sh["zeta"].nbytes(v) == 64 and sh["evals_out"].nbytes(v) == evals == 448
    for name in ("sylow_popen_linearise_batch", "sylow_popen_linearise_batch_tuned"):
        sh = shapes[name][1]
        assert sh["ctable"].nbytes(v) == ctable and sh["wires"].nbytes(v) == 2 * 3 * 10 * 32 and sh["z"].nbytes(v) == 2 * 11 * 32 and sh["t"].nbytes(v) == 2 * 32 * 32
        assert sh["evals"].nbytes(v) == evals and sh["shifts"].nbytes(v) == 96 and all(sh[k].nbytes(v) == 64 for k in ("beta", "gamma", "alpha", "zeta", "v"))
        assert sh["r_out"].nbytes(v) == 2 * 12 * 32 and sh["f_out"].nbytes(v) == 2 * 12 * 32 and sh["status"].nbytes(v) == 2
    sh = shapes["sylow_popen_open_batch"][1]
    assert sh["srs_g1_xy"].nbytes(v) == 16 * 64 and sh["ctable"].nbytes(v) == ctable and sh["t"].nbytes(v) == 2 * 32 * 32 and sh["evals_out"].nbytes(v) == evals
    assert sh["w_zeta_xy"].nbytes(v) == 128 and sh["w_omega_xy"].nbytes(v) == 128 and sh["w_zeta_inf"].nbytes(v) == 2 and sh["w_omega_inf"].nbytes(v) == 2
    assert sh["status"].nbytes(v) == 2 and sh["pi"].nbytes(v) == 2 * 8 * 32 and sh["v"].nbytes(v) == 64


def test_the_bounds_are_the_plan_s():
    plan = open(os.path.join(ROOT, "sylow_amd", "csrc", "plonk_open_plan.hpp")).read()
    assert "constexpr int PO_WIRES_MAX = fr_scan_plan::PLONK_WIRES_MAX;" in plan and "constexpr int PO_WIRES_MIN = 2;" in plan
    assert "constexpr size_t PO_EVAL_CHUNK = kzg_plan::KZG_POLY_CHUNK;" in plan and "constexpr int PO_FLUSH = 16;" in plan
    unit = open(os.path.join(ROOT, "sylow_amd", "csrc", "plonk_open.hip")).read()
    for shared in ("bn254_fr_block.hpp", "bn254_fr_acc.hpp", "kzg_scan_dev.hpp", "plonk_open_plan.hpp"):
        assert f'#include "{shared}"' in unit, "the shared helpers, no private copies"
