"""CPU: include/sylow_plonk.h, the header of the PLONK prover surface (for now the quotient polynomial).  It compiles as plain C99, the library
exports every symbol it declares, the seventh binding table of sylow_amd/_lib.py has exactly those keys and one ctypes argument per
parameter, and every prototype carries a `@shape` line that sylow_amd/_shapes.py parses and the Engine's table holds.  Its entry points are
sylow_plonk_*: the set of sylow_hip_* names is closed by the tests of the six other headers, and this header adds none."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_plonk.h")
NAMES = ["sylow_plonk_quotient_prepare", "sylow_plonk_quotient_evals_batch", "sylow_plonk_quotient_evals_batch_tuned", "sylow_plonk_quotient_batch",
         "sylow_plonk_quotient_batch_tuned"]
OTHER_HEADERS = ("sylow_hip.h", "sylow_hip_kzg_points.h", "sylow_hip_kzg_cosets.h", "sylow_hip_kzg_recover.h", "sylow_hip_kzg_cells.h", "sylow_hip_fr_scan.h")


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_plonk.h"\n'
                   "int main(void) { return SYLOW_HIP_PLONK_WIRES_MAX == 32 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_the_header_says_why_it_has_a_prefix_of_its_own():
    text = " ".join(re.sub(r"\n \*", " ", open(HEADER).read()).split())          # the comment's line breaks do not matter
    assert '#include "sylow_hip_fr_scan.h"' in open(HEADER).read()
    assert "NO sylow_hip_* symbol is added" in text and "sylow_plonk_" in text and "THE LIBRARY DRAWS NO CHALLENGE" in text
    assert "alpha AFTER THE COMMITMENT TO z IS FIXED" in text and "STATUS 0 DOES NOT PROVE DIVISIBILITY" in text


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES) and not any(n.startswith("sylow_hip_") for n in protos)
    assert set(_lib.SIGNATURES_PLONK) == set(protos)
    tables = [_lib.SIGNATURES, _lib.SIGNATURES_KZG_POINTS, _lib.SIGNATURES_KZG_COSETS, _lib.SIGNATURES_KZG_RECOVER, _lib.SIGNATURES_KZG_CELLS, _lib.SIGNATURES_FR_SCAN,
              _lib.SIGNATURES_PLONK]
    assert sum(len(t) for t in tables) == len(set().union(*tables)), "the seven tables are disjoint"
    others = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in OTHER_HEADERS]
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert params[-1] == "stream" and len(params) == len(_lib.SIGNATURES_PLONK[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_PLONK[name]
        assert not any(name in text for text in others), "the other headers do not name them"
    exported = subprocess.run(["nm", "-D", "--defined-only", sylow_amd._lib.LIB_PATH], capture_output=True, text=True, check=True, timeout=120).stdout
    assert set(re.findall(r"\b(sylow_plonk_\w+)\b", exported)) == set(NAMES), "the sylow_plonk_* exports are exactly the declared names"
    assert set(re.findall(r"\b(sylow_hip_\w+)\b", exported)) == set().union(*tables[:6]), "and this header added no sylow_hip_* export"


def test_every_prototype_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert HEADER == _shapes.HEADER_PLONK and set(shapes) == set(protos)
    for other in (_shapes.HEADER, _shapes.HEADER_KZG_POINTS, _shapes.HEADER_KZG_COSETS, _shapes.HEADER_KZG_RECOVER, _shapes.HEADER_KZG_CELLS, _shapes.HEADER_FR_SCAN):
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
    assert optional == {"sylow_plonk_quotient_prepare": [], "sylow_plonk_quotient_evals_batch": ["pi_ext"], "sylow_plonk_quotient_evals_batch_tuned": ["pi_ext"],
                        "sylow_plonk_quotient_batch": ["pi"], "sylow_plonk_quotient_batch_tuned": ["pi"]}
    v = {"log_n": 3, "log_e": 2, "W": 3, "m": 2, "len_w": 10, "len_z": 11}
    table = (4 * 32 * 9 + 4 * 4) * 8
    sh = shapes["sylow_plonk_quotient_prepare"][1]
    assert sh["selectors"].nbytes(v) == 5 * 8 * 32 and sh["sigma"].nbytes(v) == 3 * 8 * 32 and sh["table"].nbytes(v) == table
    for name in ("sylow_plonk_quotient_evals_batch", "sylow_plonk_quotient_evals_batch_tuned"):
        sh = shapes[name][1]
        assert sh["table"].nbytes(v) == table and sh["wires_ext"].nbytes(v) == 2 * 3 * 32 * 32 and sh["z_ext"].nbytes(v) == 2 * 32 * 32
        assert sh["pi_ext"].nbytes(v) == 2 * 32 * 32 and sh["t_ext_out"].nbytes(v) == 2 * 32 * 32 and sh["shifts"].nbytes(v) == 96
        assert sh["beta"].nbytes(v) == 64 and sh["gamma"].nbytes(v) == 64 and sh["alpha"].nbytes(v) == 64
    for name in ("sylow_plonk_quotient_batch", "sylow_plonk_quotient_batch_tuned"):
        sh = shapes[name][1]
        assert sh["table"].nbytes(v) == table and sh["wires"].nbytes(v) == 2 * 3 * 10 * 32 and sh["z"].nbytes(v) == 2 * 11 * 32 and sh["pi"].nbytes(v) == 2 * 8 * 32
        assert sh["t_out"].nbytes(v) == 2 * 32 * 32 and sh["status"].nbytes(v) == 2 and sh["shifts"].nbytes(v) == 96 and sh["alpha"].nbytes(v) == 64


def test_the_bounds_are_the_plan_s():
    plan = open(os.path.join(ROOT, "sylow_amd", "csrc", "plonk_quotient_plan.hpp")).read()
    assert "constexpr int PQ_WIRES_MAX = fr_scan_plan::PLONK_WIRES_MAX;" in plan and "constexpr int PQ_WIRES_MIN = 2;" in plan
    assert "constexpr uint64_t PQ_COSET_SHIFT = 5;" in plan and "constexpr uint64_t G16_COSET_SHIFT = 5;" in open(
        os.path.join(ROOT, "sylow_amd", "csrc", "groth16_prove_plan.hpp")).read(), "the shift of the Groth16 quotient"
