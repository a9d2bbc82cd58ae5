"""CPU: include/sylow_hip_kzg_recover.h, the extension header of the recovery of a KZG polynomial from any half of its cells.  It compiles as
plain C99, the library exports every symbol it declares, the fourth binding table of sylow_amd/_lib.py has exactly those keys and one ctypes
argument per parameter, and every prototype carries a `@shape` line that sylow_amd/_shapes.py parses and the Engine's table holds.  None
of the other three headers names them: their symbol sets are pinned by tests/test_capi.py, tests/test_kzg_points_header.py and
tests/test_kzg_cosets_header.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_hip_kzg_recover.h")
NAMES = ["sylow_hip_kzg_recover_vanish_batch", "sylow_hip_kzg_recover_batch"]
OTHER_HEADERS = ("sylow_hip.h", "sylow_hip_kzg_points.h", "sylow_hip_kzg_cosets.h")


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_hip_kzg_recover.h"\n'
                   "int main(void) { return SYLOW_HIP_KZG_RECOVER_LOG_C_MAX == 12 && SYLOW_HIP_KZG_RECOVER_LOG_N_MAX == 27 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES)
    assert set(_lib.SIGNATURES_KZG_RECOVER) == set(protos)
    tables = [_lib.SIGNATURES, _lib.SIGNATURES_KZG_POINTS, _lib.SIGNATURES_KZG_COSETS, _lib.SIGNATURES_KZG_RECOVER]
    assert sum(len(t) for t in tables) == len(set().union(*tables)), "the four tables are disjoint"
    others = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in OTHER_HEADERS]
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert params[-1] == "stream" and len(params) == len(_lib.SIGNATURES_KZG_RECOVER[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_KZG_RECOVER[name]
        assert not any(name in text for text in others), "the other headers' symbol sets are pinned"
        assert "coset" not in name and "points" not in name, "those names are counted by the other headers' tests"
    exported = subprocess.run(["nm", "-D", "--defined-only", sylow_amd._lib.LIB_PATH], capture_output=True, text=True, check=True, timeout=120).stdout
    recover = {s for s in re.findall(r"\b(sylow_hip_\w+)\b", exported) if "recover" in s}
    assert recover == set(NAMES), "the library exports exactly the declared names"


def test_every_prototype_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert HEADER == _shapes.HEADER_KZG_RECOVER and set(shapes) == set(protos)
    for other in (_shapes.HEADER, _shapes.HEADER_KZG_POINTS, _shapes.HEADER_KZG_COSETS):
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
    assert optional == {"sylow_hip_kzg_recover_vanish_batch": [], "sylow_hip_kzg_recover_batch": ["y_out"]}
    v = {"log_c": 3, "log_l": 2, "m": 5}
    sh = shapes["sylow_hip_kzg_recover_vanish_batch"][1]
    assert sh["present"].nbytes(v) == 5 * 8 and sh["zd_out"].nbytes(v) == 5 * 4 * 8 * 8 and sh["zc_out"].nbytes(v) == 5 * 4 * 8 * 8 and sh["status_out"].nbytes(v) == 5
    sh = shapes["sylow_hip_kzg_recover_batch"][1]
    assert sh["y"].nbytes(v) == 5 * 4 * 32 * 8 and sh["coeffs_out"].nbytes(v) == sh["y"].nbytes(v) == sh["y_out"].nbytes(v)
    assert sh["present"].nbytes(v) == 5 * 8 and sh["status_out"].nbytes(v) == 5


def test_the_bounds_are_the_plan_s():
    plan = open(os.path.join(ROOT, "sylow_amd", "csrc", "kzg_recover_plan.hpp")).read()
    head = open(HEADER).read()
    for macro, const in (("SYLOW_HIP_KZG_RECOVER_LOG_C_MAX", "RECOVER_LOG_C_MAX"), ("SYLOW_HIP_KZG_RECOVER_LOG_N_MAX", "RECOVER_LOG_N_MAX")):
        a = int(re.search(r"#define\s+" + macro + r"\s+(\d+)", head).group(1))
        b = int(re.search(r"constexpr int " + const + r" = (\d+);", plan).group(1))
        assert a == b, (macro, a, b)
