"""CPU: include/sylow_hip_fr_scan.h, the extension header of the scans over Fr and of PLONK's permutation grand product.  It compiles as plain
C99, the library exports every symbol it declares, the sixth binding table of sylow_amd/_lib.py has exactly those keys and one ctypes argument
per parameter, and every prototype carries a `@shape` line that sylow_amd/_shapes.py parses and the Engine's table holds.  None of the other
five headers names them: their symbol sets are pinned by tests/test_capi.py and the four other header tests, which also count the exported
names that hold `points`, `coset`, `recover` or `kzg_cells`."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_hip_fr_scan.h")
NAMES = ["sylow_hip_fr_scan_batch", "sylow_hip_fr_scan_batch_tuned", "sylow_hip_fr_ratio_scan_batch", "sylow_hip_fr_ratio_scan_batch_tuned",
         "sylow_hip_plonk_identity_batch", "sylow_hip_plonk_permutation_batch", "sylow_hip_plonk_permutation_batch_tuned"]
OTHER_HEADERS = ("sylow_hip.h", "sylow_hip_kzg_points.h", "sylow_hip_kzg_cosets.h", "sylow_hip_kzg_recover.h", "sylow_hip_kzg_cells.h")


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_hip_fr_scan.h"\n'
                   "int main(void) { return SYLOW_HIP_PLONK_WIRES_MAX == 32 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES)
    assert set(_lib.SIGNATURES_FR_SCAN) == set(protos)
    tables = [_lib.SIGNATURES, _lib.SIGNATURES_KZG_POINTS, _lib.SIGNATURES_KZG_COSETS, _lib.SIGNATURES_KZG_RECOVER, _lib.SIGNATURES_KZG_CELLS, _lib.SIGNATURES_FR_SCAN]
    assert sum(len(t) for t in tables) == len(set().union(*tables)), "the six tables are disjoint"
    others = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in OTHER_HEADERS]
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert params[-1] == "stream" and len(params) == len(_lib.SIGNATURES_FR_SCAN[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_FR_SCAN[name]
        assert not any(name in text for text in others), "the other headers' symbol sets are pinned"
        assert not any(s in name for s in ("points", "coset", "recover", "kzg_cells")), "those names are counted by the other headers' tests"
    exported = subprocess.run(["nm", "-D", "--defined-only", sylow_amd._lib.LIB_PATH], capture_output=True, text=True, check=True, timeout=120).stdout
    bound = set().union(*tables)
    mine = {s for s in re.findall(r"\b(sylow_hip_\w+)\b", exported) if s not in bound - set(NAMES)}
    assert mine == set(NAMES), "every exported name is declared in one of the six headers, and this one's are exactly these"


def test_every_prototype_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert HEADER == _shapes.HEADER_FR_SCAN and set(shapes) == set(protos)
    for other in (_shapes.HEADER, _shapes.HEADER_KZG_POINTS, _shapes.HEADER_KZG_COSETS, _shapes.HEADER_KZG_RECOVER, _shapes.HEADER_KZG_CELLS):
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
    assert optional == {"sylow_hip_fr_scan_batch": ["total_out"], "sylow_hip_fr_scan_batch_tuned": ["total_out"],
                        "sylow_hip_fr_ratio_scan_batch": ["num", "total_out"], "sylow_hip_fr_ratio_scan_batch_tuned": ["num", "total_out"],
                        "sylow_hip_plonk_identity_batch": [],
                        "sylow_hip_plonk_permutation_batch": ["total_out"], "sylow_hip_plonk_permutation_batch_tuned": ["total_out"]}
    assert {p for o in optional.values() for p in o} == {"total_out", "num"}
    v = {"len": 5, "m": 3, "log_n": 3, "W": 2}
    for name in ("sylow_hip_fr_scan_batch", "sylow_hip_fr_scan_batch_tuned"):
        sh = shapes[name][1]
        assert sh["a"].nbytes(v) == 480 and sh["out"].nbytes(v) == 480 and sh["total_out"].nbytes(v) == 96
    for name in ("sylow_hip_fr_ratio_scan_batch", "sylow_hip_fr_ratio_scan_batch_tuned"):
        sh = shapes[name][1]
        assert sh["num"].nbytes(v) == 480 and sh["den"].nbytes(v) == 480 and sh["out"].nbytes(v) == 480 and sh["total_out"].nbytes(v) == 96 and sh["status"].nbytes(v) == 3
    sh = shapes["sylow_hip_plonk_identity_batch"][1]
    assert sh["shifts"].nbytes(v) == 64 and sh["out"].nbytes(v) == 2 * 8 * 32
    for name in ("sylow_hip_plonk_permutation_batch", "sylow_hip_plonk_permutation_batch_tuned"):
        sh = shapes[name][1]
        assert sh["wires"].nbytes(v) == 3 * 2 * 8 * 32 and sh["sigma"].nbytes(v) == 2 * 8 * 32 and sh["shifts"].nbytes(v) == 64
        assert sh["beta"].nbytes(v) == 96 and sh["gamma"].nbytes(v) == 96 and sh["z_out"].nbytes(v) == 3 * 8 * 32 and sh["status"].nbytes(v) == 3


def test_the_bound_is_the_plan_s():
    plan = open(os.path.join(ROOT, "sylow_amd", "csrc", "fr_scan_plan.hpp")).read()
    a = int(re.search(r"#define\s+SYLOW_HIP_PLONK_WIRES_MAX\s+(\d+)", open(HEADER).read()).group(1))
    b = int(re.search(r"constexpr int PLONK_WIRES_MAX = (\d+);", plan).group(1))
    assert a == b == 32, (a, b)
