"""CPU: include/sylow_hip_kzg_cells.h, the extension header of the check of many cells of many KZG blobs as one boolean.  It compiles as plain
C99, the library exports every symbol it declares and no other with `kzg_cells` in its name, the fifth binding table of sylow_amd/_lib.py has
exactly those keys and one ctypes argument per parameter, and every prototype carries a `@shape` line that sylow_amd/_shapes.py parses and
the Engine's table holds.  None of the other four headers names them: their symbol sets are pinned by tests/test_capi.py,
tests/test_kzg_points_header.py, tests/test_kzg_cosets_header.py and tests/test_kzg_recover_header.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_hip_kzg_cells.h")
NAMES = ["sylow_hip_kzg_cells_fold_batch", "sylow_hip_kzg_cells_fold_batch_tuned", "sylow_hip_kzg_cells_reduce_batch", "sylow_hip_kzg_cells_verify_weighted"]
OTHER_HEADERS = ("sylow_hip.h", "sylow_hip_kzg_points.h", "sylow_hip_kzg_cosets.h", "sylow_hip_kzg_recover.h")


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_hip_kzg_cells.h"\n'
                   "int main(void) { return SYLOW_HIP_KZG_CELLS_LOG_N_MAX == 27 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES)
    assert set(_lib.SIGNATURES_KZG_CELLS) == set(protos)
    tables = [_lib.SIGNATURES, _lib.SIGNATURES_KZG_POINTS, _lib.SIGNATURES_KZG_COSETS, _lib.SIGNATURES_KZG_RECOVER, _lib.SIGNATURES_KZG_CELLS]
    assert sum(len(t) for t in tables) == len(set().union(*tables)), "the five tables are disjoint"
    others = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in OTHER_HEADERS]
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert params[-1] == "stream" and len(params) == len(_lib.SIGNATURES_KZG_CELLS[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_KZG_CELLS[name]
        assert not any(name in text for text in others), "the other headers' symbol sets are pinned"
        assert "kzg_cells" in name and "coset" not in name and "points" not in name and "recover" not in name, "those names are counted by the other headers' tests"
    exported = subprocess.run(["nm", "-D", "--defined-only", sylow_amd._lib.LIB_PATH], capture_output=True, text=True, check=True, timeout=120).stdout
    cells = {s for s in re.findall(r"\b(sylow_hip_\w+)\b", exported) if "kzg_cells" in s}
    assert cells == set(NAMES), "the library exports exactly the declared names"


def test_every_prototype_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert HEADER == _shapes.HEADER_KZG_CELLS and set(shapes) == set(protos)
    for other in (_shapes.HEADER, _shapes.HEADER_KZG_POINTS, _shapes.HEADER_KZG_COSETS, _shapes.HEADER_KZG_RECOVER):
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
    assert optional == {"sylow_hip_kzg_cells_fold_batch": [], "sylow_hip_kzg_cells_fold_batch_tuned": [],
                        "sylow_hip_kzg_cells_reduce_batch": ["c_inf", "pi_inf"],
                        "sylow_hip_kzg_cells_verify_weighted": ["c_inf", "gt_out", "in_range_out", "is_one", "pi_inf"]}
    v = {"log_c": 3, "log_l": 2, "rows": 5, "n_com": 3}
    for name in ("sylow_hip_kzg_cells_fold_batch", "sylow_hip_kzg_cells_fold_batch_tuned"):
        sh = shapes[name][1]
        assert sh["idx"].nbytes(v) == 40 and sh["com_idx"].nbytes(v) == 40 and sh["vals"].nbytes(v) == 5 * 4 * 4 * 8 and sh["weights"].nbytes(v) == 160
        assert sh["w_out"].nbytes(v) == 96 and sh["a_out"].nbytes(v) == 128 and sh["r_out"].nbytes(v) == 160 and sh["rz_out"].nbytes(v) == 160
        assert sh["in_range_out"].nbytes(v) == 1
    sh = shapes["sylow_hip_kzg_cells_reduce_batch"][1]
    assert sh["srs_g1_xy"].nbytes(v) == 256 and sh["c_xy"].nbytes(v) == 192 and sh["c_inf"].nbytes(v) == 3 and sh["pi_xy"].nbytes(v) == 320 and sh["pi_inf"].nbytes(v) == 5
    assert sh["f_xy"].nbytes(v) == 64 and sh["p_xy"].nbytes(v) == 64 and sh["f_inf"].nbytes(v) == 1 and sh["p_inf"].nbytes(v) == 1
    sh = shapes["sylow_hip_kzg_cells_verify_weighted"][1]
    assert sh["tau_l_g2_xy"].nbytes(v) == 128 and sh["gt_out"].nbytes(v) == 384 and sh["is_one"].nbytes(v) == 1 and sh["vals"].nbytes(v) == 640


def test_the_bound_is_the_plan_s():
    plan = open(os.path.join(ROOT, "sylow_amd", "csrc", "kzg_cells_plan.hpp")).read()
    a = int(re.search(r"#define\s+SYLOW_HIP_KZG_CELLS_LOG_N_MAX\s+(\d+)", open(HEADER).read()).group(1))
    b = int(re.search(r"constexpr int CELLS_LOG_N_MAX = (\d+);", plan).group(1))
    assert a == b, (a, b)
