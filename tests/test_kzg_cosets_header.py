"""CPU: include/sylow_hip_kzg_cosets.h, the extension header of the KZG proofs on every coset of the domain.  It compiles as plain C99, the
library exports every symbol it declares, the third binding table of sylow_amd/_lib.py has exactly those keys and one ctypes argument per
parameter, and every prototype carries a `@shape` line that sylow_amd/_shapes.py parses and the Engine's table holds.  Neither
include/sylow_hip.h nor include/sylow_hip_kzg_points.h names them: their symbol sets are pinned by tests/test_capi.py and
tests/test_kzg_points_header.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_hip_kzg_cosets.h")
NAMES = ["sylow_hip_kzg_open_cosets_prepare", "sylow_hip_kzg_open_cosets_batch", "sylow_hip_kzg_open_cosets_batch_tuned", "sylow_hip_kzg_coset_interp_batch",
         "sylow_hip_kzg_cosets_reduce_batch", "sylow_hip_kzg_verify_cosets_batch"]


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_hip_kzg_cosets.h"\nint main(void) { return SYLOW_HIP_KZG_COSETS_LOG_N_MAX == 27 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES)
    assert set(_lib.SIGNATURES_KZG_COSETS) == set(protos)
    assert not set(_lib.SIGNATURES_KZG_COSETS) & set(_lib.SIGNATURES) and not set(_lib.SIGNATURES_KZG_COSETS) & set(_lib.SIGNATURES_KZG_POINTS)
    others = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in ("sylow_hip.h", "sylow_hip_kzg_points.h")]
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert params[-1] == "stream" and len(params) == len(_lib.SIGNATURES_KZG_COSETS[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_KZG_COSETS[name]
        assert not any(name in text for text in others), "the other headers' symbol sets are pinned"
    exported = subprocess.run(["nm", "-D", "--defined-only", sylow_amd._lib.LIB_PATH], capture_output=True, text=True, check=True, timeout=120).stdout
    cosets = {s for s in re.findall(r"\b(sylow_hip_\w+)\b", exported) if "coset" in s}
    assert cosets == set(NAMES), "the library exports exactly the declared names"


def test_every_prototype_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert HEADER == _shapes.HEADER_KZG_COSETS and set(shapes) == set(protos)
    assert not set(shapes) & set(_shapes.parse()) and not set(shapes) & set(_shapes.parse(_shapes.HEADER_KZG_POINTS))
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, (names, sh) in shapes.items():
        assert names == protos[name]
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        pointers = {p.replace("*", " ").split()[-1] for p in proto.split(",") if "*" in p} - {"stream"}
        assert set(sh) == pointers, (name, set(sh) ^ pointers)           # every pointer has an extent
        assert _shapes.table()[name][1].keys() == sh.keys()              # and the Engine checks it on every call
        assert not any("-" in s.expr or "/" in s.expr for s in sh.values())
    optional = {n: sorted(p for p, s in sh.items() if s.optional) for n, (_, sh) in shapes.items()}
    assert optional == {"sylow_hip_kzg_open_cosets_prepare": [], "sylow_hip_kzg_open_cosets_batch": ["table_inf", "y_out"],
                        "sylow_hip_kzg_open_cosets_batch_tuned": ["table_inf", "y_out"], "sylow_hip_kzg_coset_interp_batch": ["in_range_out"],
                        "sylow_hip_kzg_cosets_reduce_batch": ["c_inf", "in_range_out"], "sylow_hip_kzg_verify_cosets_batch": ["c_inf", "pi_inf"]}
    v = {"log_c": 3, "log_l": 2, "m": 5, "rows": 7}
    sh = shapes["sylow_hip_kzg_open_cosets_batch_tuned"][1]
    assert sh["table_xy"].nbytes(v) == 4 * 8 * 16 * 8 and sh["table_inf"].nbytes(v) == 4 * 16 and sh["coeffs"].nbytes(v) == 5 * 4 * 32 * 8
    assert sh["pi_xy"].nbytes(v) == 5 * 8 * 8 * 8 and sh["pi_inf"].nbytes(v) == 5 * 8 and sh["y_out"].nbytes(v) == sh["coeffs"].nbytes(v)
    sh = shapes["sylow_hip_kzg_verify_cosets_batch"][1]
    assert sh["srs_g1_xy"].nbytes(v) == 8 * 4 * 8 and sh["vals"].nbytes(v) == 7 * 4 * 4 * 8 and sh["idx"].nbytes(v) == 7 * 8 and sh["tau_l_g2_xy"].nbytes(v) == 128
    assert shapes["sylow_hip_kzg_cosets_reduce_batch"][1]["z_out"].nbytes(v) == 4 * 7 * 8
