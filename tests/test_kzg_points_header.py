"""CPU: include/sylow_hip_kzg_points.h, the extension header of the several-point KZG opening.  It compiles as plain C99, the library exports
every symbol it declares, the second binding table of sylow_amd/_lib.py has exactly those keys and one ctypes argument per parameter, and
every prototype carries a `@shape` line that sylow_amd/_shapes.py parses and the Engine's table holds.  include/sylow_hip.h declares none of
them: its symbol set is pinned by tests/test_capi.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_hip_kzg_points.h")
NAMES = ["sylow_hip_kzg_points_weights_batch", "sylow_hip_kzg_quotient_points_batch", "sylow_hip_kzg_open_points_batch", "sylow_hip_kzg_points_polys_batch",
         "sylow_hip_kzg_verify_points_batch"]


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_hip_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_hip_kzg_points.h"\nint main(void) { return SYLOW_HIP_KZG_POINTS_MAX == 64 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES)
    assert set(_lib.SIGNATURES_KZG_POINTS) == set(protos)
    assert not set(_lib.SIGNATURES_KZG_POINTS) & set(_lib.SIGNATURES)
    main = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sylow_hip.h")).read(), flags=re.S)
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert params[-1] == "stream" and len(params) == len(_lib.SIGNATURES_KZG_POINTS[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_KZG_POINTS[name]
        assert name not in main, "the main header's symbol set is pinned"


def test_every_prototype_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert set(shapes) == set(protos)
    assert not set(shapes) & set(_shapes.parse()), "the default of parse() is the main header"
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, (names, sh) in shapes.items():
        assert names == protos[name]
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        pointers = {p.replace("*", " ").split()[-1] for p in proto.split(",") if "*" in p} - {"stream"}
        assert set(sh) == pointers, (name, set(sh) ^ pointers)           # every pointer has an extent
        assert _shapes.table()[name][1].keys() == sh.keys()              # and the Engine checks it on every call
    optional = {n: sorted(p for p, s in sh.items() if s.optional) for n, (_, sh) in shapes.items()}
    assert optional == {"sylow_hip_kzg_points_weights_batch": ["distinct_out"], "sylow_hip_kzg_quotient_points_batch": ["q_out", "y_out"],
                        "sylow_hip_kzg_open_points_batch": [], "sylow_hip_kzg_points_polys_batch": [],
                        "sylow_hip_kzg_verify_points_batch": ["c_inf", "pi_inf"]}
    sh = shapes["sylow_hip_kzg_verify_points_batch"][1]
    assert sh["srs_g2_xy"].nbytes({"k": 3, "n": 5}) == 16 * 4 * 8 and sh["z"].nbytes({"k": 3, "n": 5}) == 4 * 15 * 8
    assert shapes["sylow_hip_kzg_points_polys_batch"][1]["zpoly_out"].nbytes({"k": 3, "n": 5}) == 4 * 5 * 4 * 8
