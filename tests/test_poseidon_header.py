"""CPU: include/sylow_poseidon.h, the header of batched Poseidon and its Merkle trees.  It compiles as plain C99, the library exports exactly
the twelve sylow_poseidon_* names it declares, the tenth binding table of sylow_amd/_lib.py has exactly those keys and one ctypes argument
per parameter, the ten tables are disjoint, and every prototype that takes an array carries a `@shape` line that sylow_amd/_shapes.py
parses and the Engine's table holds.  Its entry points are sylow_poseidon_*: the sets of names under the older prefixes are closed by the
tests of the nine other headers, and this header adds none."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sylow_poseidon.h")
NAMES = ["sylow_poseidon_table_words", "sylow_poseidon_prepare", "sylow_poseidon_permute_batch", "sylow_poseidon_permute_batch_tuned", "sylow_poseidon_hash_batch",
         "sylow_poseidon_hash_batch_tuned", "sylow_poseidon_merkle_build_batch", "sylow_poseidon_merkle_build_batch_tuned", "sylow_poseidon_merkle_open_batch",
         "sylow_poseidon_merkle_root_batch", "sylow_poseidon_merkle_verify_batch", "sylow_poseidon_merkle_verify_batch_tuned"]
HOST_ONLY = "sylow_poseidon_table_words"          # host arithmetic: no array, no stream
OTHER_HEADERS = ("sylow_hip.h", "sylow_hip_kzg_points.h", "sylow_hip_kzg_cosets.h", "sylow_hip_kzg_recover.h", "sylow_hip_kzg_cells.h", "sylow_hip_fr_scan.h",
                 "sylow_plonk.h", "sylow_popen.h", "sylow_pverify.h")


def declared():
    """{entry point: [parameter names]} of the header's prototypes, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.replace("*", " ").split()[-1] for p in " ".join(m.group(2).split()).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sylow_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sylow_poseidon.h"\n'
                   "int main(void) { return SYLOW_POSEIDON_T_MIN == 2 && SYLOW_POSEIDON_T_MAX == 17 && SYLOW_POSEIDON_DEPTH_MAX == 28 && SYLOW_HIP_OK == 0 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True, timeout=120)


def test_the_header_states_the_instance_and_the_contract():
    raw = open(HEADER).read()
    text = " ".join(re.sub(r"\n \*", " ", raw).split())          # the comment's line breaks do not matter
    assert '#include "sylow_hip.h"' in raw and "NO SYMBOL UNDER AN OLDER PREFIX IS ADDED" in text and "sylow_poseidon_" in text
    assert "R_P = 56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68" in text and "M IS NOT SYMMETRIC" in text
    assert "pin t = 2, 3, 4, 5, 7 and 17" in text and "THE OTHER WIDTHS REST ON THE SAME GENERATOR AND HAVE NO EXTERNAL KNOWN ANSWER OF THEIR OWN" in text
    assert "THE LIBRARY KEEPS NO HIDDEN STATE" in text and "A TABLE PREPARED FOR ANOTHER t IS A CONTRACT VIOLATION" in text
    assert "THE HOT CALLS NEVER SYNCHRONISE" in text and "SYNCHRONISES THE STREAM ONCE" in text
    assert "THE WORDS DEPEND ON NEITHER THE ROUTE NOR A PIN" in text and "NOTHING IS READ OUTSIDE THE ARRAYS" in text and "ok IS 0 WHEREVER status != 0" in text


def test_library_exports_what_the_header_declares():
    import sylow_amd
    from sylow_amd import _lib
    protos = declared()
    assert sorted(protos) == sorted(NAMES) and all(n.startswith("sylow_poseidon_") for n in protos)
    assert set(_lib.SIGNATURES_POSEIDON) == set(protos)
    tables = [_lib.SIGNATURES, _lib.SIGNATURES_KZG_POINTS, _lib.SIGNATURES_KZG_COSETS, _lib.SIGNATURES_KZG_RECOVER, _lib.SIGNATURES_KZG_CELLS, _lib.SIGNATURES_FR_SCAN,
              _lib.SIGNATURES_PLONK, _lib.SIGNATURES_POPEN, _lib.SIGNATURES_PVERIFY, _lib.SIGNATURES_POSEIDON]
    assert sum(len(t) for t in tables) == len(set().union(*tables)), "the ten tables are disjoint"
    others = [re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in OTHER_HEADERS]
    lib = sylow_amd.load()
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert (params[-1] == "stream") == (name != HOST_ONLY) and len(params) == len(_lib.SIGNATURES_POSEIDON[name]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_POSEIDON[name]
        assert not any(name in text for text in others), "the other headers do not declare them"
    exported = subprocess.run(["nm", "-D", "--defined-only", sylow_amd._lib.LIB_PATH], capture_output=True, text=True, check=True, timeout=120).stdout
    assert set(re.findall(r"\b(sylow_poseidon_\w+)\b", exported)) == set(NAMES), "the sylow_poseidon_* exports are exactly the declared names"
    assert set(re.findall(r"\b(sylow_pverify_\w+)\b", exported)) == set(_lib.SIGNATURES_PVERIFY), "and this header added no sylow_pverify_* export"
    assert set(re.findall(r"\b(sylow_popen_\w+)\b", exported)) == set(_lib.SIGNATURES_POPEN), "no sylow_popen_* export"
    assert set(re.findall(r"\b(sylow_plonk_\w+)\b", exported)) == set(_lib.SIGNATURES_PLONK), "no sylow_plonk_* export"
    assert set(re.findall(r"\b(sylow_hip_\w+)\b", exported)) == set().union(*tables[:6]), "and no sylow_hip_* export"
    assert len(_lib.SIGNATURES_PVERIFY) == 5 and len(_lib.SIGNATURES_POPEN) == 6 and len(_lib.SIGNATURES_PLONK) == 5, "the closed tables are as they were"
    for t, words in ((1, 0), (2, 528), (3, 816), (17, 6324), (18, 0), (-1, 0)):
        assert lib.sylow_poseidon_table_words(t) == words, t


def test_every_prototype_with_an_array_has_a_shape_line():
    from sylow_amd import _shapes
    protos, shapes = declared(), _shapes.parse(HEADER)
    assert HEADER == _shapes.HEADER_POSEIDON and set(shapes) == set(protos) - {HOST_ONLY}
    for other in (_shapes.HEADER, _shapes.HEADER_KZG_POINTS, _shapes.HEADER_KZG_COSETS, _shapes.HEADER_KZG_RECOVER, _shapes.HEADER_KZG_CELLS, _shapes.HEADER_FR_SCAN,
                  _shapes.HEADER_PLONK, _shapes.HEADER_POPEN, _shapes.HEADER_PVERIFY):
        assert not set(shapes) & set(_shapes.parse(other))
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert "*" not in re.search(r"\b" + HOST_ONLY + r"\s*\(([^)]*)\)", text).group(1), "the one prototype without a shape line takes no pointer"
    for name, (names, sh) in shapes.items():
        assert names == protos[name]
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        pointers = {p.replace("*", " ").split()[-1] for p in proto.split(",") if "*" in p} - {"stream"}
        assert set(sh) == pointers, (name, set(sh) ^ pointers)           # every pointer has an extent
        assert _shapes.table()[name][1].keys() == sh.keys()              # and the Engine checks it on every call
        assert not any("/" in s.expr for s in sh.values())
    optional = {n: sorted(p for p, s in sh.items() if s.optional) for n, (_, sh) in shapes.items() if any(s.optional for s in sh.values())}
    assert optional == {"sylow_poseidon_hash_batch": ["init"], "sylow_poseidon_hash_batch_tuned": ["init"], "sylow_poseidon_merkle_build_batch": ["root_out"],
                        "sylow_poseidon_merkle_build_batch_tuned": ["root_out"]}
    unsized = {n: sorted(p for p, s in sh.items() if s.expr == "*") for n, (_, sh) in shapes.items()}
    assert all(u == (["table_out"] if n.endswith("prepare") else [] if n.endswith("open_batch") else ["table"]) for n, u in unsized.items()), unsized
    v = {"t": 5, "k": 4, "n": 7, "m": 3, "depth": 4, "q": 6, "n_roots": 6}
    for name in NAMES[2:4]:
        assert shapes[name][1]["state"].nbytes(v) == 32 * 5 * 7 == shapes[name][1]["out"].nbytes(v)
    for name in NAMES[4:6]:
        sh = shapes[name][1]
        assert sh["inputs"].nbytes(v) == 32 * 4 * 7 and sh["init"].nbytes(v) == 32 * 7 == sh["out"].nbytes(v)
    for name in NAMES[6:8]:
        sh = shapes[name][1]
        assert sh["leaves"].nbytes(v) == 32 * 3 * 16 and sh["nodes_out"].nbytes(v) == 32 * 3 * 15 and sh["root_out"].nbytes(v) == 96
        assert sh["nodes_out"].nbytes(dict(v, depth=1)) == 96, "a tree of two leaves has one node"
    sh = shapes["sylow_poseidon_merkle_open_batch"][1]
    assert sh["leaves"].nbytes(v) == 1536 and sh["nodes"].nbytes(v) == 1440 and sh["tree"].nbytes(v) == 48 == sh["index"].nbytes(v)
    assert sh["siblings_out"].nbytes(v) == 32 * 4 * 6 and sh["status"].nbytes(v) == 6
    for name in NAMES[9:]:
        sh = shapes[name][1]
        assert sh["leaf"].nbytes(v) == 192 and sh["index"].nbytes(v) == 48 and sh["siblings"].nbytes(v) == 768 and sh["status"].nbytes(v) == 6
    assert shapes[NAMES[9]][1]["root_out"].nbytes(v) == 192
    for name in NAMES[10:]:
        assert shapes[name][1]["roots"].nbytes(v) == 192 and shapes[name][1]["roots"].nbytes(dict(v, n_roots=1)) == 32 and shapes[name][1]["ok"].nbytes(v) == 6


def test_the_unit_uses_the_shared_arithmetic_and_the_plan():
    unit = open(os.path.join(ROOT, "sylow_amd", "csrc", "poseidon.hip")).read()
    for shared in ("bn254_fr_acc.hpp", "bn254_fr_dev.hpp", "poseidon_plan.hpp"):
        assert f'#include "{shared}"' in unit
    assert "mul_acc(" in unit and "fr_reduce_wide(" in unit and "fr_mul(" in unit and "#pragma unroll 1" in unit
    assert "17 (r - 1)^2 + (r - 1) < 2^512" in unit and "static_assert(T_MAX <= 17" in unit, "the accumulator bound is restated where the mix relies on it"
    assert "hipStreamSynchronize" in unit.split("sylow_poseidon_prepare")[-1].split("sylow_poseidon_permute_batch_tuned")[0]
    assert unit.count("hipStreamSynchronize") == 1 and "hipDeviceSynchronize" not in unit, "the hot calls never synchronise"
    plan = open(os.path.join(ROOT, "sylow_amd", "csrc", "poseidon_plan.hpp")).read()
    assert "NARROW_T_MAX" in plan and "profiles/poseidon/" in plan
    makefile = open(os.path.join(ROOT, "sylow_amd", "csrc", "Makefile")).read()
    assert " poseidon " in makefile
