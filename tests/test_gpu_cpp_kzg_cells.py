"""The C ABI of the check of many cells of many blobs as one boolean called from C++ with raw device pointers through
include/sylow_hip_kzg_cells.h (tests/cpp/kzg_cells_host_test.cpp), compiled with g++ and run on the GPU at (log_c, log_l) = (2, 2): the Fr
half against words baked in from tests/kzg_cells_model.py, then real openings through the weighted check."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_cells_host_test.cpp")


def build_exe(exe):
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_kzg_cells_compiles(tmp_path):
    """CPU: the test builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    exe = str(tmp_path / "kzg_cells_host_test")
    build_exe(exe)
    assert os.path.exists(exe)


def test_the_baked_values_are_the_model_s():
    """CPU: the constants of the C++ source against tests/kzg_cells_model.py"""
    import re

    import kzg_cells_model as M
    src = open(SRC).read()

    def table(name):
        body = re.search(r"static const uint64_t " + name + r"\[\d+\]\[4\] = \{(.*?)\n\};", src, flags=re.S).group(1)
        rows = re.findall(r"\{([^{}]*)\}", body)
        return [sum(int(w.strip().rstrip("ul"), 0) << (64 * k) for k, w in enumerate(r.split(","))) for r in rows]

    idx, com = [0, 1, 1, 3, 2, 4, 1], [0, 1, 0, 1, 2, 0, 1]
    assert "f_idx = {0, 1, 1, 3, 2, 4, 1}, f_cm = {0, 1, 0, 1, 2, 0, 1}" in src
    assert "7919 * (k + 1) * (j + 1) + j * j + 1" in src and "k == 6 ? 0 : 1000003 * (k + 1) + 17" in src
    rows = [(idx[k], com[k], [7919 * (k + 1) * (j + 1) + j * j + 1 for j in range(4)], 0 if k == 6 else 1000003 * (k + 1) + 17) for k in range(7)]
    W, r, rz = M.scalars(rows, 2, 2, 2)
    assert table("W") == W and table("RZ") == rz and table("A") == M.fold(rows, 2, 2, 2) == M.fold_columns(rows, 2, 2, 2)
    assert r == [rows[k][3] if k < 4 else 0 for k in range(7)] and not M.in_range(rows, 2, 2)


@pytest.mark.gpu
def test_cpp_kzg_cells_runs(tmp_path):
    exe = str(tmp_path / "kzg_cells_host_test")
    build_exe(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    # the fold is the model's on the default form and both routes; the eight rows are accepted and in range; one altered value is rejected,
    # and accepted again with that row's weight 0; a row that names no cell clears the flag and is_one with it; the reduction's one row
    # holds under the single-point verifier; log_c + log_l = 28 and route = 2 are E_ARG
    assert lines["CELLS"] == "1 11 011 00 1 11"
