"""The C ABI of the recovery of a KZG polynomial from half of its cells called from C++ with raw device pointers through
include/sylow_hip_kzg_recover.h (tests/cpp/kzg_recover_host_test.cpp), compiled with g++ and run on the GPU: two blobs at
(log_c, log_l) = (2, 2) against values baked in from tests/kzg_recover_model.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kzg_recover_host_test.cpp")


def build_exe(exe):
    libdir = os.path.join(ROOT, "sylow_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                           "-L", libdir, "-lsylow_hip", f"-Wl,-rpath,{libdir}"])


def test_cpp_kzg_recover_compiles(tmp_path):
    """CPU: the test builds against the C ABI with plain g++."""
    import sylow_amd
    if not os.path.exists(sylow_amd._lib.LIB_PATH):
        sylow_amd.build()
    exe = str(tmp_path / "kzg_recover_host_test")
    build_exe(exe)
    assert os.path.exists(exe)


def test_the_baked_values_are_the_model_s():
    """CPU: the constants of the C++ source against tests/kzg_recover_model.py"""
    import re

    import kzg_recover_model as M
    src = open(SRC).read()

    def table(name):
        body = re.search(r"static const uint64_t " + name + r"\[\d+\]\[4\] = \{(.*?)\n\};", src, flags=re.S).group(1)
        rows = re.findall(r"\{([^{}]*)\}", body)
        return [sum(int(w.strip().rstrip("ul"), 0) << (64 * k) for k, w in enumerate(r.split(","))) for r in rows]

    n, c = 16, 4
    blobs = [[(j + 1) * 1000003 + 7919 * k * k + 1 if k < 8 else 0 for k in range(n)] for j in range(2)]
    ys = [M.fft(f, 4) for f in blobs]
    present = [[1, 0, 1, 1], [0, 1, 1, 0]]
    assert table("Y") == ys[0] + ys[1]
    vd, vc = zip(*[M.vanish(p, 2, 2)[:2] for p in present])
    assert table("ZD") == vd[0] + vd[1] and table("ZC") == vc[0] + vc[1]
    held = [[v if p[i % c] else (1 << 256) - 1 for i, v in enumerate(y)] for y, p in zip(ys, present)]
    assert [M.recover(y, p, 2, 2) for y, p in zip(held, present)] == [(M.OK, f) for f in blobs]
    held[0][4] += 1
    held[1][5] += 1
    assert M.recover(held[0], present[0], 2, 2) == (M.INCONSISTENT, table("BAD"))
    assert M.recover(held[1], present[1], 2, 2) == (M.OK, table("OTHER")) and table("OTHER") != blobs[1]


@pytest.mark.gpu
def test_cpp_kzg_recover_runs(tmp_path):
    exe = str(tmp_path / "kzg_recover_host_test")
    build_exe(exe)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    # the vanishing values are the model's; both blobs come back with status 0 and every cell restored; a changed value is status 2 with the
    # model's words below half and another blob at half; one cell of four is status 1 and a zero row; (13, 0) and (0, 0) are E_ARG
    assert lines["RECOVER"] == "1 11 11 1 11"
