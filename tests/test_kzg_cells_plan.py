"""CPU: the planner of the batched cell check (sylow_amd/csrc/kzg_cells_plan.hpp) as a stand-alone program compiled with g++ under the address
and undefined-behaviour sanitizers -- the limits, the route rule, the keys, the keyed multiply-accumulate walked as the kernel walks it
(every (key, column) once under every slice count, slices that partition a group, permutation and LDS indices in range for groups of 0, 1,
15, 16, 17 and 33 rows, at most 16 products per fold), the Horner chunks, saturating scratch, and the header's limit equal to the plan's
(tests/cpp/kzg_cells_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kzg_cells_plan_route_keys_slices_chunks_and_scratch(tmp_path):
    exe = str(tmp_path / "kzg_cells_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "kzg_cells_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
