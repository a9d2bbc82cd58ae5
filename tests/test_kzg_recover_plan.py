"""CPU: the planner of the cell recovery (sylow_amd/csrc/kzg_recover_plan.hpp) as a stand-alone program compiled with g++ under the address and
undefined-behaviour sanitizers -- the limits on (log_c, log_l), items, grids and LDS bytes at c = 1, around one block and at the largest
shapes, every (row, k) and every element of an upper half visited once, both layouts of the vanishing values, and saturating scratch sums
(tests/cpp/kzg_recover_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kzg_recover_plan_items_grids_layouts_and_scratch(tmp_path):
    exe = str(tmp_path / "kzg_recover_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "kzg_recover_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
