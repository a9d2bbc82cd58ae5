"""CPU: the planner of PLONK's closing rounds (sylow_amd/csrc/plonk_open_plan.hpp) as a stand-alone program compiled with g++ under the
address and undefined-behaviour sanitizers -- the rows of the coefficient table, the slots of the evaluations and of the weights, the items
of the evaluation kernel over chunks of 2048 coefficients (every coefficient once under max_blocks = 1, 5 and the default, a row two and
three coefficients past a chunk, dead items past a shorter row), the tiles of the fused kernel (259 columns: three past a tile), the chunks
of whole instances against a scratch limit (0, 1, m - 1 and m instances per chunk, and "not even one fits": the refusal), saturating sums and
the pins refused (tests/cpp/plonk_open_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plonk_open_plan_slots_items_tiles_chunks_and_scratch(tmp_path):
    exe = str(tmp_path / "plonk_open_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "plonk_open_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
