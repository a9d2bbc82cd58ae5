"""CPU: the planner of PLONK's quotient polynomial (sylow_amd/csrc/plonk_quotient_plan.hpp) as a stand-alone program compiled with g++ under
the address and undefined-behaviour sanitizers -- the rows of the table, the items and the tail tiles of the fused kernel (every point once
under max_blocks = 1, 5 and the default), the wrap of i + E, the degree bound and the tail the status reads, the chunks of whole instances
against a scratch limit (0, 1, m - 1 and m instances per chunk, and "not even one fits"), saturating sums and the pins refused
(tests/cpp/plonk_quotient_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plonk_quotient_plan_rows_items_bound_chunks_and_scratch(tmp_path):
    exe = str(tmp_path / "plonk_quotient_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "plonk_quotient_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
