"""CPU: the planner of Poseidon and its Merkle trees (sylow_amd/csrc/poseidon_plan.hpp) as a stand-alone program compiled with g++ under the
address and undefined-behaviour sanitizers -- widths, depths and tables, lane groups, tiles and grids, the level offsets (they tile
[0, n - 1) exactly for depth 1 .. 28), the route choice with its pins, and the saturating sizes (tests/cpp/poseidon_plan_test.cpp).  Host
code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_poseidon_plan_groups_grids_levels_routes_and_sizes(tmp_path):
    exe = str(tmp_path / "poseidon_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "poseidon_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
