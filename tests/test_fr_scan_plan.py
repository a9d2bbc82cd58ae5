"""CPU: the planner of the scans over Fr and of PLONK's permutation grand product (sylow_amd/csrc/fr_scan_plan.hpp) as a stand-alone program
compiled with g++ under the address and undefined-behaviour sanitizers -- the items and the live lanes of tail chunks, the tile walk of phase
2 (every total visited once under totals_tile = 1, 2, the default and the maximum, for 0, 1, tile - 1, tile and tile + 1 chunks), the
one-chunk route, phase 3's items, saturating scratch and the pins refused (tests/cpp/fr_scan_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fr_scan_plan_items_tiles_routes_and_scratch(tmp_path):
    exe = str(tmp_path / "fr_scan_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "fr_scan_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
