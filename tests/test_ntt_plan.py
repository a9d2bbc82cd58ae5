"""CPU: the planner of the Fr transform (sylow_amd/csrc/ntt_plan.hpp) as a stand-alone program compiled with g++ under the address and
undefined-behaviour sanitizers -- pass counts, the uneven last pass, tiles, items and the grid cap, table and scratch words with their
saturation, the ping-pong and n^-1, against expectations written out by hand (tests/cpp/ntt_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntt_plan_geometry_and_scratch(tmp_path):
    exe = str(tmp_path / "ntt_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "ntt_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
