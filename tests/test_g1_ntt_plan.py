"""CPU: the planner of the G1 transform (sylow_amd/csrc/g1_ntt_plan.hpp) as a stand-alone program compiled with g++ under the address and
undefined-behaviour sanitizers -- every index of every stage of every size below n, each output written once, the lane-to-butterfly map a
bijection, the ping-pong ending in `out`, saturating scratch sums, and window tables that depend on the grid and not on n
(tests/cpp/g1_ntt_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_g1_ntt_plan_indices_ping_pong_and_scratch(tmp_path):
    exe = str(tmp_path / "g1_ntt_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "g1_ntt_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
