"""CPU: the planner of the multi-pair routes (sylow_amd/csrc/multi_plan.hpp) compiled with g++ -- table geometry, the slice rule, and the
job, chunk and Groth16 routes on grids, against expectations written out by hand (tests/cpp/multi_plan_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_multi_plan_routes_and_slices(tmp_path):
    exe = str(tmp_path / "multi_plan_test")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "multi_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
