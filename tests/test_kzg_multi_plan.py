"""CPU: the planner of the folded KZG openings (sylow_amd/csrc/kzg_multi_plan.hpp) as a stand-alone program compiled with g++ under the
address and undefined-behaviour sanitizers -- group offsets, tiles and grids at 0, 1 and the caps, scratch sizes, and the padded layout of
ragged groups under a byte budget, against expectations written out by hand (tests/cpp/kzg_multi_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kzg_multi_plan_geometry_scratch_and_chunks(tmp_path):
    exe = str(tmp_path / "kzg_multi_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "kzg_multi_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
