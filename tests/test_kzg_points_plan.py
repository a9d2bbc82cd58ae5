"""CPU: the planner of the several-point KZG opening (sylow_amd/csrc/kzg_points_plan.hpp) as a stand-alone program compiled with g++ under
the address and undefined-behaviour sanitizers -- the limit on k, items and grids at 0, 1 and the caps, every scratch size at its edges and
where it saturates, the chunks of the G2 half under a byte budget and the layout of the verifier's lease, against expectations written out
by hand (tests/cpp/kzg_points_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kzg_points_plan_items_grids_scratch_and_chunks(tmp_path):
    exe = str(tmp_path / "kzg_points_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "kzg_points_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
