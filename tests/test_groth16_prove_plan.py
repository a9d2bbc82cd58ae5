"""CPU: the planner of the Groth16 prover (sylow_amd/csrc/groth16_prove_plan.hpp) as a stand-alone program compiled with g++ under the
address and undefined-behaviour sanitizers -- lanes per row, grid sizes, scratch words, witnesses per chunk under a byte budget and the
case where none fits, against expectations written out by hand (tests/cpp/groth16_prove_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_groth16_prove_plan_lanes_grids_scratch_and_chunks(tmp_path):
    exe = str(tmp_path / "groth16_prove_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "groth16_prove_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
