"""CPU: the planner of the weighted KZG and Groth16 checks (sylow_amd/csrc/weighted_plan.hpp) as a stand-alone program compiled with g++
under the address and undefined-behaviour sanitizers -- the parts of the two Fr sums (one part becomes two at 257 openings and at 2049
proofs; the cap of 256 parts from 524288 proofs on, which no GPU test reaches), every offset and the total of both leases against the chain
of pointers the launch code walked before, written out by hand, and a size that does not fit size_t saturating instead of wrapping
(tests/cpp/weighted_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weighted_plan_parts_offsets_and_saturation(tmp_path):
    exe = str(tmp_path / "weighted_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "weighted_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
