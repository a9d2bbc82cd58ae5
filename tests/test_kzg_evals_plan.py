"""CPU: the planner of the evaluation-form KZG unit (sylow_amd/csrc/kzg_evals_plan.hpp) and the lone-lane inversion beside it
(sylow_amd/csrc/bn254_fr_euclid.hpp) as a stand-alone program compiled with g++ under the address and undefined-behaviour sanitizers -- chunk
counts, live lanes, scan steps, grids, the overlap rule, scratch words, and binary-Euclid inverses against pasted values of Python's pow
(tests/cpp/kzg_evals_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kzg_evals_plan_geometry_scratch_and_lone_inversion(tmp_path):
    exe = str(tmp_path / "kzg_evals_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "kzg_evals_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
