"""CPU: the planner of the KZG prover (sylow_amd/csrc/kzg_prove_plan.hpp) as a stand-alone program compiled with g++ under the address and
undefined-behaviour sanitizers -- chunk counts, grid sizes, the carry level, the commitment's route, polynomials per chunk under a byte
budget and the fallback, against expectations written out by hand (tests/cpp/kzg_prove_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kzg_prove_plan_geometry_and_routes(tmp_path):
    exe = str(tmp_path / "kzg_prove_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "kzg_prove_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
