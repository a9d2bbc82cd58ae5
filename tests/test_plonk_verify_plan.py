"""CPU: the planner of the batched PLONK verifier (sylow_amd/csrc/plonk_verify_plan.hpp) as a stand-alone program compiled with g++ under the
address and undefined-behaviour sanitizers -- T and the offsets of the terms in the header's order (every term once for several W and E),
the slots of a proof, the scratch sums of the scalars, of a chunk of the fold, of the per-proof flags and of the weighted form, each
saturating at the top, and the chunk rule: a limit that holds exactly one proof gives one, a byte less is refused, and whatever the budget
the chunk fits and one more proof does not (tests/cpp/plonk_verify_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plonk_verify_plan_terms_scratch_and_chunks(tmp_path):
    exe = str(tmp_path / "plonk_verify_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "plonk_verify_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
