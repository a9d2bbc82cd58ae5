"""CPU: the planner of the KZG proofs on every coset of the domain (sylow_amd/csrc/kzg_cosets_plan.hpp) as a stand-alone program compiled with
g++ under the address and undefined-behaviour sanitizers -- every index of every step in range, each column of each buffer written once per
step under every legal planes_log, residue slices that partition 0 .. l - 1, every read meeting what the step before wrote, the ping-pong
ending where the closing kernel reads, saturating sums, and a default plane count that depends on (c, m, l, grid) alone
(tests/cpp/kzg_cosets_plan_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kzg_cosets_plan_indices_planes_ping_pong_and_scratch(tmp_path):
    exe = str(tmp_path / "kzg_cosets_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "kzg_cosets_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
