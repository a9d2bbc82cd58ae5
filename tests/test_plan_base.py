"""CPU: what every plan header counts with (sylow_amd/csrc/plan_base.hpp) as a stand-alone program compiled with g++ under the address and
undefined-behaviour sanitizers -- the saturating product and sum at the sentinel, on both sides of SAT / b and with a zero operand, the
elements of a domain, the two range tests where they agree and where they must differ (an empty range inside a non-empty one), and the
aliasing table of an entry point with a NULL output, an output over a later output and an output over an input
(tests/cpp/plan_base_test.cpp).  Host code only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_base_saturation_ranges_and_the_aliasing_table(tmp_path):
    exe = str(tmp_path / "plan_base_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "plan_base_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
