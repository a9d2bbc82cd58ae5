"""CPU: the scratch limits tests/test_gpu_groth16_prove_routes.py sets ("holds k witnesses and not k + 1") are the rows
tests/cpp/groth16_prove_plan_test.cpp checks against the plan's own witnesses_per_chunk and prove_budget_bytes: the same shapes, limits and
chunk sizes, read out of the two files.  The program itself is built and run by tests/test_groth16_prove_plan.py.  The limit of the large
shape must also leave the G2 bucket route without a plan: that half is checked here against tools/msm_model.py."""
import os
import re
import sys

import test_gpu_groth16_prove_routes as routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import msm_model  # noqa: E402

CPP = os.path.join(ROOT, "tests", "cpp", "groth16_prove_plan_test.cpp")


def rows_of(width):
    """name -> tuple of the rows of `static const size_t ROUTE_LIMITS[][width] = { {..}, // name .. };`"""
    with open(CPP) as f:
        text = f.read()
    block = re.search(r"ROUTE_LIMITS\[\]\[%d\] = \{\n(.*?)\n\};" % width, text, re.S)
    assert block
    rows = re.findall(r"^\s*\{([0-9, ]+)\},\s*// (\w+)$", block.group(1), re.M)
    assert len(rows) == len(block.group(1).strip().split("\n")), "every line of the table is a row with its name"
    out = {name: tuple(int(x) for x in nums.split(",")) for nums, name in rows}
    assert len(out) == len(rows) and all(len(r) == width for r in out.values())
    return out


def test_the_prover_s_limits_are_the_rows_the_plan_test_checks():
    assert rows_of(6) == routes.ROUTE_LIMITS and len(routes.ROUTE_LIMITS) == 4


def test_the_plan_test_checks_every_row():
    """the program walks the whole table: witnesses_per_chunk, the budget on both sides of the limit, and the chunk sizes"""
    with open(CPP) as f:
        text = f.read()
    body = text[text.index("static void limits_of_the_route_tests()"):text.index("int main()")]
    assert "sizeof(ROUTE_LIMITS) / sizeof(ROUTE_LIMITS[0])" in body and "witnesses_per_chunk(" in body and "sizes == ROUTE_CHUNKS[i]" in body
    assert "prove_budget_bytes(log_n, n_vars, l, mc) <= limit && limit < prove_budget_bytes(log_n, n_vars, l, mc + 1)" in body
    assert "limits_of_the_route_tests();" in text[text.index("int main()"):]


def test_the_large_shape_takes_the_g2_bucket_route_by_default_and_not_under_its_limit():
    log_n, n_vars, l, m, limit, mc = routes.ROUTE_LIMITS["f_one"]
    assert n_vars >= msm_model.G2_DEFAULT_MIN and n_vars < msm_model.DEFAULT_MIN, "the G2 sum is a bucket sum, the G1 sums are not"
    c = msm_model.g2_default_window(n_vars)
    assert msm_model.g2_plan(n_vars, c) == (n_vars, msm_model.g2_scratch_bytes(c, n_vars)), "one chunk under the default budget"
    assert msm_model.g2_plan(n_vars, c, limit) is None and limit < msm_model.g2_fixed_bytes(c)
