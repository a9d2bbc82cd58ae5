"""CPU: the scratch limits tests/test_gpu_plonk_prover_routes.py sets ("holds k instances and not k + 1") are the rows
tests/cpp/plonk_open_plan_test.cpp and tests/cpp/plonk_quotient_plan_test.cpp check against the plan's own instances_per_chunk,
open_budget_bytes and chunk_budget_bytes: the same shapes, limits and chunk sizes, read out of the three files.  The two programs themselves
are built and run by tests/test_plonk_open_plan.py and tests/test_plonk_quotient_plan.py."""
import os
import re

import test_gpu_plonk_prover_routes as routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_of(cpp, width):
    """name -> tuple of the rows of `static const size_t ROUTE_LIMITS[][width] = { {..}, // name .. };` in tests/cpp/<cpp>"""
    with open(os.path.join(ROOT, "tests", "cpp", cpp)) as f:
        text = f.read()
    block = re.search(r"ROUTE_LIMITS\[\]\[%d\] = \{\n(.*?)\n\};" % width, text, re.S)
    assert block, cpp
    rows = re.findall(r"^\s*\{([0-9, ]+)\},\s*// (\w+)$", block.group(1), re.M)
    assert len(rows) == len(block.group(1).strip().split("\n")), "every line of the table is a row with its name"
    out = {name: tuple(int(x) for x in nums.split(",")) for nums, name in rows}
    assert len(out) == len(rows) and all(len(r) == width for r in out.values())
    return out


def test_the_opening_route_s_limits_are_the_rows_the_plan_test_checks():
    assert rows_of("plonk_open_plan_test.cpp", 9) == routes.OPEN_LIMITS and len(routes.OPEN_LIMITS) == 4


def test_the_quotient_route_s_limits_are_the_rows_the_plan_test_checks():
    assert rows_of("plonk_quotient_plan_test.cpp", 7) == routes.QUOTIENT_LIMITS and len(routes.QUOTIENT_LIMITS) == 2


def test_the_plan_tests_check_every_row():
    """both programs walk the whole table: instances_per_chunk, the budget on both sides of the limit, and the chunk sizes"""
    for cpp in ("plonk_open_plan_test.cpp", "plonk_quotient_plan_test.cpp"):
        with open(os.path.join(ROOT, "tests", "cpp", cpp)) as f:
            text = f.read()
        body = text[text.index("static void limits_of_the_route_tests()"):text.index("int main()")]
        assert "sizeof(ROUTE_LIMITS) / sizeof(ROUTE_LIMITS[0])" in body and "instances_per_chunk(" in body and "sizes == ROUTE_CHUNKS[i]" in body, cpp
        assert "limits_of_the_route_tests();" in text[text.index("int main()"):], cpp
