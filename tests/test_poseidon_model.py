"""CPU: the Poseidon model (tests/poseidon_model.py) against published circomlib values (tests/golden/poseidon_kats.json): the hashes for
t = 2, 3, 4, 5, 7 and 17, four words of the t = 3 table (M is not symmetric), R_P per width, and the integers behind the accumulator bound
of the mix at t = 17.  The widths without a known answer of their own rest on the same generator; what is checked for them is the shape of
the draw."""
import json
import os

import pytest

import poseidon_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_kats.json")))


def test_the_field_and_the_partial_rounds():
    assert int(KATS["field"], 16) == P.R and P.R_F == 8
    assert {int(t): rp for t, rp in KATS["partial_rounds"].items()} == P.R_P and sorted(P.R_P) == list(range(2, 18))


def test_the_t3_table_words():
    C, M = P.params(3)
    k = {n: int(v, 16) for n, v in KATS["t3_table"].items()}
    assert C[0] == k["C[0]"] and M[0][0] == k["M[0][0]"] and M[0][1] == k["M[0][1]"] and M[1][0] == k["M[1][0]"]
    assert M[0][1] != M[1][0], "M is not symmetric: the transposed mix is another function"
    assert len(C) == (8 + 57) * 3 and len(P.table(3)) == (8 + 57) * 3 + 9


@pytest.mark.parametrize("kat", KATS["hashes"], ids=lambda k: "k%d_%d" % (len(k["inputs"]), k["inputs"][0]))
def test_known_answers(kat):
    assert P.hash(kat["inputs"]) == int(kat["hash"])
    assert P.hash(kat["inputs"]) == P.permute([0] + kat["inputs"])[0]


def test_the_widths_the_known_answers_cover():
    assert sorted({len(k["inputs"]) + 1 for k in KATS["hashes"]}) == [2, 3, 4, 5, 7, 17]


@pytest.mark.parametrize("t", range(2, 18))
def test_every_width_draws_canonical_distinct_parameters(t):
    consts, xs, ys = P.draws(t)
    assert len(consts) == (8 + P.R_P[t]) * t and all(0 <= c < P.R for c in consts)
    assert len(set(xs + ys)) == 2 * t and all((x + y) % P.R for x in xs for y in ys), "no sum is 0: every entry of M has an inverse"
    C, M = P.params(t)
    assert all(M[i][j] * (xs[i] + ys[j]) % P.R == 1 for i in range(t) for j in range(t))


def test_the_accumulator_bound_of_the_mix_at_t_17():
    """a row of the mix adds 17 products of canonical values into 16 limbs before one reduction (poseidon.hip)"""
    assert 17 * (P.R - 1) ** 2 + (P.R - 1) < 1 << 512
    assert 16 * P.R ** 2 < 1 << 512 and P.R ** 2 * 100 < 58 * (1 << 508), "the bound mul_acc states, and r^2 < 0.58 2^508"
    assert 28 * (P.R - 1) ** 2 >= 1 << 512, "the headroom ends well above 17 terms and below 28"


def test_init_chains_and_the_tree_helpers():
    assert P.hash([1, 2], init=5) == P.permute([5, 1, 2])[0] != P.hash([1, 2])
    leaves = list(range(10, 18))
    nodes = P.merkle_nodes(leaves)
    assert len(nodes) == 7 and nodes[0] == P.hash([10, 11]) and nodes[4] == P.hash([nodes[0], nodes[1]]) and nodes[6] == P.hash([nodes[4], nodes[5]])
    assert [P.level_offset(3, k) for k in (1, 2, 3)] == [0, 4, 6]
    for i in range(8):
        assert P.merkle_root(leaves[i], i, P.merkle_open(leaves, i)) == nodes[-1]
    assert P.merkle_root(leaves[0], 1, P.merkle_open(leaves, 0)) != nodes[-1]
