"""GPU: batched Poseidon and its Merkle trees (include/sylow_poseidon.h) bit-exact against the integer model (tests/poseidon_model.py).

  * the parameter table of every width, read back;
  * the published known answers through hash_batch on both routes;
  * hash and permute of every width on each route it has, at n = 1, 63 .. 65, 255 .. 257, 3 * 256 + 1 under max_blocks = 2 (the grid
    stride) and at the seams of the wide groups; rows hold 0, 1, r - 1, r, r + 1, 2^256 - 1 and random words; hash with a non-null init is
    element 0 of permute;
  * trees of depth 1, 2, 8, 9, 10 with m = 1 and 3: every node, root_out, and the same words with wide_max pinned to 0, 4 and 2^20;
  * build -> open -> root / verify round trips, one bad query among good ones, out-of-range queries, n_roots = 1 and q.

A batch is laid out from a pool of states per width whose model values are computed once and shared."""
import json
import os
import random
from functools import lru_cache

import numpy as np
import pytest

import poseidon_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_kats.json")))
R = P.R
TOP = (1 << 256) - 1
EDGES = (0, 1, R - 1, R, R + 1, TOP)
POOL = 23                        # states per width; prime, so that a batch lays them out differently against every group and block size
NARROW_T_MAX = 5                 # poseidon_plan.hpp; test_the_route_limit_is_the_plan_s reads it back
NARROW, WIDE = 0, 1
SIZES = (1, 63, 64, 65, 255, 256, 257)
STRIDE_N = 3 * 256 + 1
SEAMS = {3: (15, 16, 17), 5: (7, 8, 9), 6: (7, 8, 9), 7: (7, 8, 9), 8: (7, 8, 9), 17: (1, 2, 3)}
M64 = (1 << 64) - 1


def limbs(values):
    return np.array([[(int(v) >> (64 * k)) & M64 for k in range(4)] for v in values], dtype=np.uint64).reshape(-1, 4)


def ints(words):
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(w[i, k]) << (64 * k) for k in range(4)) for i in range(w.shape[0])]


def routes(t):
    return (NARROW, WIDE) if t <= NARROW_T_MAX else (WIDE,)


@lru_cache(maxsize=None)
def pool(t):
    """(states, their permutations, the hashes of their last t - 1 elements with init = 0): POOL states of width t"""
    rng = random.Random(0x9053 + t)
    states = []
    for p in range(POOL):
        s = [rng.randrange(1 << 256) for _ in range(t)]
        if p < 2 * len(EDGES):
            s[p % t] = EDGES[p % len(EDGES)]           # an edge value at a moving position
        if p == 2 * len(EDGES):
            s = [EDGES[i % len(EDGES)] for i in range(t)]
        states.append(s)
    return states, [P.permute(s) for s in states], [P.hash(s[1:]) for s in states]


def batch(t, n):
    """n states from the pool, item j = pool[(5 j + n) % POOL]"""
    pick = [(5 * j + n) % POOL for j in range(n)]
    states, perms, hashes = pool(t)
    rows = lambda src: limbs([v % (1 << 256) for j in pick for v in src[j]]).reshape(n, t, 4)
    return rows(states), limbs([v for j in pick for v in perms[j]]).reshape(n, t, 4), limbs([hashes[j] for j in pick])


@pytest.fixture(scope="module")
def tables(engine):
    return {t: engine.poseidon_table(t) for t in range(2, 18)}


def test_the_route_limit_is_the_plan_s():
    plan = open(os.path.join(ROOT, "sylow_amd", "csrc", "poseidon_plan.hpp")).read()
    assert "constexpr int NARROW_T_MAX = %d;" % NARROW_T_MAX in plan


@pytest.mark.gpu
def test_tables_match_the_model(engine, tables):
    for t in range(2, 18):
        want = limbs(P.table(t))
        assert tables[t].shape == want.shape == (engine.lib.sylow_poseidon_table_words(t) // 4, 4)
        assert np.array_equal(tables[t].download(), want), t


@pytest.mark.gpu
@pytest.mark.parametrize("route", [NARROW, WIDE, -1])
def test_known_answers(engine, tables, route):
    for kat in KATS["hashes"]:
        k = len(kat["inputs"])
        got = engine.poseidon_hash(tables[k + 1], limbs(kat["inputs"]).reshape(1, k, 4), route=route)
        assert ints(got) == [int(kat["hash"])], (kat["inputs"], route)


@pytest.mark.gpu
@pytest.mark.parametrize("t", range(2, 18))
def test_hash_and_permute_of_every_width_on_each_route(engine, tables, t):
    for route in routes(t):
        for n in SIZES + (STRIDE_N,) + SEAMS.get(t, ()):
            pins = {"route": route, "max_blocks": 2 if n == STRIDE_N else -1}
            states, perms, hashes = batch(t, n)
            assert np.array_equal(engine.poseidon_permute(tables[t], states, **pins), perms), (t, route, n, "permute")
            assert np.array_equal(engine.poseidon_hash(tables[t], states[:, 1:], **pins), hashes), (t, route, n, "hash")
            with_init = engine.poseidon_hash(tables[t], states[:, 1:], init=states[:, 0], **pins)
            assert np.array_equal(with_init, perms[:, 0]), (t, route, n, "hash with init = element 0 of permute")
    n = 65
    states, perms, hashes = batch(t, n)
    assert np.array_equal(engine.poseidon_permute(tables[t], states), perms) and np.array_equal(engine.poseidon_hash(tables[t], states[:, 1:]), hashes), "default route"


# ---- trees -----------------------------------------------------------------------------------------------------------------------------------
DEPTHS = (1, 2, 8, 9, 10)


@lru_cache(maxsize=None)
def forest(depth, m=3):
    """(leaves [m][n] as ints -- tree 0 opens with edge values --, nodes [m][n - 1] by the model)"""
    rng = random.Random(0x7EE + depth)
    n = 1 << depth
    leaves = [[rng.randrange(1 << 256) for _ in range(n)] for _ in range(m)]
    for i, e in enumerate(EDGES[:n]):
        leaves[0][i] = e
    return leaves, [P.merkle_nodes(row) for row in leaves]


def model_open(depth, j, index):
    """the siblings of leaf `index` of tree j of forest(depth), level 0 first, read from the forest's nodes (nothing is hashed again)"""
    leaves, nodes = forest(depth)
    levels = [[v % R for v in leaves[j]]] + [nodes[j][P.level_offset(depth, k):P.level_offset(depth, k) + (1 << (depth - k))] for k in range(1, depth + 1)]
    return [levels[k][(index >> k) ^ 1] for k in range(depth)]


def leaf_words(leaves):
    return limbs([v for row in leaves for v in row]).reshape(len(leaves), len(leaves[0]), 4)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
def test_trees_match_the_model_under_every_route_seam(engine, tables, depth):
    leaves, nodes = forest(depth)
    n = 1 << depth
    for m in (1, 3):
        want = limbs([v for row in nodes[:m] for v in row]).reshape(m, n - 1, 4)
        for wide_max in (-1, 0, 4, 1 << 20):
            got, roots = engine.poseidon_merkle_build(tables[3], leaf_words(leaves[:m]), wide_max=wide_max)
            assert got.shape == (m, n - 1, 4) and np.array_equal(got, want), (depth, m, wide_max)
            assert np.array_equal(roots, got[:, -1]), "root_out is the last node"
    got, _ = engine.poseidon_merkle_build(tables[3], leaf_words(leaves), wide_max=4, max_blocks=1)
    assert np.array_equal(got, limbs([v for row in nodes for v in row]).reshape(3, n - 1, 4)), "one block walks a level with a stride"


def built(engine, tables, depth, m=3):
    leaves, nodes = forest(depth)
    dleaves = engine.to_device(np.ascontiguousarray(leaf_words(leaves[:m]).transpose(0, 2, 1)))
    dnodes, droot = engine.poseidon_merkle_build_device(tables[3], dleaves, depth, m)
    return leaves, nodes, dleaves, dnodes, engine.from_device_soa(droot)[:m]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [5, 10])
def test_build_open_root_verify_round_trip(engine, tables, depth):
    leaves, nodes, dleaves, dnodes, roots = built(engine, tables, depth)
    n, m = 1 << depth, 3
    assert ints(roots) == [row[-1] for row in nodes]
    rng = random.Random(depth)
    queries = [(j, i) for j in range(m) for i in range(n)] if depth == 5 else [(rng.randrange(m), rng.randrange(n)) for _ in range(70)] + [(2, n - 1), (0, 0)]
    tree, index = [j for j, _ in queries], [i for _, i in queries]
    q = len(queries)
    sib, status = engine.poseidon_merkle_open(dleaves, dnodes, depth, m, tree, index)
    assert not status.any() and sib.shape == (q, depth, 4)
    assert ints(sib) == [s for j, i in queries for s in model_open(depth, j, i)], "the gather against the model"
    leaf = limbs([leaves[j][i] for j, i in queries])
    got, status = engine.poseidon_merkle_root(tables[3], leaf, index, sib)
    assert not status.any() and np.array_equal(got, roots[tree]), "every path leads to its tree's root"
    for route in (NARROW, WIDE, -1):
        ok, status = engine.poseidon_merkle_verify(tables[3], leaf, index, sib, roots[tree], route=route)
        assert ok.all() and not status.any(), route
        own = [k for k in range(q) if tree[k] == 0]                  # n_roots = 1: the queries of tree 0 against its root alone
        ok, status = engine.poseidon_merkle_verify(tables[3], leaf[own], [index[k] for k in own], sib[own], roots[:1], route=route)
        assert ok.all() and not status.any() and len(own) >= 2
        # one flipped sibling word, a wrong index bit, another tree's root: false for that query alone
        a, b, c = 1, q // 2, q - 1
        bad_sib, bad_index, bad_roots = sib.copy(), list(index), roots[tree].copy()
        bad_sib[a, depth - 1, 2] ^= np.uint64(1)
        bad_index[b] ^= 1 << (depth // 2)
        bad_roots[c] = roots[(tree[c] + 1) % m]
        ok, status = engine.poseidon_merkle_verify(tables[3], leaf, bad_index, bad_sib, bad_roots, route=route)
        assert not status.any() and [k for k in range(q) if not ok[k]] == sorted({a, b, c}), route
        assert P.merkle_root(leaves[tree[a]][index[a]], index[a], ints(bad_sib[a])) != nodes[tree[a]][-1], "the model agrees that the flip breaks the path"


@pytest.mark.gpu
def test_queries_out_of_range_read_nothing_and_fail(engine, tables):
    depth, m = 5, 3
    leaves, nodes, dleaves, dnodes, roots = built(engine, tables, depth)
    n = 1 << depth
    tree = [0, m, 1, (1 << 64) - 1, 2, 0]
    index = [3, 0, n, 5, (1 << 64) - 1, n - 1]
    bad = [0, 1, 1, 1, 1, 0]
    sib, status = engine.poseidon_merkle_open(dleaves, dnodes, depth, m, tree, index)
    assert list(status) == bad and not sib[[1, 2, 3, 4]].any() and ints(sib[0]) == model_open(depth, 0, 3) == P.merkle_open(leaves[0], 3) and ints(sib[5]) == model_open(depth, 0, n - 1)
    # the walk: an index of 2^depth or more sets the status, zeroes the row and fails the check, whatever the path holds
    leaf = limbs([leaves[0][3], 1, 2, leaves[0][5], 4, leaves[0][n - 1]])
    index2 = [3, 0, n, 5, (1 << 64) - 1, n - 1]
    sib2 = sib.copy()
    sib2[3] = limbs(model_open(depth, 0, 5))
    got, status = engine.poseidon_merkle_root(tables[3], leaf, index2, sib2)
    assert list(status) == [0, 0, 1, 0, 1, 0] and not got[[2, 4]].any() and ints(got[[0, 3, 5]]) == [nodes[0][-1]] * 3
    for route in (NARROW, WIDE):
        ok, status = engine.poseidon_merkle_verify(tables[3], leaf, index2, sib2, roots[:1], route=route)
        assert list(status) == [0, 0, 1, 0, 1, 0] and list(ok) == [1, 0, 0, 1, 0, 1], route
    zero_root = np.zeros((1, 4), dtype=np.uint64)
    ok, status = engine.poseidon_merkle_verify(tables[3], leaf[[2]], [n], sib2[[2]], zero_root)
    assert list(ok) == [0] and list(status) == [1], "ok is 0 wherever the status is set, even against the zero row"


@pytest.mark.gpu
def test_the_host_classes(engine):
    from sylow_amd import api
    api.set_engine(engine)
    h = api.Poseidon(3)
    assert ints(h.hash([[1, 2], [0, 0]])) == [int(KATS["hashes"][1]["hash"]), int(KATS["hashes"][2]["hash"])]
    assert ints(h.permute([[0, 1, 2]])[0])[0] == int(KATS["hashes"][1]["hash"])
    leaves, nodes = forest(5)
    tree = api.PoseidonMerkleTree(5, h)
    assert ints(tree.build(leaves)) == [row[-1] for row in nodes]
    sib, status = tree.open([7, 9], tree=[0, 2])
    assert not status.any()
    roots, _ = tree.root_of([leaves[0][7], leaves[2][9]], [7, 9], sib)
    assert ints(roots) == [nodes[0][-1], nodes[2][-1]]
    assert list(tree.verify([leaves[0][7], leaves[2][9]], [7, 9], sib)) == [True, False], "against the root of tree 0"
    assert list(tree.verify([leaves[0][7], leaves[2][9]], [7, 9], sib, roots=tree.roots[[0, 2]])) == [True, True]
