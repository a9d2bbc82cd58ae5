"""The input and memory contract for the entry points of include/sylow_poseidon.h (poseidon.hip).  They are declared in a header of their
own, under a prefix of their own, so their rows live here and not in the tables of tests/test_gpu_input_contract.py, which mirror
include/sylow_hip.h.

  * Every entry point runs between guard bands under two fill bytes (tests/guarded_engine.py, imported and subclassed: the prototypes of
    the new header are added to its constness table): no write outside an `@shape` extent, no modified const input, and no output byte
    left unwritten -- for n = 1 .. 65 on both routes, at widths whose wide groups have 1, 3 and 15 idle lanes, and the outputs equal the
    model's.  THE IDLE LANES OF A WIDE GROUP, AND THE GROUPS PAST n, ARE THE POINT: a store from one of them lands in a neighbour's
    element or in a guard band.
  * Every SYLOW_HIP_E_ARG case of the header, with nothing written; n = 0, m = 0 and q = 0 launch nothing, whatever the pointers."""
import re

import numpy as np
import pytest

import poseidon_model as P
import test_gpu_input_contract as T
import test_gpu_poseidon as G
from guarded_engine import FILLS, GuardedEngine
from test_poseidon_header import HEADER, HOST_ONLY

E_ARG = -2
SENTINEL = 0x5A5A5A5A5A5A5A5A
OUTPUTS = ("table_out", "out", "nodes_out", "root_out", "siblings_out", "status", "ok")


def prototypes():
    """{entry point: [(is a pointer, const, name)]} of the new header, the host-only size query aside"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+(sylow_poseidon_\w+)\s*\(([^)]*)\)\s*;", text):
        if m.group(1) != HOST_ONLY:
            out[m.group(1)] = [("*" in p, "const" in p.split(), p.replace("*", " ").split()[-1]) for p in " ".join(m.group(2).split()).split(",")]
    return out


def test_outputs_are_the_non_const_pointers():
    protos = prototypes()
    assert len(protos) == 11 and not set(protos) & set(T.CONTRACT), "include/sylow_hip.h does not declare them"
    for name, params in protos.items():
        pointers = [p for p in params if p[0] and p[2] != "stream"]
        assert all(p[1] == (p[2] not in OUTPUTS) for p in pointers) and any(not p[1] for p in pointers), name


class GuardedHasher(GuardedEngine):
    """GuardedEngine reads the constness of every pointer from include/sylow_hip.h; the prototypes of the new header are added to its table"""

    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream, fill)
        for name, params in prototypes().items():
            assert name not in self._const
            self._const[name] = {p: const for ptr, const, p in params if ptr}


@pytest.mark.gpu
@pytest.mark.parametrize("t", [3, 5, 17])                 # wide groups of 4, 8 and 32 lanes: 1, 3 and 15 idle
def test_hash_and_permute_stay_inside_their_buffers_for_n_1_to_65(engine, t):
    guarded = GuardedHasher(engine.device, engine.stream)
    seen = []
    for fill in FILLS:
        guarded.fill = fill
        table = guarded.poseidon_table(t)
        assert np.array_equal(table.download(), G.limbs(P.table(t)))
        for route in G.routes(t):
            for n in range(1, 66):
                states, perms, hashes = G.batch(t, n)
                assert np.array_equal(guarded.poseidon_permute(table, states, route=route), perms), (t, route, n)
                assert np.array_equal(guarded.poseidon_hash(table, states[:, 1:], route=route), hashes), (t, route, n)
        assert np.array_equal(guarded.poseidon_hash(table, states[:, 1:], init=states[:, 0]), perms[:, 0])
        assert np.array_equal(guarded.poseidon_hash(table, states[:, 1:], init=states[:, 0], route=G.WIDE), perms[:, 0])
        assert np.array_equal(guarded.poseidon_permute(table, states), perms), "the untuned entry points"
        seen.append(set(guarded.audited))
    want = {(n, p) for n, params in prototypes().items() for ptr, _, p in params
            if ptr and p != "stream" and ("permute" in n or "hash" in n or "prepare" in n)}
    assert seen[0] == seen[1] == want, want ^ seen[0]


@pytest.mark.gpu
def test_trees_and_paths_stay_inside_their_buffers(engine):
    guarded = GuardedHasher(engine.device, engine.stream)
    for fill in FILLS:
        guarded.fill = fill
        table = guarded.poseidon_table(3)
        for depth in (1, 2, 3, 5):
            leaves, nodes = G.forest(depth)
            n = 1 << depth
            for m in (1, 2, 3):
                want = G.limbs([v for row in nodes[:m] for v in row]).reshape(m, n - 1, 4)
                for wide_max in (-1, 0, 2, 1 << 20):
                    got, roots = guarded.poseidon_merkle_build(table, G.leaf_words(leaves[:m]), wide_max=wide_max)
                    assert np.array_equal(got, want) and np.array_equal(roots, want[:, -1]), (depth, m, wide_max)
            dleaves = guarded.to_device(np.ascontiguousarray(G.leaf_words(leaves).transpose(0, 2, 1)))
            dnodes, droot = guarded.poseidon_merkle_build_device(table, dleaves, depth, 3)
            roots = guarded.from_device_soa(droot)
            for q in (1, 2, 3, 5, 9, 65):
                tree, index = [k % 3 for k in range(q)], [(7 * k + 1) % n for k in range(q)]
                if q >= 5:
                    tree[2], index[4] = 3, n                          # out of range: a zero row, nothing read
                sib, status = guarded.poseidon_merkle_open(dleaves, dnodes, depth, 3, tree, index)
                bad = [int(tree[k] >= 3 or index[k] >= n) for k in range(q)]
                assert list(status) == bad
                leaf = G.limbs([leaves[tree[k] % 3][index[k] % n] for k in range(q)])
                got, status = guarded.poseidon_merkle_root(table, leaf, index, sib)
                good = [k for k in range(q) if not bad[k]]
                assert np.array_equal(got[good], roots[[tree[k] for k in good]])
                # the walk knows no trees: a path fails by its index or by its words (a zero row can be the true sibling of a small tree)
                walks = [int(index[k] < n and P.merkle_root(G.ints(leaf[k])[0], index[k], G.ints(sib[k])) == nodes[tree[k] % 3][-1]) for k in range(q)]
                assert all(walks[k] for k in good) and list(status) == [int(index[k] >= n) for k in range(q)]
                for route in (G.NARROW, G.WIDE, -1):
                    ok, status = guarded.poseidon_merkle_verify(table, leaf, index, sib, roots[[t % 3 for t in tree]], route=route)
                    assert list(ok) == walks and list(status) == [int(index[k] >= n) for k in range(q)], (depth, q, route)
                    guarded.poseidon_merkle_verify(table, leaf, index, sib, roots[:1], route=route)
    names = {n for n, _ in guarded.audited}
    assert {n for n in prototypes() if "merkle" in n} <= names, set(prototypes()) - names
    for name, params in prototypes().items():
        if "merkle" in name:
            pointers = {p for ptr, _, p in params if ptr and p != "stream"}
            assert pointers == {p for n, p in guarded.audited if n == name}, (name, pointers)


@pytest.mark.gpu
def test_argument_errors_write_nothing(engine):
    lib, st = engine.lib, engine.stream
    t, n, depth, m, q = 3, 5, 3, 2, 4
    fill = np.full(8192, SENTINEL, dtype=np.uint64)                 # every array is as large as the largest (a table has at most 6324 words)
    keys = ("table", "in", "init", "out", "leaves", "nodes", "root", "tree", "index", "sib", "leaf", "roots")
    arrays = {k: engine.to_device(fill) for k in keys}
    flags = {k: engine.to_device(np.full(64, 0x5A, dtype=np.uint8)) for k in ("status", "ok")}
    p = {k: d.ptr for k, d in list(arrays.items()) + list(flags.items())}
    bad = lambda rc: rc == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    sub = lambda lst, **kw: [kw.get("i%d" % k, v) for k, v in enumerate(lst)]
    calls = {
        "prepare": (lib.sylow_poseidon_prepare, [t, p["table"]]),
        "permute": (lib.sylow_poseidon_permute_batch, [p["table"], t, p["in"], n, p["out"]]),
        "permute_t": (lib.sylow_poseidon_permute_batch_tuned, [p["table"], t, p["in"], n, -1, -1, p["out"]]),
        "hash": (lib.sylow_poseidon_hash_batch, [p["table"], t - 1, p["in"], p["init"], n, p["out"]]),
        "hash_t": (lib.sylow_poseidon_hash_batch_tuned, [p["table"], t - 1, p["in"], p["init"], n, -1, -1, p["out"]]),
        "build": (lib.sylow_poseidon_merkle_build_batch, [p["table"], p["leaves"], depth, m, p["nodes"], p["root"]]),
        "build_t": (lib.sylow_poseidon_merkle_build_batch_tuned, [p["table"], p["leaves"], depth, m, -1, -1, p["nodes"], p["root"]]),
        "open": (lib.sylow_poseidon_merkle_open_batch, [p["leaves"], p["nodes"], depth, m, p["tree"], p["index"], q, p["sib"], p["status"]]),
        "root": (lib.sylow_poseidon_merkle_root_batch, [p["table"], p["leaf"], p["index"], p["sib"], depth, q, p["root"], p["status"]]),
        "verify": (lib.sylow_poseidon_merkle_verify_batch, [p["table"], p["leaf"], p["index"], p["sib"], depth, q, p["roots"], 1, p["ok"], p["status"]]),
        "verify_t": (lib.sylow_poseidon_merkle_verify_batch_tuned, [p["table"], p["leaf"], p["index"], p["sib"], depth, q, p["roots"], 1, -1, -1, p["ok"], p["status"]]),
    }
    run = lambda key, args: calls[key][0](*args, st)
    pointers = {k: [i for i, v in enumerate(full) if v in p.values()] for k, (_, full) in calls.items()}
    optional = {"hash": [3], "hash_t": [3], "build": [5], "build_t": [7]}                 # init and root_out may be NULL
    # NULL where an array is required
    for key, (_, full) in calls.items():
        for i in pointers[key]:
            rc = run(key, [None if k == i else v for k, v in enumerate(full)])
            assert (rc == 0) if i in optional.get(key, ()) else bad(rc), (key, i)
    engine.sync()
    for k in ("out", "nodes", "root"):                                                      # the three accepted calls wrote; refill
        arrays[k].upload(fill)
    # t (k) and depth out of range, whatever the batch size; the pins; n_roots
    for key, at, values in (("prepare", 0, (1, 18, 0, -1)), ("permute", 1, (1, 18, 0, -2)), ("permute_t", 1, (1, 18)), ("hash", 1, (0, 17, -1)), ("hash_t", 1, (0, 17)),
                            ("build", 2, (0, 29, -1)), ("build_t", 2, (0, 29)), ("open", 2, (0, 29)), ("root", 4, (0, 29)), ("verify", 4, (0, 29)), ("verify_t", 4, (0, 29))):
        full = calls[key][1]
        for v in values:
            assert bad(run(key, sub(full, **{"i%d" % at: v}))), (key, v)
            size_at = {"permute": 3, "permute_t": 3, "hash": 4, "hash_t": 4, "build": 3, "build_t": 3, "open": 6, "root": 5, "verify": 5, "verify_t": 5}.get(key)
            if size_at is not None:
                assert bad(run(key, sub(full, **{"i%d" % at: v, "i%d" % size_at: 0}))), (key, v, "an empty batch")
    for key, route_at in (("permute_t", 4), ("hash_t", 5), ("verify_t", 8)):
        full = calls[key][1]
        assert bad(run(key, sub(full, **{"i%d" % route_at: 2}))) and bad(run(key, sub(full, **{"i%d" % (route_at + 1): 0}))), key
    assert bad(run("build_t", sub(calls["build_t"][1], i5=0)))
    for n_roots in (0, 2, q + 1):
        assert bad(run("verify", sub(calls["verify"][1], i7=n_roots))) and bad(run("verify_t", sub(calls["verify_t"][1], i7=n_roots)))
    # an output that overlaps an input or another output, by byte ranges: one word in, and the last word of the range
    for key, (fn, full) in calls.items():
        params = prototypes()[fn.__name__]
        names = [n for _, _, n in params]
        const = {n for ptr, c, n in params if ptr and c}
        outs = [i for i in pointers[key] if names[i] not in const]
        ins = [i for i in pointers[key] if names[i] in const]
        assert outs and (ins or key == "prepare")
        for o in outs:
            for i in ins:
                assert bad(run(key, sub(full, **{"i%d" % o: full[i] + 8}))), (key, names[o], names[i])
            for o2 in outs:
                if o2 != o:
                    assert bad(run(key, sub(full, **{"i%d" % o: full[o2]}))), (key, names[o], names[o2])
    full = calls["permute"][1]
    assert bad(run("permute", sub(full, i4=p["in"] + 32 * t * n - 8))) and bad(run("permute", sub(full, i4=p["in"] - 32 * t * n + 8)))
    assert run("permute", sub(full, i4=p["in"] + 32 * t * n)) == 0, "the first byte past the input is free"
    engine.sync()
    arrays["in"].upload(fill)
    # n = 0, m = 0, q = 0: OK, nothing launched, whatever the pointers
    assert lib.sylow_poseidon_permute_batch(None, t, None, 0, None, st) == 0 and lib.sylow_poseidon_hash_batch(None, 2, None, None, 0, None, st) == 0
    assert lib.sylow_poseidon_merkle_build_batch(None, None, depth, 0, None, None, st) == 0
    assert lib.sylow_poseidon_merkle_open_batch(None, None, depth, m, None, None, 0, None, None, st) == 0
    assert lib.sylow_poseidon_merkle_root_batch(None, None, None, None, depth, 0, None, None, st) == 0
    assert lib.sylow_poseidon_merkle_verify_batch(None, None, None, None, depth, 0, None, 7, None, None, st) == 0
    engine.sync()
    for k, d in arrays.items():
        assert np.array_equal(d.download(), fill), f"{k}: nothing written"
    for k, d in flags.items():
        assert (d.download() == 0x5A).all(), k
