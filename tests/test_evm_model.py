"""tests/evm_model.py before it may judge the GPU: the model against the reference's own test vectors (examples/reth_bn128.rs:229-502, held in
tests/golden/reference_kats.json), and the job generator against the conditions that keep it from degenerating.  CPU only."""
import pytest

import evm_model as M
from helpers import SEED

SEEDS = [SEED, SEED + 1, 0xA17B]          # the committed seed and two others: what SYLOW_TEST_SEED would select


@pytest.fixture(scope="module")
def vec(kats):
    lits = kats["eip_vectors_raw"]["hex_literals"]
    assert len(lits) == 20
    return {e["line"]: bytes.fromhex(e["hex"]) for e in lits}


def _show(name, res, want):
    print(f"  {name}: {res.error or res.out.hex()}  (reference: {want if isinstance(want, str) else want.hex()})")
    assert (res.error or res.out) == want, name


def test_reference_vectors_through_the_model(vec, coracle):
    """all 20 hex literals of the reference's tests, as tests/test_gpu_evm.py replays them, with the gas limits used there"""
    used = set()

    def v(line):
        used.add(line)
        return vec[line]
    add = [(v(230), 500, v(238)), (v(249), 500, v(257)), (v(268), 499, M.OUT_OF_GAS), (b"", 500, v(283)), (v(294), 500, M.FAILED_TO_CREATE)]
    for i, (data, limit, want) in enumerate(add):
        _show(f"ecAdd[{i}]", M.model_add(data, M.ADD_GAS, limit), want)
    mul = [(v(312), 40_000, v(319)), (v(330), 39_999, M.OUT_OF_GAS), (v(342), 40_000, v(349)), (b"", 40_000, v(361)), (v(372), 40_000, M.FAILED_TO_CREATE)]
    for i, (data, limit, want) in enumerate(mul):
        _show(f"ecMul[{i}]", M.model_mul(data, M.MUL_GAS, limit), want)
    full = 2 * M.PAIR_PER_POINT + M.PAIR_BASE
    pair = [(v(389), 260_000, v(406)), (v(419), full - 1, M.OUT_OF_GAS), (b"", 260_000, v(447)), (v(460), 260_000, M.FAILED_TO_CREATE), (v(483), 260_000, M.PAIR_LENGTH)]
    for i, (data, limit, want) in enumerate(pair):
        _show(f"ecPairing[{i}]", M.model_pair(data, M.PAIR_PER_POINT, M.PAIR_BASE, limit), want)
    assert used == set(vec), sorted(set(vec) - used)
    assert vec[283] == vec[361] == bytes(64) and vec[406] == vec[447] == (1).to_bytes(32, "big")
    # the vector that runs out of gas is a valid job: with enough gas it is the reference's answer for the same bytes (reth_bn128.rs:419)
    assert M.model_pair(vec[419], M.PAIR_PER_POINT, M.PAIR_BASE, full).out == (1).to_bytes(32, "big")


def test_model_order_of_checks():
    """the order the reference's `?` gives (reth_bn128.rs:127-217), on hand-made inputs"""
    w = lambda x: int(x).to_bytes(32, "big")
    g1, off, big = w(1) + w(2), w(1) + w(1), w(M.P) + w(2)
    assert M.model_add(off + big) == M.Result(None, M.FAILED_TO_CREATE, 1)           # point 1 is finished before point 2 is read
    assert M.model_add(big + off) == M.Result(None, M.NOT_A_MEMBER, 4)
    assert M.model_add(w(1) + w(M.P) + off) == M.Result(None, M.NOT_A_MEMBER, 4)
    assert M.model_add(g1 + off, 500, 499) == M.Result(None, M.OUT_OF_GAS, None)
    assert M.model_add(g1[:63]).error == M.FAILED_TO_CREATE                          # (1, 0) after padding
    assert M.model_add(g1 + bytes(64) + b"\xff" * 40).out == g1                      # truncated to 128 bytes
    assert M.model_mul(g1 + w(M.r)).out == bytes(64) and M.model_mul(g1 + w(M.r + 1)).out == g1
    assert M.model_mul(g1 + w(M.U256_MAX)).status == 0 and M.model_mul(off + w(M.U256_MAX)).status == 1
    g2 = b"".join(w(v) for v in (M.R.G2_GEN_AFF[0][1], M.R.G2_GEN_AFF[0][0], M.R.G2_GEN_AFF[1][1], M.R.G2_GEN_AFF[1][0]))
    bad_g2_word = g2[:96] + w(M.U256_MAX)
    assert M.model_pair(off + bad_g2_word) == M.Result(None, M.NOT_A_MEMBER, 4)       # six reads before either point
    assert M.model_pair(off + g2[:96] + w(5)) == M.Result(None, M.FAILED_TO_CREATE, 1)
    assert M.model_pair(off + g2 + big + g2) == M.Result(None, M.FAILED_TO_CREATE, 1)  # earlier pairs before later ones
    assert M.model_pair(g1 + g2 + b"\x00", gas_limit=0).error == M.OUT_OF_GAS         # gas before length
    assert M.model_pair(g1 + g2 + b"\x00").error == M.PAIR_LENGTH
    assert M.model_pair(bytes(192) + g1 + bytes(128) + bytes(64) + g2).out == (1).to_bytes(32, "big")   # identity pairs only (EIP-197)
    assert M.model_pair(bytes(64) + g2[:64] + bytes(64)).status == 1                 # two zero words: not the identity, not on the twist


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_pool_holds_every_class(seed, coracle):
    pool = M.build_pool(seed)
    counts = M.tag_counts(pool.add + pool.mul + pool.pair)
    need = M.required_tags()
    print(f"  seed {seed:#x}: {len(pool.add)} ecAdd, {len(pool.mul)} ecMul, {len(pool.pair)} ecPairing jobs; {len(need)} classes, "
          f"fewest: {sorted((counts[t], t) for t in need)[:5]}")
    assert len(set(need)) == len(need)
    short = {t: counts[t] for t in need if counts[t] < 3}
    assert not short, short
    for kind in ("add", "mul", "pair"):
        jobs, exp = getattr(pool, kind), M.expected(kind, seed)
        assert len(exp) == len(jobs)                                   # every generated job has its model row: none is left uncompared
        errors = M.Counter()
        for j, (host, dev) in zip(jobs, exp):
            assert host is not None and (host.error is None) != (host.out is None)
            errors[host.error] += 1
            want = [t for t in j.tags if t.startswith("expect.")]
            if want:                                                   # the defect a job was built with is the one the model finds
                assert dev.status == int(want[0][7:]) and dev.error == M.ERROR_OF_STATUS[dev.status] and host == dev, (j.tags, dev)
            if f"{kind}.valid" in j.tags:
                assert dev.status == 0 and dev.error is None, (j.tags, dev)
            if dev is None:
                assert kind == "pair" and len(j.data) % 192 and host.error in (M.PAIR_LENGTH, M.OUT_OF_GAS)
            if j.gas_limit is not None and j.gas_limit < M.cost_of(kind, j):
                assert host.error == M.OUT_OF_GAS
        print(f"    {kind}: {dict(errors)}")
        assert errors[M.OUT_OF_GAS] >= 2 and errors[M.NOT_A_MEMBER] >= 9 and errors[M.FAILED_TO_CREATE] >= 9 and errors[None] >= 20
    assert sum(h.error == M.PAIR_LENGTH for h, _ in M.expected("pair", seed)) >= 9
    # products that are one and that are not: by construction (sum a_i b_i = 0 mod r) and through the oracle's pairings
    valid = [(j, d) for j, (_, d) in zip(pool.pair, M.expected("pair", seed)) if d is not None and d.error is None]
    ones = sum(d.out == (1).to_bytes(32, "big") for _, d in valid)
    print(f"    valid ecPairing jobs: {len(valid)}, product one: {ones}")
    assert len(valid) / 3 <= ones <= 2 * len(valid) / 3
    for j, d in valid:
        if "pair.balanced" in j.tags or "pair.all_identity" in j.tags or "pair.size.0" in j.tags:
            assert d.out == (1).to_bytes(32, "big"), j.tags
        if "pair.unbalanced" in j.tags:
            assert d.out == bytes(32), j.tags
    # the ecMul pool's order: every defective point sits between two valid rows (a wrong row offset shows on both sides)
    exp = M.expected("mul", seed)
    nb = [i for i, j in enumerate(pool.mul) if "mul.defect_neighbour" in j.tags]
    assert all(exp[i][1].error and not exp[i - 1][1].error for i in nb)
