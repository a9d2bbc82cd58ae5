"""The EVM precompile batches (sylow_hip_evm_ecadd_batch / _ecmul_batch / _ecpairing_batch, sylow_amd/evm.py) against the byte-level model
of tests/evm_model.py, job by job: output bytes or error name for every job of every call, and the raw per-element status of the C ABI.

The pool of tests/evm_model.py (a few hundred distinct jobs with named defect classes; tests/test_evm_model.py checks the model and the
pool on the CPU) is judged once by the model; the batches below are tiles and permutations of it, so every copy of a pool job has the
answer of its model row wherever it sits in a batch.  Output buffers are pre-filled with FILL before every raw call: a row that is never
written cannot pass for 64 zero bytes, a result of 0, or status OK."""
import numpy as np
import pytest

import evm_model as M
from helpers import SEED

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def pool(coracle):
    return M.build_pool(SEED)


@pytest.fixture(scope="module")
def exp(pool):
    """kind -> [(Result of the precompile under the job's gas limit, Result of the device entry point or None)] in pool order; the oracle's
    pairings for the ecPairing pool are paid here, once per session"""
    return {kind: M.expected(kind, SEED) for kind in ("add", "mul", "pair")}


def _filled(engine, n):
    return engine.to_device(np.full(max(n, 1), FILL, dtype=np.uint8))


def _perm(idx, salt):
    idx = np.asarray(idx)
    return idx[np.random.default_rng(SEED + salt).permutation(len(idx))].tolist()


def _report(bad, n, what):
    assert not bad, f"{what}: {len(bad)} of {n} rows differ from the model; first: {bad[:4]}"


# ---- ecAdd / ecMul ---------------------------------------------------------------------------------------------------------------------
FIXED = {"add": ("sylow_hip_evm_ecadd_batch", 128), "mul": ("sylow_hip_evm_ecmul_batch", 96)}


def raw_fixed(engine, kind, jobs, idx):
    """the C entry point on the rows idx of the pool (padded / truncated to the fixed length) -> (outputs, statuses)"""
    name, in_len = FIXED[kind]
    n = len(idx)
    d_in = engine.to_device(np.frombuffer(b"".join(M.right_pad(jobs[i].data, in_len) for i in idx), dtype=np.uint8))
    d_out, d_st = _filled(engine, 64 * n), _filled(engine, n)
    engine._call(name, d_in.ptr, d_out.ptr, d_st.ptr, n)
    out, st = d_out.download().tobytes(), d_st.download()
    return [out[64 * k:64 * k + 64] for k in range(n)], st[:n]


def check_fixed(engine, kind, jobs, exp, idx, what):
    """rows idx through the C entry point (output + raw status of every row) and through evm.run_add / run_mul (output or error under
    each job's own gas limit) -> the raw outputs"""
    from sylow_amd import evm
    outs, st = raw_fixed(engine, kind, jobs, idx)
    bad = []
    for k, i in enumerate(idx):
        dev = exp[i][1]
        want = dev.out if dev.error is None else bytes(64)               # a rejected row: its status, and 64 zero bytes
        if int(st[k]) != dev.status or outs[k] != want:
            bad.append((k, i, jobs[i].tags, int(st[k]), dev.status, outs[k].hex(), want.hex()))
    _report(bad, len(idx), f"{what} (C entry point)")
    run = evm.run_add if kind == "add" else evm.run_mul
    got = run(engine, [jobs[i].data for i in idx], M.cost_of(kind, None), [M.limit_of(kind, jobs[i]) for i in idx])
    bad = [(k, i, jobs[i].tags, g, exp[i][0]) for k, (i, g) in enumerate(zip(idx, got))
           if (getattr(g, "kind", None), g if isinstance(g, bytes) else None) != (exp[i][0].error, exp[i][0].out)]
    _report(bad, len(idx), f"{what} (evm.run_{kind})")
    return outs, st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ecadd_sizes(engine, pool, exp, n):
    """k_evm_ecadd, one lane per row: below, at and above one wavefront, and a second block with a tail (BLOCK = 256)"""
    idx = _perm(range(len(pool.add)), n)[:n] if n <= len(pool.add) else _perm(list(range(len(pool.add))) * 2, n)[:n]
    check_fixed(engine, "add", pool.add, exp["add"], idx, f"ecAdd n={n}")


def test_ecadd_pool_and_tiles(engine, pool, exp):
    every = list(range(len(pool.add)))
    check_fixed(engine, "add", pool.add, exp["add"], every, "ecAdd pool")
    tiled = _perm(every * 16, 1)
    assert len(tiled) > 3000
    a, sa = check_fixed(engine, "add", pool.add, exp["add"], tiled, "ecAdd pool x 16, permuted")
    other = _perm(every * 16, 2)
    assert other != tiled
    check_fixed(engine, "add", pool.add, exp["add"], other, "ecAdd pool x 16, another permutation")


def _both_mul_routes(engine, fn):
    """fn() on k_evm_ecmul_wide (eight lanes per row: the default up to SIGN_WIDE_MAX = 16384 rows) and on k_evm_ecmul (one lane per
    row: SIGN_WIDE_MAX = 0 sends every batch there, g1.hip sylow_hip_evm_ecmul_batch)"""
    prev = engine.get_option("SIGN_WIDE_MAX")
    try:
        engine.set_option("SIGN_WIDE_MAX", -1)
        wide = fn()
        engine.set_option("SIGN_WIDE_MAX", 0)
        lane = fn()
    finally:
        engine.set_option("SIGN_WIDE_MAX", prev)
    return wide, lane


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 65, 257])
def test_ecmul_sizes_both_routes(engine, pool, exp, n):
    """around one wavefront of k_evm_ecmul_wide (8 rows) and of k_evm_ecmul (64 rows), and past a block.  The rows are a window of the
    pool IN ORDER, where a defective point follows every scalar: a wrong row offset answers with the neighbour's status"""
    start = (37 * n) % (len(pool.mul) - n)
    idx = list(range(start, start + n))
    (wo, ws), (lo, ls) = _both_mul_routes(engine, lambda: check_fixed(engine, "mul", pool.mul, exp["mul"], idx, f"ecMul n={n}"))
    assert wo == lo and np.array_equal(ws, ls)


def test_ecmul_pool_both_routes(engine, pool, exp):
    """every scalar class of the pool (m r + d, 2^256 - 1, 2^255, p, the GLV edges) on both kernels.  The scalar rule is judged end to end,
    [k mod r] P: evm_read_scalar's subtraction of r alone cannot be seen from outside, because glv_decompose (bn254_pairing.hpp) subtracts r
    once more from whatever it is given"""
    every = list(range(len(pool.mul)))
    for idx, what in ((every, "ecMul pool"), (_perm(every * 5, 3), "ecMul pool x 5, permuted")):
        (wo, ws), (lo, ls) = _both_mul_routes(engine, lambda: check_fixed(engine, "mul", pool.mul, exp["mul"], idx, what))
        assert wo == lo and np.array_equal(ws, ls), what                          # the two routes agree byte for byte


# ---- ecPairing -------------------------------------------------------------------------------------------------------------------------
def raw_pair(engine, jobs, idx):
    """sylow_hip_evm_ecpairing_batch on the jobs idx (whole pairs only) -> (result, status); `in` is NULL when the batch holds no pair"""
    n = len(idx)
    counts = [len(jobs[i].data) // 192 for i in idx]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n_pairs = int(off[-1])
    d_in = engine.to_device(np.frombuffer(b"".join(jobs[i].data for i in idx), dtype=np.uint8)) if n_pairs else None
    d_off, d_res, d_st = engine.to_device(off), _filled(engine, n), _filled(engine, n)
    engine._call("sylow_hip_evm_ecpairing_batch", d_in.ptr if n_pairs else None, d_off.ptr, n, n_pairs, d_res.ptr, d_st.ptr)
    return d_res.download()[:n], d_st.download()[:n]


def shape(jobs, idx):
    return len(idx), sum(len(jobs[i].data) // 192 for i in idx)


def check_pair(engine, jobs, exp, idx, what, host=True):
    """the jobs idx through the C entry point (result + raw status of every job that holds whole pairs) and, with the host rules (gas, then
    length), through evm.run_pair: no job is left out of either comparison it can enter"""
    from sylow_amd import evm
    dev_idx = [i for i in idx if exp[i][1] is not None]
    res, st = raw_pair(engine, jobs, dev_idx)
    bad = []
    for k, i in enumerate(dev_idx):
        dev = exp[i][1]
        want = dev.out[-1] if dev.error is None else 0
        if int(st[k]) != dev.status or int(res[k]) != want:
            bad.append((k, i, jobs[i].tags, "status", int(st[k]), dev.status, "result", int(res[k]), want))
    _report(bad, len(dev_idx), f"{what} (C entry point)")
    if host:
        got = evm.run_pair(engine, [jobs[i].data for i in idx], M.PAIR_PER_POINT, M.PAIR_BASE, [M.limit_of("pair", jobs[i]) for i in idx])
        bad = [(k, i, jobs[i].tags, g, exp[i][0]) for k, (i, g) in enumerate(zip(idx, got))
               if (getattr(g, "kind", None), g if isinstance(g, bytes) else None) != (exp[i][0].error, exp[i][0].out)]
        _report(bad, len(idx), f"{what} (evm.run_pair)")
    return res, st


@pytest.fixture(scope="module")
def pair_sets(pool, exp):
    jobs, e = pool.pair, exp["pair"]
    dev = [i for i in range(len(jobs)) if e[i][1] is not None]
    return {"all": list(range(len(jobs))), "dev": dev,
            "valid": [i for i in dev if e[i][1].error is None], "defect": [i for i in dev if e[i][1].error is not None],
            "short": [i for i in dev if len(jobs[i].data) <= 192],                      # empty and one-pair jobs, valid or not
            "empty": [i for i in dev if not jobs[i].data]}


def _tables_batch(pair_sets):
    return _perm(pair_sets["all"] * 3, 10)


def _two_slot_batch(pool, pair_sets):
    base = pair_sets["all"] * 3
    n, k = shape(pool.pair, [i for i in base if len(pool.pair[i].data) % 192 == 0])
    extra = []
    while k + sum(len(pool.pair[i].data) // 192 for i in extra) >= 2 * (n + len(extra)) - 64:
        extra += pair_sets["short"]
    return _perm(base + extra, 11)


def test_ecpairing_pool_single_job_route(engine, pool, exp, pair_sets):
    """the pool as it is.  Route: single_job_product (multi_plan.hpp single_job_route: 1 <= n_pairs <= 6144 and n_jobs <= 1024) -- one
    wavefront per pair, one per job for the product and the final exponentiation"""
    n, k = shape(pool.pair, pair_sets["dev"])
    assert n <= 1024 and 1 <= k <= 6144, (n, k)
    check_pair(engine, pool.pair, exp["pair"], pair_sets["all"], "ecPairing pool")
    check_pair(engine, pool.pair, exp["pair"], _perm(pair_sets["all"], 12), "ecPairing pool, permuted")


def test_ecpairing_line_tables_route(engine, pool, exp, pair_sets):
    """the pool three times, permuted.  Route: multi_pairing_tables (more than 1024 jobs rules the single-job route out; use_tables: the
    average is two pairs or more, the slot count is the rounded-up average and longer jobs finish on the in-register tail of
    k_glued_from_tables).  The same batch in a second order: the answer of a job does not depend on its neighbours"""
    idx = _tables_batch(pair_sets)
    n, k = shape(pool.pair, [i for i in idx if exp["pair"][i][1] is not None])
    assert n > 1024 and k >= 2 * n, (n, k)
    check_pair(engine, pool.pair, exp["pair"], idx, "ecPairing pool x 3 (line tables)")
    other = _perm(pair_sets["all"] * 3, 13)
    assert other != idx
    check_pair(engine, pool.pair, exp["pair"], other, "ecPairing pool x 3, another permutation", host=False)


def test_ecpairing_two_slot_route(engine, pool, exp, pair_sets):
    """the same with copies of the empty and one-pair jobs mixed in until n_pairs < 2 n_jobs.  Route: use_tables declines (average below
    two), n_pairs <= 2 n_jobs selects k_multi_pairing<2> -- and the jobs of 9 and 17 pairs run through its two slots in chunks"""
    idx = _two_slot_batch(pool, pair_sets)
    dev = [i for i in idx if exp["pair"][i][1] is not None]
    n, k = shape(pool.pair, dev)
    sizes = {len(pool.pair[i].data) // 192 for i in dev}
    assert n > 1024 and k < 2 * n and {0, 1, 9, 17} <= sizes, (n, k, sizes)
    check_pair(engine, pool.pair, exp["pair"], idx, "ecPairing with short jobs mixed in (two-slot kernel)")


def test_ecpairing_forced_table_modes(engine, pool, exp, pair_sets):
    """MULTI_TABLES = 0: use_tables is false for every batch, so the three-times pool (more than two pairs per job) runs on
    k_multi_pairing<KMAXW>, the four-slot in-register schedule.  MULTI_TABLES = 1: tables for every job size, so the batch that averages
    below two pairs gets one-slot tables and every longer job the in-register tail"""
    big, short = _tables_batch(pair_sets), _two_slot_batch(pool, pair_sets)
    n, k = shape(pool.pair, [i for i in big if exp["pair"][i][1] is not None])
    assert n > 1024 and k > 2 * n
    prev = engine.get_option("MULTI_TABLES")
    try:
        engine.set_option("MULTI_TABLES", 0)
        r0 = check_pair(engine, pool.pair, exp["pair"], big, "ecPairing pool x 3, MULTI_TABLES=0 (k_multi_pairing<KMAXW>)", host=False)
        engine.set_option("MULTI_TABLES", 1)
        r1 = check_pair(engine, pool.pair, exp["pair"], short, "ecPairing short mix, MULTI_TABLES=1 (one-slot tables)", host=False)
        r2 = check_pair(engine, pool.pair, exp["pair"], big, "ecPairing pool x 3, MULTI_TABLES=1", host=False)
    finally:
        engine.set_option("MULTI_TABLES", prev)
    assert np.array_equal(r0[0], r2[0]) and np.array_equal(r0[1], r2[1])


@pytest.mark.parametrize("n", [193, 1345])
def test_ecpairing_defects_at_block_edges(engine, pool, exp, pair_sets, n):
    """valid jobs with a defective job first, last and at every multiple of 64: the status of a wavefront's first job stays its own.
    193 jobs: the single-job route; 1345: line tables (valid pool jobs average above two pairs)"""
    rng = np.random.default_rng(SEED + n)
    valid, defect = pair_sets["valid"], pair_sets["defect"]
    idx = [int(rng.choice(defect)) if (j % 64 == 0 or j == n - 1) else int(rng.choice(valid)) for j in range(n)]
    check_pair(engine, pool.pair, exp["pair"], idx, f"ecPairing n={n}, defects at 0, 64, ..., last")
    st = raw_pair(engine, pool.pair, idx)[1]
    assert [j for j in range(n) if st[j]] == [j for j in range(n) if j % 64 == 0 or j == n - 1]


def test_ecpairing_every_job_defective(engine, pool, exp, pair_sets):
    """no valid job at all: as the pool holds them (single-job route) and five times over (line tables)"""
    d = pair_sets["defect"]
    check_pair(engine, pool.pair, exp["pair"], d, "ecPairing defects only")
    idx = _perm(d * 5, 14)
    assert len(idx) > 1024
    res, st = check_pair(engine, pool.pair, exp["pair"], idx, "ecPairing defects only x 5")
    assert st.all() and not res.any()


@pytest.mark.parametrize("n", [1, 5, 1500])
def test_ecpairing_only_empty_jobs(engine, pool, exp, pair_sets, n):
    """n_pairs = 0, `in` = NULL.  No pair: single_job_route and use_tables both decline, k_multi_pairing<2> runs over jobs that hold
    nothing and every job answers 1 (EIP-197: the empty product); evm.run_pair passes NULL too"""
    from sylow_amd import evm
    idx = [pair_sets["empty"][j % len(pair_sets["empty"])] for j in range(n)]
    res, st = check_pair(engine, pool.pair, exp["pair"], idx, f"ecPairing {n} empty jobs")
    assert res.tolist() == [1] * n and st.tolist() == [0] * n
    assert evm.run_pair(engine, [b""] * n) == [(1).to_bytes(32, "big")] * n
