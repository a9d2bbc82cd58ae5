"""GPU: the Groth16 prover (groth16_prove.hip) past one block, one chunk, one lane group and one shape of circuit, word for word against the
integer model of tests/groth16_prove_model.py and Python integers.  Which shape was chosen for which edge:

the proving route
  (a) circuit n8 (3, 8, 7, 2), m = 7 witnesses that differ from their neighbours (the satisfied one, the zero one, random words), distinct
      r and s: unchunked, in chunks of 3, 3, 1 and of 2, 2, 2, 1 -- the offsets z + j0 4 n_vars and j0 + j of prove_chunk and
      k_g16_close_prep, a ragged last chunk, and the verifier's flags against the model's
  (b) n8, m = 513: two full blocks and one lane through k_g16_close_prep, k_g16_close_put and the 4 mc / 5 mc split of k_g16_close_gather;
      the edge words among r and s; rows whose A, B or C is the identity BY DESIGN in every block (the zero witness under the randomness of
      groth16_prove_model.planted_randomness), so that a flag in the wrong row shows; unchunked and in chunks of 257, 256
  (c) (2, 3, 4, 3) with no free variable: no private variable at all, l_query and its flags NULL, the sum over l_query of n = 0 terms
  (d) no constraint at log_n 0 and 1: rows = nnz = 0, every col and val NULL (and h_query too at log_n 0), under the circuit's own key
      (A = alpha + r delta) and under a free key (the sums over z still count)
  (e) (3, 5, 7, 2): three padding rows of the domain
  (f) 2^16 + 3 variables on a domain of 8 under a free key: the G2 sum takes the bucket route inside the prover (its own lease on top of the
      prover's, on the prover's stream); once more under a limit that holds one witness and leaves that route without a plan

the sparse product
  (g) m = 65537 vectors: the grid's y is 65535 rows, two arrays are reached by the stride
  (h) 2^6 lanes per row and n_out = 4 2^20 + 5: 2^20 + 2 row blocks on a grid of 2^20, live rows on both sides of the wrap
  (i) every product (r - 1)^2, rows of L entries per lane around the 16 of a fold and the 27 that 512 bits hold, on every lane pin

Where many points are expected they are the library's fixed-base generator products of the model's logarithms (tests/test_gpu_groups.py pins
those to the oracle), and a sample of rows is the oracle's too.  Every scratch limit is a row of ROUTE_LIMITS;
tests/cpp/groth16_prove_plan_test.cpp holds the same rows and checks them against the plan (tests/test_groth16_prove_route_limits.py
compares the two).  A chunked run proves the witnesses in REVERSED order: its output buffers then cannot hold the right words by accident,
left there by the unchunked run before it.

Not covered: the grid strides of k_fr_canon, k_fr_slice and k_g16_quot_coset (2^28 elements, 8 GB), and the G1 bucket route inside the prover
(2^18 variables, three queries of 262 144 points)."""
import os
import random
import sys

import numpy as np
import pytest

import groth16_prove_model as M
from groth16_prove_model import EDGE_WORDS, R
from test_gpu_groth16_prove import SENTINEL, batch, circuit, csr_arrays, prove, verify, words

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import msm_model  # noqa: E402

pytestmark = pytest.mark.gpu
# name -> (log_n, n_vars, n_inputs, m, the limit in bytes, the witnesses of a full chunk under it)
ROUTE_LIMITS = {
    "a_three": (3, 7, 2, 7, 16000, 3),
    "a_two": (3, 7, 2, 7, 12000, 2),
    "b_257": (3, 7, 2, 513, 1350000, 257),
    "f_one": (3, 65539, 2, 2, 6000000, 1),
}


def limit_for(name, ct, m):
    log_n, n_vars, l, rows, limit, _ = ROUTE_LIMITS[name]
    assert (log_n, n_vars, l, rows) == (ct.log_n, ct.n_vars, ct.l, m), "the row is this call's shape"
    return limit


def prove_reversed_under(engine, limit, ct, key, zs, rs, ss):
    """the same proofs under a scratch limit, proved last witness first and handed back in the caller's order"""
    try:
        engine.set_scratch_limit(limit)
        got = prove(engine, ct, key, zs[::-1], rs[::-1], ss[::-1])
    finally:
        engine.set_scratch_limit(0)
    return tuple((xy[::-1], inf[::-1]) for xy, inf in got)


def assert_same(got, want, what):
    for name, (x, xi), (y, yi) in zip("ABC", got, want):
        x, y, xi, yi = np.asarray(x), np.asarray(y), np.asarray(xi), np.asarray(yi)
        assert x.shape == y.shape and xi.shape == yi.shape, (what, name)
        bad = np.flatnonzero((x != y).any(axis=1) | (xi != yi))
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} of {len(xi)} rows, first {bad[:8].tolist()}"


def model_dlogs(st, zs, rs, ss):
    return [st.proof_dlogs(z, r, s) for z, r, s in zip(zs, rs, ss)]


def generator_points(engine, dlogs):
    """the proofs as the library's fixed-base products of the model's logarithms"""
    return (engine.g1_generator_mul(words([d[0] for d in dlogs])), engine.g2_generator_mul(words([d[1] for d in dlogs])),
            engine.g1_generator_mul(words([d[2] for d in dlogs])))


def assert_rows_are_the_oracle_s(got, dlogs, rows):
    want = M.proof_points([dlogs[j] for j in rows])
    assert_same(tuple((np.asarray(xy)[rows], np.asarray(inf)[rows]) for xy, inf in got), want, f"rows {rows} against the oracle")


def model_verifies(st, dlogs, zs, l):
    return [st.verifies(d, z[1:l + 1]) for d, z in zip(dlogs, zs)]


# ---- (a) distinct witnesses through ragged chunks ------------------------------------------------------------------------------------------
def test_distinct_witnesses_through_ragged_chunks(engine):
    ct, z, st, key, vk = circuit(engine, "n8")
    m, rng = 7, random.Random(0x6A1)
    zs = M.witness_mix(ct, z, m, seed=0x6A2)
    rs, ss = [rng.randrange(1, R) for _ in range(m)], [rng.randrange(1, R) for _ in range(m)]
    assert len(set(rs + ss)) == 2 * m
    dlogs = model_dlogs(st, zs, rs, ss)
    assert len(set(dlogs)) == m, "every row has a proof of its own"
    want = M.proof_points(dlogs)                                     # 21 points: all from the oracle
    got = prove(engine, ct, key, zs, rs, ss)
    assert_same(got, want, "unchunked")
    ok = model_verifies(st, dlogs, zs, ct.l)
    assert True in ok and False in ok and ok == [ct.satisfied([v % R for v in w]) for w in zs]
    assert list(verify(engine, vk, got, zs, ct.l)) == ok, "the verifier accepts exactly the rows the model's equation accepts"
    for name in ("a_three", "a_two"):
        part = prove_reversed_under(engine, limit_for(name, ct, m), ct, key, zs, rs, ss)
        assert_same(part, got, f"{name} against the unchunked call")
        assert_same(part, want, f"{name} against the model")
        assert list(verify(engine, vk, part, zs, ct.l)) == ok, name


# ---- (b) the closing kernels past one block -------------------------------------------------------------------------------------------------
PLANTED = {7: "zero", 130: "A", 255: "A", 257: "B", 300: "C", 400: "B", 512: "zero"}    # row -> the point that is the identity there ("zero": r = s = 0, C)


def test_the_closing_kernels_past_one_block(engine):
    ct, z, st, key, vk = circuit(engine, "n8")
    m, rng = 513, random.Random(0x6B1)
    zs = M.witness_mix(ct, z, m, seed=0x6B2, zero_rows=tuple(PLANTED))
    rs, ss = [rng.randrange(1, R) for _ in range(m)], [rng.randrange(1, R) for _ in range(m)]
    for k, e in enumerate(EDGE_WORDS):                               # the edge words among r and s, on both sides of the block boundaries
        rs[250 + 2 * k], ss[251 + 2 * k], rs[505 + k], ss[511 - k] = e, e, e, EDGE_WORDS[(k + 3) % 7]
    for row, what in PLANTED.items():
        rs[row], ss[row] = (0, 0) if what == "zero" else M.planted_randomness(st, what, rng)
    dlogs = model_dlogs(st, zs, rs, ss)
    flags = [[int(d[k] == 0) for d in dlogs] for k in range(3)]     # asserted on the CPU first: the planted rows and no other
    assert [np.flatnonzero(f).tolist() for f in flags] == [[130, 255], [257, 400], [7, 300, 512]]
    want = generator_points(engine, dlogs)
    assert [np.asarray(w[1]).tolist() for w in want] == flags
    sample = sorted({0, 255, 256, m - 1} | set(PLANTED))
    assert_rows_are_the_oracle_s(want, dlogs, sample)
    got = prove(engine, ct, key, zs, rs, ss)
    assert_same(got, want, "unchunked")
    assert [np.asarray(g[1]).tolist() for g in got] == flags, "every flag in its own row"
    assert_rows_are_the_oracle_s(got, dlogs, sample)
    part = prove_reversed_under(engine, limit_for("b_257", ct, m), ct, key, zs, rs, ss)     # chunks of 257 and 256: the second starts inside block 1
    assert_same(part, got, "chunks of 257, 256 against the unchunked call")
    assert_same(part, want, "chunks of 257, 256 against the model")


# ---- (c), (d), (e) shapes the entry point admits -------------------------------------------------------------------------------------------
def small_case(shape, seed, free=1, free_key=False):
    log_n, n_cons, n_vars, l = shape
    ct, z = M.make_circuit(log_n, n_cons, n_vars, l, seed=seed, free=free)
    st = M.free_key(ct, seed + 1) if free_key else M.Setup(ct, seed + 1)
    return ct, z, st, M.key_points(st)


def prove_and_check(engine, ct, st, key, zs, rs, ss, verifies=True):
    dlogs = model_dlogs(st, zs, rs, ss)
    got = prove(engine, ct, key, zs, rs, ss)
    assert_same(got, M.proof_points(dlogs), "against the model")
    if verifies:
        ok = model_verifies(st, dlogs, zs, ct.l)
        assert ok == [ct.satisfied([v % R for v in w]) for w in zs]
        assert list(verify(engine, M.vk_points(st), got, zs, ct.l)) == ok
    return got, dlogs


def test_no_private_variable(engine):
    ct, z, st, key = small_case((2, 3, 4, 3), 0x6C1, free=0)
    assert ct.n_vars - ct.l - 1 == 0 and key["l_query"][0].shape == (0, 8) and key["l_query"][1].shape == (0,), "l_query goes in as NULL"
    rng = random.Random(0x6C2)
    zs = M.witness_mix(ct, z, 3, seed=0x6C3)
    assert z in zs
    got, dlogs = prove_and_check(engine, ct, st, key, zs, [rng.randrange(R), EDGE_WORDS[6], 0], [EDGE_WORDS[3], rng.randrange(R), rng.randrange(R)])
    assert len(set(dlogs)) == 3


@pytest.mark.parametrize("log_n", [0, 1])
def test_no_constraint(engine, log_n):
    rng = random.Random(0x6D1 + log_n)
    for free_key in (False, True):
        ct, z, st, key = small_case((log_n, 0, 3, 1), 0x6D2 + log_n, free_key=free_key)
        rp, col, val = csr_arrays(ct.a)
        assert ct.n_cons == 0 and rp.tolist() == [0] and col.size == 0 and val.shape == (0, 4), "rows = nnz = 0: col and val go in as NULL"
        assert key["h_query"][0].shape[0] == (1 << log_n) - 1
        zs = [z, [1] + [rng.randrange(1 << 256) for _ in range(2)]]  # no constraint: every witness satisfies the circuit
        rs, ss = [rng.randrange(R), EDGE_WORDS[2]], [rng.randrange(R), rng.randrange(R)]
        got, dlogs = prove_and_check(engine, ct, st, key, zs, rs, ss, verifies=False)         # every IC_j is the identity: no verifying key to speak of
        if not free_key:                                             # u = v = 0: A = alpha + r delta, B = beta + s delta
            assert [d[:2] for d in dlogs] == [((st.alpha + r * st.delta) % R, (st.beta + s * st.delta) % R) for r, s in zip(rs, ss)]
            assert key["a_query"][1].all() and key["b_g2_query"][1].all(), "every query point is the identity"
        else:
            assert dlogs[0][0] != (st.alpha + rs[0] * st.delta) % R and len(set(dlogs)) == 2, "the sums over z count"


def test_a_short_circuit_on_a_small_domain(engine):
    ct, z, st, key = small_case((3, 5, 7, 2), 0x6E1)
    assert ct.n_cons == 5 and ct.n == 8
    rng = random.Random(0x6E2)
    zs = [z, [1] + [rng.randrange(1 << 256) for _ in range(6)]]      # the second is unsatisfied: h by the definition on the coset
    prove_and_check(engine, ct, st, key, zs, [rng.randrange(R), rng.randrange(R)], [rng.randrange(R), rng.randrange(R)])


# ---- (f) the G2 bucket route inside the prover ----------------------------------------------------------------------------------------------
def test_the_g2_bucket_route_inside_the_prover(engine):
    log_n, n_vars, l, m, limit, mc = ROUTE_LIMITS["f_one"]
    c = msm_model.g2_default_window(n_vars)
    assert msm_model.G2_DEFAULT_MIN <= n_vars < msm_model.DEFAULT_MIN and msm_model.g2_plan(n_vars, c) is not None, "by default the G2 sum is a bucket sum"
    assert msm_model.g2_plan(n_vars, c, limit) is None and mc == 1, "under the limit it has no plan, and one witness still fits"
    ct, z = M.make_circuit(log_n, 8, n_vars, l, seed=0x6F1, free=2)
    st = M.free_key(ct, seed=0x6F2)
    key = M.key_points(st, lambda d: engine.g1_generator_mul(words(d)), lambda d: engine.g2_generator_mul(words(d)))
    assert key["b_g2_query"][0].shape == (n_vars, 16) and key["l_query"][0].shape == (n_vars - l - 1, 8) and key["h_query"][0].shape == (7, 8)
    rng = random.Random(0x6F3)
    zs = [[1] + [rng.getrandbits(256) for _ in range(n_vars - 1)], M.zero_witness(ct)]
    rs, ss = [rng.randrange(R), rng.randrange(R)], [rng.randrange(R), rng.randrange(R)]
    want = M.proof_points(model_dlogs(st, zs, rs, ss))               # six points, the oracle's
    assert_same(prove(engine, ct, key, zs, rs, ss), want, "the bucket route")
    assert_same(prove_reversed_under(engine, limit_for("f_one", ct, m), ct, key, zs, rs, ss), want, "the composed route, a witness per chunk")


# ---- (g), (h), (i) the sparse product ------------------------------------------------------------------------------------------------------
def test_spmv_more_arrays_than_the_grid_has_rows_in_y(engine):
    m, rng = 65537, random.Random(0x671)
    row = [(0, rng.randrange(R)), (1, EDGE_WORDS[6])]
    vecs = [[rng.getrandbits(256), rng.getrandbits(256)] for _ in range(m)]
    for k, e in enumerate(EDGE_WORDS):
        vecs[k][k & 1], vecs[m - 1 - k][k & 1] = e, EDGE_WORDS[(k + 2) % 7]          # arrays 65530 .. 65536: on both sides of the grid's last row
    want = np.array([(row[0][1] * (a % R) + row[1][1] * (b % R)) % R for a, b in vecs], dtype=object)
    assert len(set(want.tolist())) == m, "no two arrays share a result"
    want = words(want.tolist()).reshape(m, 1, 4)
    csr, w = csr_arrays([row]), words([v for pair in vecs for v in pair]).reshape(m, 2, 4)
    got = engine.fr_spmv(csr, w)
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert bad.size == 0, f"default lanes: {bad.size} arrays differ, first {bad[:8].tolist()}"
    got = engine.fr_spmv(csr, w[::-1], lanes_log=6)                  # reversed: nothing an earlier call left behind is right
    bad = np.flatnonzero((got != want[::-1]).any(axis=(1, 2)))
    assert bad.size == 0, f"2^6 lanes: {bad.size} arrays differ, first {bad[:8].tolist()}"


def test_spmv_more_row_blocks_than_the_grid_has_in_x(engine):
    lg, n_out, n_cols, rng = 6, 4 * (1 << 20) + 5, 5, random.Random(0x681)
    assert -(-n_out // (256 >> lg)) == (1 << 20) + 2, "two row blocks past the grid of 2^20"
    live = {0: 3, (1 << 22) - 1: 2, 1 << 22: 5, (1 << 22) + 4: 1}    # row -> entries; every other row is empty
    mat = {i: [(rng.randrange(n_cols), rng.randrange(1, R)) for _ in range(ln)] for i, ln in live.items()}
    vec = [rng.randrange(1, R) for _ in range(n_cols)]
    dw = engine.to_device(np.ascontiguousarray(batch([vec]).transpose(0, 2, 1)))
    fill = np.full(4 * n_out + 64, SENTINEL, dtype=np.uint64)
    for rows in (n_out, (1 << 22) + 1):                              # every row a row of the matrix; then rows 2^22 + 1 .. n_out - 1 are the padding
        rp = np.zeros(rows + 1, dtype=np.uint64)
        inside = [i for i in sorted(mat) if i < rows]
        for i in inside:
            rp[i + 1:] += np.uint64(len(mat[i]))
        col = np.array([c for i in inside for c, _ in mat[i]], dtype=np.uint64)
        val = words([v for i in inside for _, v in mat[i]])
        drp, dcol, dval, dout = engine.to_device(rp), engine.to_device(col), engine.to_device_soa(val, 4), engine.to_device(fill)
        engine._call("sylow_hip_fr_spmv_batch_tuned", drp.ptr, dcol.ptr, dval.ptr, rows, len(col), dw.ptr, n_cols, 1, n_out, lg, dout.ptr)
        got = dout.download()
        assert (got[4 * n_out:] == SENTINEL).all(), "nothing beyond out is touched"
        got = got[:4 * n_out].reshape(4, n_out)
        assert np.flatnonzero(got.any(axis=0)).tolist() == inside, f"rows = {rows}: zero everywhere else, the sentinel nowhere"
        want = words([M.matvec([mat[i]], vec)[0] for i in inside])
        assert all(want.any(axis=1)) and np.array_equal(got[:, inside].T, want), f"rows = {rows}"


SPMV_L = (15, 16, 17, 27, 28, 29, 33)                                # entries per lane: the fold at 16, the 27 products that 512 bits hold


@pytest.mark.parametrize("lg", range(7))
def test_spmv_accumulator_at_its_bound(engine, lg):
    top = (R - 1) ** 2
    assert 27 * top < 1 << 512 <= 28 * top and top % R == 1, "28 unreduced products of (r - 1)^2 do not fit: a fold must come before"
    lanes = 1 << lg
    lens = [L * lanes for L in SPMV_L] + [300, 1025]
    mixed = 58 * lanes + 1                                           # a last row alternating (r - 1)(r - 1) and (r - 1) 1, 29 or 30 per lane
    rp = np.cumsum([0] + lens + [mixed]).astype(np.uint64)
    col = np.zeros(int(rp[-1]), dtype=np.uint64)
    col[int(rp[-2]) + 1::2] = 1
    vec = words([R - 1, 1])                                          # column 0: r - 1, column 1: 1
    want = words(lens + [(-(-mixed // 2) + (mixed // 2) * (R - 1)) % R])
    assert want[-1].tolist() == [1, 0, 0, 0]
    for v in (R - 1, 2 * R - 1):                                     # the same value as two words
        val = np.tile(words([v]), (len(col), 1))
        got = engine.fr_spmv((rp, col, val), vec, lanes_log=lg)
        assert np.array_equal(got, want), f"val {'2 r - 1' if v > R else 'r - 1'}: rows {np.flatnonzero((got != want).any(axis=1)).tolist()} of lengths {lens + [mixed]}"
    if lg == 3:                                                      # and the lanes the plan picks for this density
        assert np.array_equal(engine.fr_spmv((rp, col, val), vec), want)
