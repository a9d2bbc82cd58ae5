"""GPU: the Groth16 prover -- sylow_hip_fr_spmv_batch(_tuned), sylow_hip_groth16_quotient_batch and sylow_hip_groth16_prove_batch
(groth16_prove.hip) -- against the integer model of tests/groth16_prove_model.py.  Every comparison is exact, word for word: the sparse
product against sums of Python integers, the quotient against exact polynomial division (and, for an unsatisfied input, against the
definition on the coset), the proofs against the oracle's generator multiples of the model's discrete logarithms and through the library's
own verifier.  Circuits, keys and references are made once per shape."""
import functools
import random

import numpy as np
import pytest

import groth16_model as G
import groth16_prove_model as M
from groth16_prove_model import EDGE_WORDS, R

pytestmark = pytest.mark.gpu
E_ARG = -2
SENTINEL = 0x5A5A5A5A5A5A5A5A
LANES = range(7)                                                    # every lanes-per-row pin: 2^0 .. 2^6


def words(a):
    return G.limbs(list(a))


def batch(arrays):
    """m lists of n ints -> [m, n, 4] words"""
    return np.stack([words(a) for a in arrays])


def csr_arrays(rows):
    rp, col, val = M.csr(rows)
    return np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint64), (words(val) if val else np.zeros((0, 4), dtype=np.uint64))


# ---- spmv --------------------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 15, 16, 17, 33, 300]                            # the accumulation boundary, and rows longer than any lane group
N_COLS = 41


@functools.lru_cache(maxsize=None)
def spmv_case(rows):
    """a matrix of `rows` rows whose lengths walk ROW_LENGTHS, columns 0 and n_cols - 1 and the edge words among the entries, three vectors
    with the edge words in them: (rows as lists, vectors as lists)"""
    rng = random.Random(0x5B37 + rows)
    mat = []
    for i in range(rows):
        ln = ROW_LENGTHS[(i + 3) % len(ROW_LENGTHS)]                  # one row: 16 entries
        row = [(rng.randrange(N_COLS), rng.randrange(R)) for _ in range(ln)]
        for k, (c, v) in enumerate(row[:2 * len(EDGE_WORDS)]):
            row[k] = ((0, N_COLS - 1)[k & 1] if k < 4 else c, EDGE_WORDS[(k + i) % len(EDGE_WORDS)])
        mat.append(row)
    vecs = []
    for j in range(3):
        w = [rng.randrange(1 << 256) for _ in range(N_COLS)]
        for k, e in enumerate(EDGE_WORDS):
            w[(5 * k + j) % N_COLS] = e
        w[0], w[N_COLS - 1] = EDGE_WORDS[(j + 2) % 7], EDGE_WORDS[(j + 6) % 7]
        vecs.append(w)
    return mat, vecs


@pytest.mark.parametrize("rows", [1, 7, 255, 256, 257])
def test_spmv_rows_lengths_and_every_lane_pin(engine, rows):
    mat, vecs = spmv_case(rows)
    csr = csr_arrays(mat)
    want = batch([M.matvec(mat, w) for w in vecs])
    got = engine.fr_spmv(csr, batch(vecs))
    assert np.array_equal(got, want), f"{int((got != want).any(axis=2).sum())} of {3 * rows} values differ at the default lanes"
    for lg in LANES:
        assert np.array_equal(engine.fr_spmv(csr, batch(vecs), lanes_log=lg), want), f"2^{lg} lanes per row"
    one = engine.fr_spmv(csr, words(vecs[1]))                        # m = 1
    assert np.array_equal(one, want[1])


@pytest.mark.parametrize("lg", [-1, 0, 3, 6])
def test_spmv_padding_sentinels_and_empty_matrix(engine, lg):
    rows, n_out, m = 7, 12, 3
    mat, vecs = spmv_case(rows)
    rp, col, val = csr_arrays(mat)
    drp, dcol, dval = engine.to_device(rp), engine.to_device(col), engine.to_device_soa(val, 4)
    dw = engine.to_device(np.ascontiguousarray(batch(vecs).transpose(0, 2, 1)))
    fill = np.full(m * 4 * n_out + 64, SENTINEL, dtype=np.uint64)
    dout = engine.to_device(fill)
    engine._call("sylow_hip_fr_spmv_batch_tuned", drp.ptr, dcol.ptr, dval.ptr, rows, len(col), dw.ptr, N_COLS, m, n_out, lg, dout.ptr)
    got = dout.download()
    assert (got[m * 4 * n_out:] == SENTINEL).all(), "nothing beyond out is touched"
    got = got[:m * 4 * n_out].reshape(m, 4, n_out).transpose(0, 2, 1)
    assert np.array_equal(got[:, :rows], batch([M.matvec(mat, w) for w in vecs])) and not got[:, rows:].any(), "the padding rows are zero"
    # nnz = 0: every row is empty, NULL col and val
    dout, dzero = engine.to_device(fill), engine.to_device(np.zeros(rows + 1, dtype=np.uint64))
    engine._call("sylow_hip_fr_spmv_batch_tuned", dzero.ptr, None, None, rows, 0, dw.ptr, N_COLS, m, n_out, lg, dout.ptr)
    got = dout.download()
    assert not got[:m * 4 * n_out].any() and (got[m * 4 * n_out:] == SENTINEL).all()


def test_spmv_columns_past_the_vector_and_row_ends_past_nnz_contribute_nothing(engine):
    rng = random.Random(0x5B38)
    mat = [[(rng.randrange(N_COLS), rng.randrange(R)) for _ in range(ln)] for ln in (3, 20, 1, 40)]
    mat[0][1] = (N_COLS, 5)                                          # col = n_cols
    mat[1][17] = (1 << 63, 7)                                        # col = 2^63
    mat[3][0] = ((1 << 64) - 1, 9)
    vec = [rng.randrange(R) for _ in range(N_COLS)]
    want = words(M.matvec(mat, vec))
    for lg in (-1, 0, 2, 6):
        assert np.array_equal(engine.fr_spmv(csr_arrays(mat), words(vec), lanes_log=lg), want), lg
    # a malformed row_ptr: ends past nnz are clamped, an end before its start is an empty row -- a wrong number, never a fault
    rp, col, val = csr_arrays(mat)
    bad = rp.copy()
    bad[2], bad[4] = 10 ** 12, (1 << 64) - 1                         # row 1 runs to nnz; row 2 starts past nnz and is empty; row 3 runs to nnz
    flat = [e for row in mat for e in row]
    clamped = [flat[int(rp[0]):int(rp[1])], flat[int(rp[1]):], [], flat[int(rp[3]):]]
    for lg in (0, 6):
        assert np.array_equal(engine.fr_spmv((bad, col, val), words(vec), lanes_log=lg), words(M.matvec(clamped, vec))), lg


def test_spmv_argument_errors(engine):
    lib = engine.lib
    mat, vecs = spmv_case(7)
    rp, col, val = csr_arrays(mat)
    drp, dcol, dval = engine.to_device(rp), engine.to_device(col), engine.to_device_soa(val, 4)
    dw = engine.to_device(np.ascontiguousarray(batch(vecs).transpose(0, 2, 1)))
    fill = np.full((3, 4, 8), SENTINEL, dtype=np.uint64)
    dout = engine.to_device(fill)
    plain = lambda *a: lib.sylow_hip_fr_spmv_batch(*a, engine.stream)
    tuned = lambda *a: lib.sylow_hip_fr_spmv_batch_tuned(*a, engine.stream)
    assert plain(drp.ptr, dcol.ptr, dval.ptr, 7, len(col), dw.ptr, N_COLS, 3, 6, dout.ptr) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()   # n_out < rows
    assert plain(drp.ptr, dcol.ptr, dval.ptr, 7, len(col), dw.ptr, N_COLS, 1 << 62, 8, dout.ptr) == E_ARG                                             # a size overflow
    assert plain(drp.ptr, dcol.ptr, dval.ptr, 7, len(col), dw.ptr, 1 << 61, 3, 8, dout.ptr) == E_ARG
    assert plain(None, dcol.ptr, dval.ptr, 7, len(col), dw.ptr, N_COLS, 3, 8, dout.ptr) == E_ARG and plain(drp.ptr, dcol.ptr, dval.ptr, 7, len(col), dw.ptr, N_COLS, 3, 8, None) == E_ARG
    assert tuned(drp.ptr, dcol.ptr, dval.ptr, 7, len(col), dw.ptr, N_COLS, 3, 8, 7, dout.ptr) == E_ARG
    assert plain(drp.ptr, dcol.ptr, dval.ptr, 7, len(col), dw.ptr, N_COLS, 0, 8, dout.ptr) == 0 and plain(None, None, None, 0, 0, None, 0, 3, 0, None) == 0   # no-ops
    engine.sync()
    assert np.array_equal(dout.download(), fill), "nothing written"


# ---- the quotient ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quotient_case(log_n, seed=0):
    """(a, b, c) with c = a b mod r and the edge words in a and b, and the exact quotient"""
    rng = random.Random(0x9107 + 64 * seed + log_n)
    n = 1 << log_n
    a, b = [rng.randrange(1 << 256) for _ in range(n)], [rng.randrange(1 << 256) for _ in range(n)]
    for k, e in enumerate(EDGE_WORDS):
        a[k % n], b[(n - 1 - k) % n] = e, EDGE_WORDS[(k + 3) % len(EDGE_WORDS)]
    c = [x * y % R for x, y in zip(a, b)]
    h, rem = M.quotient_exact(a, b, c, log_n)
    assert not any(rem) and h[n - 1] == 0
    return a, b, c, h


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 5, 6, 7, 11])     # 11: more than one tile, three passes at the default
def test_quotient_is_exact_division(engine, log_n):
    cases = [quotient_case(log_n, s) for s in range(3)]
    got = engine.groth16_quotient(batch([c[0] for c in cases]), batch([c[1] for c in cases]), batch([c[2] for c in cases]))        # m = 3
    for j, c in enumerate(cases):
        assert np.array_equal(got[j], words(c[3])), f"log_n {log_n} array {j}: {int((got[j] != words(c[3])).any(axis=1).sum())} of {1 << log_n} coefficients differ"
        assert not got[j][-1].any(), "h[n - 1] = 0 is written"
    a, b, c, h = cases[1]
    one = engine.groth16_quotient(batch([a]), batch([b]), batch([c]))                                                              # m = 1
    assert np.array_equal(one[0], words(h))


@pytest.mark.parametrize("log_n", [0, 3, 6])
def test_quotient_of_an_unsatisfied_input_is_the_definition(engine, log_n):
    rng = random.Random(0x9108 + log_n)
    n = 1 << log_n
    a, b, c = ([rng.randrange(1 << 256) for _ in range(n)] for _ in range(3))
    want = M.quotient_coset(a, b, c, log_n)
    assert any(M.quotient_exact(a, b, c, log_n)[1])
    sat = quotient_case(log_n)
    got = engine.groth16_quotient(batch([a, sat[0]]), batch([b, sat[1]]), batch([c, sat[2]]))
    assert np.array_equal(got[0], words(want)) and np.array_equal(got[1], words(sat[3]))


def test_quotient_argument_errors_and_empty_batch(engine):
    lib = engine.lib
    fill = np.full((1, 4, 8), SENTINEL, dtype=np.uint64)
    da, dh = engine.to_device(fill), engine.to_device(fill)
    call = lambda *a: lib.sylow_hip_groth16_quotient_batch(*a, engine.stream)
    assert call(da.ptr, da.ptr, da.ptr, -1, 1, dh.ptr) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    assert call(da.ptr, da.ptr, da.ptr, 29, 1, dh.ptr) == E_ARG
    assert call(None, da.ptr, da.ptr, 3, 1, dh.ptr) == E_ARG and call(da.ptr, da.ptr, da.ptr, 3, 1, None) == E_ARG
    assert call(da.ptr, da.ptr, da.ptr, 3, 0, dh.ptr) == 0 and call(None, None, None, 3, 0, None) == 0
    engine.sync()
    assert np.array_equal(dh.download(), fill), "nothing written"


# ---- the proof ---------------------------------------------------------------------------------------------------------------------------
# (log_n, n_cons, n_vars, l, free variables): the largest has two constraints fewer than its domain has points
CIRCUITS = {"n1": (0, 1, 3, 1, 1), "n8": (3, 8, 7, 2, 2), "n64": (6, 64, 50, 3, 2), "n2048": (11, 2046, 1500, 4, 2)}
SINGLES = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")
_KEYS = {}


def circuit(engine, name):
    """(circuit, witness, setup, key arrays, vk arrays), made once per shape.  The oracle makes every point but the queries of the largest
    circuit (6500 points at 4 ms each): those come from the library's fixed-base generator products, which tests/test_gpu_groups.py pins to
    the oracle; the expected PROOFS are the oracle's on every shape."""
    if name not in _KEYS:
        log_n, n_cons, n_vars, l, free = CIRCUITS[name]
        ct, z = M.make_circuit(log_n, n_cons, n_vars, l, seed=0x616 + log_n, free=free)
        st = M.Setup(ct, seed=0x617 + log_n)
        big = n_vars > 1000
        key = M.key_points(st, (lambda d: engine.g1_generator_mul(words(d))) if big else None, (lambda d: engine.g2_generator_mul(words(d))) if big else None)
        _KEYS[name] = (ct, z, st, key, M.vk_points(st))
    return _KEYS[name]


def prove(engine, ct, key, zs, rs, ss):
    mats = [csr_arrays(m) for m in (ct.a, ct.b, ct.c)]
    pk = {k: (v[0] if k in SINGLES else v) for k, v in key.items()}
    return engine.groth16_prove(mats, ct.n_vars, ct.l, ct.log_n, pk, batch(zs), words(rs), words(ss))


def check_proofs(got, st, zs, rs, ss):
    (a, ai), (b, bi), (c, ci) = got
    (wa, wai), (wb, wbi), (wc, wci) = M.proof_points([st.proof_dlogs(z, r, s) for z, r, s in zip(zs, rs, ss)])
    for what, x, y in (("A", a, wa), ("B", b, wb), ("C", c, wc), ("A flags", ai, wai), ("B flags", bi, wbi), ("C flags", ci, wci)):
        assert np.array_equal(np.asarray(x), np.asarray(y)), what


def verify(engine, vk, got, zs, l):
    (a, ai), (b, bi), (c, ci) = got
    inputs = np.stack([words([v for v in z[1:l + 1]]) for z in zs]).reshape(len(zs), l, 4)
    return engine.groth16_verify(vk, a, b, c, inputs, ai, bi, ci).astype(bool)


@pytest.mark.parametrize("name", list(CIRCUITS))
def test_proofs_match_the_model_and_verify(engine, name):
    ct, z, st, key, vk = circuit(engine, name)
    rng = random.Random(0x618)
    free = CIRCUITS[name][4]
    z2 = z[:-free] + [rng.randrange(1 << 256), EDGE_WORDS[6]][:free]   # a second witness: the free variables take any words
    assert ct.satisfied([v % R for v in z2])
    zs, rs, ss = [z, z2], [rng.randrange(R), EDGE_WORDS[4]], [rng.randrange(R), EDGE_WORDS[5]]
    got = prove(engine, ct, key, zs, rs, ss)                         # two witnesses per call
    check_proofs(got, st, zs, rs, ss)
    assert verify(engine, vk, got, zs, ct.l).all(), "the library's own verifier accepts both proofs"
    wrong = [[z[0], z[1] + 1] + z[2:], z2]                           # a valid proof checked against inputs + 1
    assert list(verify(engine, vk, got, wrong, ct.l)) == [False, True]


@pytest.mark.parametrize("name", ["n1", "n8", "n64"])
def test_randomness_at_zero_and_at_the_edge_words_and_the_zero_witness(engine, name):
    ct, z, st, key, vk = circuit(engine, name)
    z0 = [1] + [0] * (ct.n_vars - 1)                                 # zero but for z_0: every sum is empty
    rs, ss = [0] + EDGE_WORDS, [0] + EDGE_WORDS[::-1]
    zs = [z0 if k % 3 == 2 else z for k in range(len(rs))]
    got = prove(engine, ct, key, zs, rs, ss)
    check_proofs(got, st, zs, rs, ss)
    assert verify(engine, vk, got, zs, ct.l).all()


def test_an_unsatisfied_witness_gives_a_proof_the_verifier_rejects(engine):
    ct, z, st, key, vk = circuit(engine, "n8")
    bad = list(z)
    bad[ct.l + 1] = (bad[ct.l + 1] + 1) % R
    assert not ct.satisfied(bad)
    zs, rs, ss = [bad, z], [11, 12], [13, 14]
    got = prove(engine, ct, key, zs, rs, ss)
    check_proofs(got, st, zs, rs, ss)                                # still the formulas' points, with h by the definition on the coset
    assert list(verify(engine, vk, got, zs, ct.l)) == [False, True]


def test_identity_flagged_entries_in_every_query(engine):
    """a flagged entry adds nothing whatever its words hold: the key keeps the true points and flags one more entry per query"""
    ct, z, st, _, _ = circuit(engine, "n8")
    st2 = M.Setup(ct, seed=0x617 + ct.log_n)
    st2.flagged = {"a_query": {2}, "b_g1_query": {0, 3}, "b_g2_query": {0, 3}, "h_query": {1, ct.n - 2}, "l_query": {0}}
    key = M.key_points(st2)
    for q in ("a_query", "b_g1_query", "b_g2_query", "l_query"):     # the free variables' entries are identities of their own
        assert key[q][1][-1] == 1
    zs, rs, ss = [z, z], [21, 0], [0, 22]
    check_proofs(prove(engine, ct, key, zs, rs, ss), st2, zs, rs, ss)


def test_chunks_under_a_scratch_limit_and_a_limit_too_small(engine):
    ct, z, st, key, vk = circuit(engine, "n64")
    rng = random.Random(0x619)
    zs, rs, ss = [z] * 5, [rng.randrange(R) for _ in range(5)], [rng.randrange(R) for _ in range(5)]
    want = prove(engine, ct, key, zs, rs, ss)
    try:
        engine.set_scratch_limit(60000)                              # (6, 50, 3): two witnesses cost 52 856 bytes, three 78 744 -- chunks of 2, 2, 1
        got = prove(engine, ct, key, zs, rs, ss)
        engine.set_scratch_limit(1000)
        with pytest.raises(Exception, match="scratch limit"):
            prove(engine, ct, key, zs, rs, ss)
    finally:
        engine.set_scratch_limit(0)
    for x, y in zip(got, want):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    check_proofs(got, st, zs, rs, ss)


def test_prove_argument_errors_and_empty_batch(engine):
    ct, z, st, key, vk = circuit(engine, "n8")
    lib = engine.lib
    mats = [csr_arrays(m) for m in (ct.a, ct.b, ct.c)]
    up = [engine._csr_up(x) for x in mats]
    csr_args = [v for u in up for v in (u[0].ptr, u[1].ptr, u[2].ptr, u[4])]
    single = [engine.to_device_soa(key[k][0], w) for k, w in (("alpha_g1", 8), ("beta_g1", 8), ("delta_g1", 8), ("beta_g2", 16), ("delta_g2", 16))]
    held = []
    for k, w in (("a_query", 8), ("b_g1_query", 8), ("b_g2_query", 16), ("h_query", 8), ("l_query", 8)):
        held += [engine.to_device_soa(key[k][0], w), engine.to_device(np.asarray(key[k][1], dtype=np.uint8))]
    dz = engine.to_device(np.ascontiguousarray(batch([z]).transpose(0, 2, 1)))
    dr, ds = engine.to_device_soa(words([1]), 4), engine.to_device_soa(words([2]), 4)
    fill8, fill16, fillf = np.full((8, 1), SENTINEL, dtype=np.uint64), np.full((16, 1), SENTINEL, dtype=np.uint64), np.full(8, 0x5A, dtype=np.uint8)
    outs = [engine.to_device(x) for x in (fill8, fillf, fill16, fillf, fill8, fillf)]

    def call(n_cons, n_vars, l, log_n, m):
        return lib.sylow_hip_groth16_prove_batch(*csr_args, n_cons, n_vars, l, log_n, *[d.ptr for d in single], *[d.ptr for d in held], dz.ptr, dr.ptr, ds.ptr, m,
                                                 *[d.ptr for d in outs], engine.stream)
    assert call(ct.n_cons, ct.n_vars, ct.l, -1, 1) == E_ARG and b"bad argument" in lib.sylow_hip_last_error()
    assert call(ct.n_cons, ct.n_vars, ct.l, 29, 1) == E_ARG
    assert call(ct.n_cons, ct.n_vars, ct.l, 2, 1) == E_ARG           # n_cons = 8 > 2^2
    assert call(ct.n_cons, ct.n_vars, ct.n_vars, ct.log_n, 1) == E_ARG and call(ct.n_cons, ct.n_vars, ct.n_vars + 1, ct.log_n, 1) == E_ARG    # l >= n_vars
    assert call(ct.n_cons, ct.n_vars, ct.l, ct.log_n, 0) == 0        # m = 0: OK, nothing launched
    engine.sync()
    for d, f in zip(outs, (fill8, fillf, fill16, fillf, fill8, fillf)):
        assert np.array_equal(d.download(), f), "nothing written"
    assert call(ct.n_cons, ct.n_vars, ct.l, ct.log_n, 1) == 0        # and the same arguments with m = 1 prove
    engine.sync()
    a = np.ascontiguousarray(outs[0].download().T)
    assert np.array_equal(a, M.proof_points([st.proof_dlogs(z, 1, 2)])[0][0])


def test_api_round_trip(engine):
    from sylow_amd import api
    api.set_engine(engine)
    ct, z, st, key, vk = circuit(engine, "n8")
    g1 = lambda k: api.G1Affine(*key[k])
    pk = api.Groth16ProvingKey(g1("alpha_g1"), g1("beta_g1"), g1("delta_g1"), api.G2Affine(*key["beta_g2"]), api.G2Affine(*key["delta_g2"]), g1("a_query"),
                               g1("b_g1_query"), api.G2Affine(*key["b_g2_query"]), g1("h_query"), g1("l_query"))
    circ = api.Groth16Circuit(M.csr(ct.a), M.csr(ct.b), M.csr(ct.c), ct.n_vars, ct.l, ct.log_n)
    a, b, c = api.groth16_prove(pk, circ, [z, z], [5, 6], [7, 8])
    check_proofs(((a.xy, a.infinity), (b.xy, b.infinity), (c.xy, c.infinity)), st, [z, z], [5, 6], [7, 8])
    vkey = api.Groth16VerifyingKey(api.G1Affine(vk[0]), api.G2Affine(vk[1]), api.G2Affine(vk[2]), api.G2Affine(vk[3]), api.G1Affine(vk[4]))
    assert api.groth16_verify(vkey, a, b, c, [z[1:ct.l + 1]] * 2).all()
    with pytest.raises(ValueError):
        api.Groth16Circuit(M.csr(ct.a), M.csr(ct.b), M.csr(ct.c), ct.n_vars, ct.n_vars, ct.log_n)
