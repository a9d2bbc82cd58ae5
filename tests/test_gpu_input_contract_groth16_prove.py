"""The input contract (tests/test_gpu_input_contract.py) for the Groth16 prover's entry points.  sylow_hip_fr_spmv_batch(_tuned) and
sylow_hip_groth16_quotient_batch have only Fr-valued arguments and are exempt (their edge words: tests/test_gpu_groth16_prove.py).
sylow_hip_groth16_prove_batch takes the proving key's coordinate words -- five single points and five queries, each query with an optional
flag array -- so its row runs through the same check (check_row: every key array as representatives x + k p; NULL flags against all-zero
flags), on the circuit of 8 constraints with four proofs.  The rows and the case are registered in that file's tables when the suite is
collected, so its CPU completeness tests see them.  Beside it: words >= r in z, r, s and the matrices' values give the proofs of their
residues."""
import random

import numpy as np
import pytest

import groth16_prove_model as M
import test_gpu_input_contract as T
from groth16_model import limbs

FR_ONLY = "Fr-valued arguments: tested with their own edge values (test_gpu_groth16_prove.py)"
QUERIES = {"a_query": T.G1A, "b_g1_query": T.G1A, "b_g2_query": T.G2A, "h_query": T.G1A, "l_query": T.G1A}
ROWS = {
    "sylow_hip_fr_spmv_batch": T.ex(FR_ONLY),
    "sylow_hip_fr_spmv_batch_tuned": T.ex(FR_ONLY),
    "sylow_hip_groth16_quotient_batch": T.ex(FR_ONLY),
    "sylow_hip_groth16_prove_batch": T.Row({"alpha_g1": T.G1A, "beta_g1": T.G1A, "delta_g1": T.G1A, "beta_g2": T.G2A, "delta_g2": T.G2A, **QUERIES},
                                           [q + "_inf" for q in QUERIES]),
}
T.CONTRACT.update(ROWS)
N_PROOFS = 4
_DATA = []


def data():
    """a satisfied circuit of 8 constraints over 7 variables, its key and the randomness of four proofs.  The queries hold identities (A has
    no entry in column 0, one variable is in no row): with NULL or all-zero flags those entries enter as the words they hold, the same in
    both calls, which is all check_row compares there"""
    if not _DATA:
        ct, z = M.make_circuit(3, 8, 7, 2, seed=0xC0, free=1)
        st = M.Setup(ct, seed=0xC1)
        key = M.key_points(st)
        assert all(np.asarray(key[q][1]).any() for q in ("a_query", "b_g1_query", "b_g2_query", "l_query"))
        rng = random.Random(0xC2)
        _DATA.append((ct, z, st, key, [rng.randrange(M.R) for _ in range(N_PROOFS)], [rng.randrange(M.R) for _ in range(N_PROOFS)]))
    return _DATA[0]


def mats(ct, lift=0):
    """the three CSR matrices; lift: added to every value (a multiple of r leaves the residues alone)"""
    out = []
    for rows in (ct.a, ct.b, ct.c):
        rp, col, val = M.csr(rows)
        out.append((np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint64), limbs([v + lift for v in val])))
    return out


def run(eng, ct, pk, zs, rs, ss, lift=0):
    (a, ai), (b, bi), (c, ci) = eng.groth16_prove(mats(ct, lift), ct.n_vars, ct.l, ct.log_n, pk, np.stack([limbs(z) for z in zs]), limbs(rs), limbs(ss))
    return [a, ai, b, bi, c, ci]


@T.case("groth16_prove_batch")
def _prove(eng, c, pool, nm):
    ct, z, st, key, rs, ss = data()
    pk = {k: c.fp(k, key[k][0]) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")}
    pk.update({q: (c.fp(q, key[q][0]), c.flag(q + "_inf", np.asarray(key[q][1], dtype=np.uint8))) for q in QUERIES})
    return run(eng, ct, pk, [z] * N_PROOFS, rs, ss)


def test_rows_name_real_parameters():
    from sylow_amd import _shapes
    from test_rust_ffi import parse_header
    protos, shapes = parse_header(), _shapes.parse()
    for name, row in ROWS.items():
        assert name in protos and T.CONTRACT[name] is row
        if row.exempt:
            assert name not in T.CASES
            continue
        assert set(row.fp) | set(row.flags) <= {p[3] for p in protos[name][1]}, name
        assert {p for p, sh in shapes[name][1].items() if sh.optional and sh.dtype == "u8"} == set(row.flags), name
        assert name in T.CASES


@pytest.mark.gpu
def test_groth16_prove_reduces_representatives_and_accepts_null_flags(engine):
    name = "sylow_hip_groth16_prove_batch"
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    ct, z, st, key, rs, ss = data()
    (wa, _), (wb, _), (wc, _) = M.proof_points([st.proof_dlogs(z, r, s) for r, s in zip(rs, ss)])
    assert np.array_equal(base[0], wa) and np.array_equal(base[2], wb) and np.array_equal(base[4], wc), "the canonical call is the model's proofs"
    assert not any(np.asarray(base[k]).any() for k in (1, 3, 5))


@pytest.mark.gpu
def test_words_at_or_above_r_give_the_proofs_of_their_residues(engine):
    ct, z, st, key, rs, ss = data()
    pk = {k: (v[0] if k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2") else v) for k, v in key.items()}
    R, top = M.R, 1 << 256
    lift = lambda v, k: v + ((top - 1 - v) // R if k is None else k) * R       # the largest representative, or v + k r
    base = run(engine, ct, pk, [z] * N_PROOFS, rs, ss)
    zs = [[lift(v, (1, 2, None, 4)[j] if (i + j) % 2 == 0 else 0) for i, v in enumerate(z)] for j in range(N_PROOFS)]      # v + 4 r < 5 r < 2^256
    assert all(max(w) >= R and max(w) < top for w in zs)
    cases = {"z": (zs, rs, ss, 0), "r": ([z] * N_PROOFS, [lift(v, (1, None, 3, 4)[j]) for j, v in enumerate(rs)], ss, 0),
             "s": ([z] * N_PROOFS, rs, [lift(v, (None, 1, 2, 4)[j]) for j, v in enumerate(ss)], 0), "val": ([z] * N_PROOFS, rs, ss, R),
             "all": (zs, [lift(v, None) for v in rs], [lift(v, 1) for v in ss], 2 * R)}
    for what, (w, r, s, lf) in cases.items():
        got = run(engine, ct, pk, w, r, s, lf)
        for k, (x, y) in enumerate(zip(got, base)):
            assert np.array_equal(x, y), f"{what} as words >= r: output {k} differs"
