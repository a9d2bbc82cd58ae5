"""The input contract (tests/test_gpu_input_contract.py) for the entry points that hash under a caller-chosen expander.  That file keeps
one CONTRACT row per declared entry point and a GPU case per non-exempt row; this one registers the rows and cases of the six expander
entry points in its tables when the suite is collected, so its CPU completeness tests see them, and runs the two verifiers through the same
check (check_row: every Fp argument as representatives x + k p, NULL flags against all-zero flags) at one batch size per route."""
import numpy as np
import pytest

import test_gpu_input_contract as T
from test_gpu_input_contract import coeffs, pool, pool_all, verify_sizes  # noqa: F401  (fixtures)

MESSAGES = "message bytes and a tag: no field input (test_gpu_expanders.py)"
ROWS = {
    "sylow_hip_expand_message_batch": T.ex(MESSAGES),
    "sylow_hip_hash_to_field_expander_batch": T.ex(MESSAGES),
    "sylow_hip_hash_to_g1_expander_batch": T.ex(MESSAGES),
    "sylow_hip_bls_sign_expander_batch": T.ex(T.SCALAR),
    "sylow_hip_bls_verify_expander_batch": T.Row({"pk_xy": T.G2A, "sig_xy": T.G1A}, ["pk_inf", "sig_inf"]),
    "sylow_hip_bls_verify_hashed_batch": T.Row({"pk_xy": T.G2A, "h_xy": T.G1A, "sig_xy": T.G1A}, ["pk_inf", "h_inf", "sig_inf"]),
}
T.CONTRACT.update(ROWS)


@T.case("bls_verify_expander_batch")
def _verify_expander(eng, c, pool, nm):
    pk, sig, msgs, ki, si = T._verify_inputs(pool, T.ROUTE["n"])      # the pool's signatures are under the library suite: expander 0, NULL tag
    return [eng.bls_verify(c.fp("pk_xy", pk), msgs, c.fp("sig_xy", sig), pk_inf=c.flag("pk_inf", ki), sig_inf=c.flag("sig_inf", si), expander=0)]


@T.case("bls_verify_hashed_batch")
def _verify_hashed(eng, c, pool, nm):
    n = T.ROUTE["n"]
    pk, sig, msgs, ki, si = T._verify_inputs(pool, n)
    key = pool.setdefault("hashed", {})
    if n not in key:
        key[n] = eng.hash_to_g1(msgs)[0]
    return [eng.bls_verify_hashed(c.fp("pk_xy", pk), c.fp("h_xy", key[n]), c.fp("sig_xy", sig), pk_inf=c.flag("pk_inf", ki),
                                  h_inf=c.flag("h_inf", T._flags(n, 2, 29)), sig_inf=c.flag("sig_inf", si))]


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
        assert {p for p, sh in shapes[name][1].items() if sh.optional and sh.dtype == "u8" and p.endswith("_inf")} == set(row.flags), name
        assert name in T.CASES


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["one", "two_per_wave", "quad", "round_tail"])
@pytest.mark.parametrize("name", sorted(n for n, r in ROWS.items() if not r.exempt))
def test_expander_verifier_reduces_representatives(engine, pool_all, verify_sizes, name, route):
    n = T.ROUTE["n"] = verify_sizes[route]
    try:
        base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, pool_all))
    finally:
        T.ROUTE["n"] = 64
    ok = np.asarray(base[0])
    assert ok.any() and (n < 7 or not ok.all()), f"{name}: the batch should hold valid and invalid signatures"
