"""CPU half of the memory contract (tests/test_gpu_memory_contract.py runs it on the GPU through tests/guarded_engine.py).

MEMORY_CONTRACT has one row per entry point include/sylow_hip.h declares: the GPU tests that drive it between guard bands, or the reason
it is exempt.  The tests here fail when an entry point has no row, when a row names a test that does not drive it, when the exempt set is
not exactly the one written down, when an exempt row has a device output array, and when a pointer parameter of an annotated prototype
is missing from the parser's const / output table or its qualifier contradicts its name (an `out*`, `status`, `ok` or `is_one` array
declared const, an optional `*_inf` input not const) -- so a new entry point cannot skip the contract."""
import numpy as np
import pytest

from guarded_engine import GUARD, audit_bytes, constness


class Row:
    def __init__(self, tests=(), exempt=None):
        self.tests, self.exempt = tuple(tests), exempt


HOST_ONLY = "host-only runtime call: no device array"
MEMORY = "malloc / free / memcpy: the primitives the guarded buffers are made of"
B, PAIRING, VERIFY, WIDE, GROUPS, FIELDS, STATUS, JOBS, NTT = (
    "test_input_contract_driver_stays_inside_its_buffers", "test_ragged_pairing", "test_ragged_bls_verify", "test_ragged_wide_and_one_lane",
    "test_ragged_group_ops", "test_ragged_fields", "test_ragged_status_only_outputs", "test_ragged_jobs", "test_ragged_fr_ntt")
HOST = {"pairing_host": "test_pairing_host_stays_inside_host_arrays", "bls_verify_host": "test_bls_verify_host_stays_inside_host_arrays",
        "pairing_host_bytes": "test_pairing_host_bytes_stays_inside_host_arrays",
        "bls_verify_host_bytes": "test_bls_verify_host_bytes_stays_inside_host_arrays", "host_xoshiro_fp": "test_host_xoshiro_fp_stays_inside_its_array"}


def _rows(tests, names):
    return {s: Row(tests) for s in names.split()}


MEMORY_CONTRACT = {
    **{s: Row(exempt=HOST_ONLY) for s in ["init", "init_devices", "set_device", "shutdown", "trim", "set_scratch_limit", "set_option", "get_option",
                                          "wall_clock_khz", "last_error", "device_count", "stream_sync", "host_malloc", "host_free",
                                          "g2_line_table_words"]},
    **{s: Row(exempt=MEMORY) for s in ["malloc", "free", "memcpy_h2d", "memcpy_d2h"]},
    "clock_probe": Row(exempt="acc is an accumulator by contract: the kernels of later calls add to it, nothing is written by the call itself"),
    **_rows([B], """bls_aggregate_partial_batch bls_aggregate_verify_batch bls_batch_verify_weighted bls_verify_expander_batch
            bls_verify_hashed_batch bls_weighted_partial_batch fp12_cyclotomic_sqr_batch fp12_frobenius_batch fp12_inv_batch
            fp12_product_final_exp fp12_sparse_mul_batch fp12_sqr_batch fp2_frobenius_batch fp2_residue_mul_batch fp2_sqr_batch
            fp6_frobenius_batch fp6_inv_batch fp6_residue_mul_batch fp6_sqr_batch g1_ct_eq_batch g1_ntt_batch g1_ntt_batch_tuned
            g1_on_curve_batch g1_projective_new_batch g1_to_be_bytes_batch g2_ct_eq_batch g2_double_batch g2_lincomb_batch g2_line_table
            g2_msm g2_msm_tuned g2_precompute_batch g2_projective_new_batch g2_psi_batch g2_sub_batch g2_to_be_bytes_batch
            glued_miller_loop_batch glued_miller_loop_precomputed_batch groth16_batch_verify_weighted groth16_prove_batch
            groth16_vk_x_batch gt_pow_batch kzg_batch_verify_weighted kzg_combine_openings_batch kzg_commit_batch kzg_commit_batch_tuned
            kzg_commit_evals_batch kzg_fold_batch kzg_open_all_batch kzg_open_all_batch_tuned kzg_open_all_prepare kzg_open_batch
            kzg_open_evals_batch kzg_open_multi_batch kzg_open_multi_evals_batch kzg_srs_lagrange kzg_verify_line_table_batch
            kzg_verify_multi_batch miller_loop_precomputed_batch pairing_product_all pairing_product_batch pairing_product_partial_batch
            svdw_map_batch"""),
    **_rows([B, FIELDS], """fext_add_batch fext_neg_batch fext_scale_batch fext_sub_batch fp12_mul_batch fp2_inv_batch fp2_mul_batch fp6_mul_batch
            fp_add_batch fp_inv_batch fp_is_square_batch fp_mul_batch fp_neg_batch fp_pow_batch fp_sqr_batch fp_sqrt_batch fp_sub_batch
            fp_to_be_bytes_batch"""),
    **_rows([B, GROUPS], """g1_add_batch g1_double_batch g1_normalize_batch g1_sub_batch g1_sum_batch g2_add_batch g2_normalize_batch
            g2_scalar_mul_batch g2_scalar_mul_subgroup_batch g2_subgroup_check_batch g2_sum_batch"""),
    **_rows([B, JOBS], "g1_lincomb_batch multi_pairing_batch"),
    **_rows([B, PAIRING], "final_exp_batch miller_loop_batch pairing_batch"),
    **_rows([B, STATUS], "g1_msm g1_msm_tuned groth16_verify_batch kzg_verify_batch"),
    **_rows([B, VERIFY], """bls_verify_batch bls_verify_fused_batch bls_verify_line_table_batch bls_verify_same_signer_batch
            bls_verify_two_pairings_batch"""),
    **_rows([B, WIDE], "g1_scalar_mul_batch"),
    **_rows([FIELDS], """all_valid aos_to_soa expand_message_batch f29_hook_batch f29_raw_hook_batch flags_all fp12_hook_batch
            fp_compute_naf_batch fp_from_be_bytes_batch fr_add_batch fr_batch_inv fr_from_be_bytes_batch fr_group_powers_batch fr_inv_batch
            fr_lincomb_batch fr_mul_batch fr_neg_batch fr_spmv_batch fr_spmv_batch_tuned fr_sqr_batch fr_sub_batch fr_to_be_bytes_batch
            groth16_quotient_batch hash_to_field_batch hash_to_field_expander_batch kzg_quotient_batch kzg_quotient_evals_batch soa_to_aos"""),
    **_rows([GROUPS], "evm_ecadd_batch g1_from_be_bytes_batch g1_generator_mul_batch g2_from_be_bytes_batch g2_generator_mul_batch"),
    **_rows([JOBS], "evm_ecpairing_batch"),
    **_rows([WIDE], "bls_sign_batch bls_sign_expander_batch evm_ecmul_batch hash_to_g1_batch hash_to_g1_expander_batch"),
    **_rows([NTT], "fr_ntt_batch fr_ntt_batch_tuned"),
    "pairing_host": Row([B, HOST["pairing_host"]]), "bls_verify_host": Row([B, HOST["bls_verify_host"]]),
    **{s: Row([HOST[s]]) for s in ["pairing_host_bytes", "bls_verify_host_bytes", "host_xoshiro_fp"]},
}
MEMORY_CONTRACT = {"sylow_hip_" + k: v for k, v in MEMORY_CONTRACT.items()}
EXEMPT = {"sylow_hip_" + s for s in ["init", "init_devices", "set_device", "shutdown", "trim", "set_scratch_limit", "set_option", "get_option",
                                     "wall_clock_khz", "last_error", "device_count", "stream_sync", "host_malloc", "host_free",
                                     "g2_line_table_words", "malloc", "free", "memcpy_h2d", "memcpy_d2h", "clock_probe"]}

# @shape items of driven entry points that are not device arrays of the call, so no guarded buffer can stand behind them
NOT_AUDITED = {
    "comm": "an ncclComm_t handle (NULL = one rank), not an array",
    "dst_host": "a host byte string read before the call returns (the Python layer passes `bytes`)",
    "group_start": "a HOST array by contract (include/sylow_hip.h: the host plans scratch and routes from it)",
}


def test_every_pointer_parameter_is_const_or_output():
    from sylow_amd import _shapes
    from test_rust_ffi import parse_header
    protos, kinds = parse_header(), constness()
    for name, (names, shapes) in _shapes.parse().items():
        pointers = {p[3] for p in protos[name][1] if p[1] and p[3] != "stream"}
        assert set(shapes) <= pointers, (name, sorted(set(shapes) - pointers))
        for param in pointers:                                      # the parser saw every pointer the prototype has: none is left without a kind
            assert param in kinds[name], f"{name}: the parser did not classify {param}"
        # an array named out* / *_out / status / ok is an output, an input named *_inf with `?` is const: the parser reads the qualifier, not the name
        for param in shapes:
            if param.startswith("out") or param.endswith("_out") or param in ("status", "ok", "is_one"):
                assert kinds[name][param] is False, (name, param)
            if shapes[param].optional and param.endswith("_inf") and not param.startswith(("out", "pi_")):
                assert kinds[name][param] is True, (name, param)


def test_every_declared_entry_point_has_a_memory_contract_row():
    import __graft_entry__
    import test_gpu_memory_contract as G
    declared = set(__graft_entry__.declared_symbols())
    assert not declared - set(MEMORY_CONTRACT), f"entry points without a memory-contract row: {sorted(declared - set(MEMORY_CONTRACT))}"
    assert not set(MEMORY_CONTRACT) - declared, f"rows for entry points the header no longer declares: {sorted(set(MEMORY_CONTRACT) - declared)}"
    tables = {B: G.T.CASES, PAIRING: G.PAIRING, VERIFY: G.VERIFY, WIDE: G.WIDE, GROUPS: G.GROUPS, FIELDS: G.FIELDS, STATUS: G.STATUS, JOBS: G.JOBS}
    for name, row in MEMORY_CONTRACT.items():
        if row.exempt:
            assert not row.tests and row.exempt.strip(), name
            continue
        assert row.tests, f"{name}: a driven row names its GPU tests"
        for t in row.tests:
            assert callable(getattr(G, t, None)), f"{name}: test_gpu_memory_contract.py has no {t}"
            if t in tables:
                assert name in tables[t], f"{name}: {t} does not drive it"
        for t, table in tables.items():
            assert (name in table) == (t in row.tests), f"{name}: the row and the drivers of {t} disagree"
    assert set(G.DRIVERS) == set().union(G.PAIRING, G.VERIFY, G.WIDE, G.GROUPS, G.FIELDS, G.STATUS, G.JOBS)


def test_the_exempt_set_is_exactly_the_one_written_down():
    from sylow_amd import _shapes
    assert {n for n, r in MEMORY_CONTRACT.items() if r.exempt} == EXEMPT
    shapes = _shapes.parse()
    for name in EXEMPT:
        for param, sh in shapes.get(name, ((), {}))[1].items():
            if name == "sylow_hip_clock_probe":
                assert param == "acc"                               # an accumulator by contract
            else:
                assert param.endswith("_host"), f"{name}: exempt, but {param} is a device array"
    for s in ("malloc", "free", "memcpy_h2d", "memcpy_d2h"):
        assert "sylow_hip_" + s not in shapes                       # raw pointers and byte counts: nothing to annotate


def test_items_left_out_of_the_audit_are_what_they_are_said_to_be():
    from sylow_amd import _shapes
    from test_rust_ffi import parse_header
    protos = parse_header()
    for name, (_, shapes) in _shapes.parse().items():
        for param, sh in shapes.items():
            if param == "comm":
                assert sh.dtype == "void" and sh.optional, name
            if param in NOT_AUDITED:
                assert dict((p[3], p[2]) for p in protos[name][1])[param] or param == "comm", (name, param)     # inputs only


def test_the_audit_reports_each_kind_of_violation():
    """the audit's rules on host bytes: no kernel has to misbehave for this"""
    before = np.full(GUARD * 2 + 64, 0x5A, dtype=np.uint8)
    after = before.copy()
    audit_bytes("f", "a", before, after, 0x5A, 64, True, 64)
    after[GUARD + 9] = 1
    with pytest.raises(AssertionError, match=r"f: a is declared const and was modified at byte offset 9$"):
        audit_bytes("f", "a", before, after, 0x5A, 64, True, 64)
    audit_bytes("f", "out", before, after, 0x5A, 64, False, 32)      # inside the extent: an output may change
    after[GUARD + 40] = 1
    with pytest.raises(AssertionError, match=r"f: a write to out beyond its @shape extent of 32 bytes, at byte offset 40$"):
        audit_bytes("f", "out", before, after, 0x5A, 64, False, 32)
    after = before.copy()
    after[GUARD + 64] = 0
    with pytest.raises(AssertionError, match=r"f: a write past the end of out \(64 bytes\), at byte offset 64$"):
        audit_bytes("f", "out", before, after, 0x5A, 64, False, 64)
    after = before.copy()
    after[GUARD - 1] = 0
    with pytest.raises(AssertionError, match=r"f: a write in front of out, at byte offset -1$"):
        audit_bytes("f", "out", before, after, 0x5A, 64, False, 64)
    assert GUARD % 256 == 0 and GUARD >= 256 * 8
