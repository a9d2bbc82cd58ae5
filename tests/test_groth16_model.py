"""CPU: the Groth16 model of tests/groth16_model.py checks itself -- valid instances pass, every defect class gives the boolean its name
says, the model agrees row by row with the Solidity verifier's call sequence run through the byte-level precompile model
(tests/evm_model.py: ecMul and ecAdd per input, then ecPairing on four pairs), and the weighted product over the literal pairs is the
identity exactly for valid batches.  Also: the header declares the three entry points and their shapes."""
import numpy as np
import pytest

import evm_model as E
import groth16_model as M

L = 3


@pytest.fixture(scope="module")
def planted():
    valid = M.make_instance(12, L, seed=0x6716)
    defects = {1: "c_swapped", 3: "input_plus_one", 4: "a_negated", 5: "b_swapped", 7: "a_identity", 8: "a_c_identity_valid", 10: "vk_x_identity"}
    return valid, M.plant(valid, defects)


def test_valid_instances_pass(planted):
    valid, _ = planted
    assert M.model_verify(valid).all()
    assert M.model_verify(M.make_instance(3, 0, seed=5)).all()          # no public input: vk_x = IC_0


def test_every_defect_gives_the_boolean_its_name_says(planted):
    _, bad = planted
    assert set(bad.planted.values()) == set(M.DEFECTS)
    got, want = M.model_verify(bad), bad.expected()
    assert np.array_equal(got, want), (got, want)
    assert not want[[1, 3, 4, 5, 6, 7]].any() and want[[0, 2, 8, 9, 10, 11]].all()
    assert M.is_identity(M.model_vk_x(bad))[10] and not M.is_identity(M.model_vk_x(bad))[[0, 8]].any()


def _w(v):
    return int(v).to_bytes(32, "big")


def _g1b(xy, inf=False):
    x, y = M.ints(np.asarray(xy).reshape(2, 4))
    return bytes(64) if inf else _w(x) + _w(y)


def _g2b(xy):
    x0, x1, y0, y1 = M.ints(np.asarray(xy).reshape(4, 4))
    return _w(x1) + _w(x0) + _w(y1) + _w(y0)


def solidity_verify(inst, i):
    """the snarkjs verifier's calls for proof i: vk_x through ecMul + ecAdd per input, then ecPairing on (-A, B), (alpha, beta), (vk_x, gamma),
    (C, delta)"""
    vk_x = _g1b(inst.ic[0])
    for j in range(inst.l):
        term = E.model_mul(_g1b(inst.ic[j + 1]) + _w(inst.inputs[i][j]))
        assert term.error is None
        vk_x = E.model_add(vk_x + term.out).out
    a = inst.a[i].copy()
    a[4:8] = M.limbs([(M.P - M.ints(a[4:8])[0]) % M.P])[0]
    data = (_g1b(a, inst.a_inf[i]) + _g2b(inst.b[i]) + _g1b(inst.alpha[0]) + _g2b(inst.beta[0]) + vk_x + _g2b(inst.gamma[0])
            + _g1b(inst.c[i], inst.c_inf[i]) + _g2b(inst.delta[0]))
    res = E.model_pair(data)
    assert res.error is None
    return res.out == _w(1)


def test_model_agrees_with_the_solidity_call_sequence(planted):
    _, bad = planted
    want = M.model_verify(bad)
    assert [solidity_verify(bad, i) for i in range(bad.n)] == list(want)


def test_weighted_product_is_one_exactly_for_valid_batches(planted):
    valid, bad = planted
    w = [0x9E3779B97F4A7C15 ^ (0x1234567 * (i + 1)) for i in range(valid.n)]
    gt, literal = M.weighted_product(valid, w)
    assert literal and np.array_equal(gt, M.ONE48)
    one_bad = M.plant(valid, {4: "a_negated"})
    gt_bad, literal = M.weighted_product(one_bad, w)
    assert literal and not np.array_equal(gt_bad, M.ONE48)
    w0 = list(w)
    w0[4] = 0
    assert np.array_equal(M.weighted_product(one_bad, w0)[0], M.ONE48)


def test_header_declares_the_entry_points_and_their_shapes():
    import __graft_entry__
    from sylow_amd import _shapes
    names = {"sylow_hip_groth16_vk_x_batch", "sylow_hip_groth16_verify_batch", "sylow_hip_groth16_batch_verify_weighted"}
    assert names <= set(__graft_entry__.declared_symbols())
    shapes = _shapes.parse()
    assert names <= set(shapes)
    sh = shapes["sylow_hip_groth16_verify_batch"][1]
    assert {"vk_alpha", "vk_beta", "vk_gamma", "vk_delta", "vk_ic", "a_xy", "a_inf", "b_xy", "b_inf", "c_xy", "c_inf", "inputs", "ok"} == set(sh)
    assert sh["a_inf"].optional and not sh["vk_ic"].optional and not sh["ok"].optional
    assert {"weights", "gt_out", "is_one"} <= set(shapes["sylow_hip_groth16_batch_verify_weighted"][1])
    assert {"vk_ic", "inputs", "out_xy", "out_inf"} == set(shapes["sylow_hip_groth16_vk_x_batch"][1])
