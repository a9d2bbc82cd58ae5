"""The input contract (tests/test_gpu_input_contract.py) for the three Groth16 entry points: sylow_hip_groth16_vk_x_batch,
sylow_hip_groth16_verify_batch and sylow_hip_groth16_batch_verify_weighted.  The rows and their cases are registered in that file's tables
when the suite is collected, so its CPU completeness tests see them; each runs through the same check (check_row: every Fp argument as
representatives x + k p, NULL flags against all-zero flags) at n = 64 on valid proofs with a few invalid rows."""
import numpy as np
import pytest

import groth16_model as M
import test_gpu_input_contract as T

VK = {"vk_alpha": T.G1A, "vk_beta": T.G2A, "vk_gamma": T.G2A, "vk_delta": T.G2A, "vk_ic": T.G1A}
PROOFS = {"a_xy": T.G1A, "b_xy": T.G2A, "c_xy": T.G1A}
FLAGS = ["a_inf", "b_inf", "c_inf"]
ROWS = {
    "sylow_hip_groth16_vk_x_batch": T.Row({"vk_ic": T.G1A}, []),
    "sylow_hip_groth16_verify_batch": T.Row({**VK, **PROOFS}, FLAGS),
    "sylow_hip_groth16_batch_verify_weighted": T.Row({**VK, **PROOFS}, FLAGS),
}
T.CONTRACT.update(ROWS)
N = T.D                                                            # 64
_INST = []


def instance():
    if not _INST:
        _INST.append(M.plant(M.make_instance(N, 3, seed=0xC0), {5: "a_negated", 20: "c_swapped", 33: "input_plus_one"}))
    return _INST[0]


def _vk(c, g):
    return (c.fp("vk_alpha", g.alpha), c.fp("vk_beta", g.beta), c.fp("vk_gamma", g.gamma), c.fp("vk_delta", g.delta), c.fp("vk_ic", g.ic))


def _proof_args(c, g):
    return dict(a_inf=c.flag("a_inf", T._flags(N, 1, 13)), b_inf=c.flag("b_inf", T._flags(N, 2, 17)), c_inf=c.flag("c_inf", T._flags(N, 3, 19)))


@T.case("groth16_vk_x_batch")
def _vk_x(eng, c, pool, nm):
    g = instance()
    return list(eng.groth16_vk_x(c.fp("vk_ic", g.ic), g.input_words()))


@T.case("groth16_verify_batch")
def _verify(eng, c, pool, nm):
    g = instance()
    return [eng.groth16_verify(_vk(c, g), c.fp("a_xy", g.a), c.fp("b_xy", g.b), c.fp("c_xy", g.c), g.input_words(), **_proof_args(c, g))]


@T.case("groth16_batch_verify_weighted")
def _weighted(eng, c, pool, nm):
    g = instance()
    w = M.limbs([(0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1) for i in range(N)])
    gt, one = eng.groth16_batch_verify_weighted(_vk(c, g), c.fp("a_xy", g.a), c.fp("b_xy", g.b), c.fp("c_xy", g.c), g.input_words(), w, **_proof_args(c, g))
    return [gt, np.array([one])]


def test_rows_name_real_parameters():
    from sylow_amd import _shapes
    from test_rust_ffi import parse_header
    protos, shapes = parse_header(), _shapes.parse()
    for name, row in ROWS.items():
        assert name in protos and T.CONTRACT[name] is row
        assert set(row.fp) | set(row.flags) <= {p[3] for p in protos[name][1]}, name
        assert {p for p, sh in shapes[name][1].items() if sh.optional and sh.dtype == "u8" and p.endswith("_inf")} == set(row.flags), name
        assert name in T.CASES


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_groth16_reduces_representatives(engine, name):
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"
    if name == "sylow_hip_groth16_verify_batch":
        ok = np.asarray(base[0]).astype(bool)
        assert not ok[[5, 20, 33]].any() and ok.sum() > N // 2     # planted rows fail, most others pass (flagged rows aside)
