"""The input contract (tests/test_gpu_input_contract.py) for the entry points that collapse many G2 points into one: sylow_hip_g2_sum_batch,
sylow_hip_g2_lincomb_batch, sylow_hip_g2_msm and sylow_hip_g2_msm_tuned.  That file keeps one CONTRACT row per declared entry point and a GPU
case per non-exempt row; this one registers the four rows and their cases in its tables when the suite is collected, so its CPU completeness
tests see them, and runs each through the same check (check_row: every Fp argument as representatives x + k p, NULL flags against all-zero
flags) at n = 64."""
import numpy as np
import pytest

import test_gpu_input_contract as T
from test_gpu_input_contract import pool  # noqa: F401  (fixture)

ROWS = {
    "sylow_hip_g2_sum_batch": T.Row({"q_xy": T.G2A}, ["q_inf"]),
    "sylow_hip_g2_lincomb_batch": T.Row({"p_xy": T.G2A}, ["p_inf"]),
    "sylow_hip_g2_msm": T.Row({"p_xy": T.G2A}, ["p_inf"]),
    "sylow_hip_g2_msm_tuned": T.Row({"p_xy": T.G2A}, ["p_inf"]),
}
T.CONTRACT.update(ROWS)
N = T.D                                                            # 64


def _scalars(seed, n):
    rng = T.Xoshiro(T.SEED + seed)
    return T.limbs([rng.fp() for _ in range(n - 2)] + [0, 1])


@T.case("g2_sum_batch")
def _g2_sum(eng, c, pool, nm):
    p = pool["g2"].copy()
    p[N - 5:] = p[:5]                                              # repeated points: the doubling case of the fold
    return list(eng.g2_sum(c.fp("q_xy", p), q_inf=c.flag("q_inf", T._flags(N, 1, 5))))


@T.case("g2_lincomb_batch")
def _g2_lincomb(eng, c, pool, nm):
    nj, nt = 4, 16                                                 # 64 terms
    p = T._tile(pool["g2"], nj * nt, 3)
    return list(eng.g2_lincomb(c.fp("p_xy", p), _scalars(31, nj * nt), nj, nt, p_inf=c.flag("p_inf", T._flags(nj * nt, 2, 6))))


@T.case("g2_msm", "g2_msm_tuned")
def _g2_msm(eng, c, pool, nm):
    p = T._tile(pool["g2"], N, 5)
    kw = dict(window=6, min_n=0) if nm == "g2_msm_tuned" else {}   # the bucket route; the plain call takes the composed route at n = 64
    return list(eng.g2_msm(c.fp("p_xy", p), _scalars(32, N), p_inf=c.flag("p_inf", T._flags(N, 5, 9)), **kw))


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
def test_g2_sums_reduce_representatives(engine, pool, name):
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, pool))
    assert not np.asarray(base[1]).all(), f"{name}: the result should not be the identity"
