"""CPU: the model of the folded KZG openings (tests/kzg_multi_model.py) against the algebra it claims, and the boundary of the new unit: the
six entry points are declared, exported, bound and annotated; the plan header's constants are what the tests take their sizes from."""
import numpy as np
import pytest

import kzg_multi_model as M
import kzg_prove_model as KP
from helpers import SEED, Xoshiro

R = M.R
NAMES = ["sylow_hip_fr_lincomb_batch", "sylow_hip_fr_group_powers_batch", "sylow_hip_kzg_open_multi_batch", "sylow_hip_kzg_open_multi_evals_batch",
         "sylow_hip_kzg_combine_openings_batch", "sylow_hip_kzg_verify_multi_batch"]
TAU = 0xC0FFEE0DDBA11 * 0x1F2E3D4C5B6A7988 % R
SIZES = [0, 3, 1, 0, 5, 2, 0]                                       # ragged, an empty group first, in the middle and last


def instance(seed, ln=9, sizes=SIZES):
    rng = Xoshiro(SEED + seed)
    gs = M.offsets(sizes)
    polys = [[rng.u256() for _ in range(ln)] for _ in range(gs[-1])]
    z = [rng.u256() for _ in sizes]
    gamma = [rng.u256() for _ in sizes]
    return polys, gs, z, gamma


def test_entry_points_are_declared_bound_and_annotated():
    import __graft_entry__
    import sylow_amd
    from sylow_amd import _lib, _shapes
    declared = __graft_entry__.declared_symbols()
    lib, table = sylow_amd.load(), _shapes.parse()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        names, shapes = table[name]
        assert names[-1] == "stream" and len(names) == len(_lib.SIGNATURES[name]), name
        assert "group_start" in shapes and shapes["group_start"].expr == "G+1" and not shapes["group_start"].optional
    assert "sylow_hip_kzg_fold_batch" in declared                          # "fold" alone keeps its earlier meaning
    # the shape check sees a short output: G = 3 groups of len = 8 need 4 * 8 * 3 words
    live = {0x1000: 1 << 20, 0x2000: 1 << 20, 0x3000: 32 * 8 * 3 - 8}
    with pytest.raises(ValueError, match="out holds"):
        _shapes.check_call("sylow_hip_fr_lincomb_batch", (0x1000, 8, 5, 0x2000, 0x7000, 3, 0x3000), live)
    _shapes.check_call("sylow_hip_fr_lincomb_batch", (0x1000, 8, 5, 0x2000, 0x7000, 3, 0x3000), {**live, 0x3000: 32 * 8 * 3})


def test_plan_constants():
    c = M.plan_constants()
    assert c["KZGM_LINCOMB_FLUSH"] == 16 and c["KZGM_LINCOMB_TILE"] == c["KZGM_BLOCK"] == 256
    # the accumulator bound written next to the kernel: a residue and FL products of canonical factors fit 512 bits
    assert (R - 1) + c["KZGM_LINCOMB_FLUSH"] * (R - 1) ** 2 < 1 << 512
    assert (R - 1) + (c["KZGM_LINCOMB_FLUSH"] + 12) * (R - 1) ** 2 >= 1 << 512      # and not many more would
    assert c["KZGM_GRID_Y_CAP"] <= 65535 and c["KZGM_OFFSET_ARGS"] * 8 <= 4096 - 64
    assert c["KZGM_BYTES_PER_SLOT"] == KP.plan_constants()["KZG_SHORT_BYTES_PER_TERM"] + 8


def test_powers_and_lincomb_rules():
    gs = M.offsets([0, 4, 1, 0, 3])
    gamma = [5, 0, R + 1, 7, R - 1]
    assert M.powers(gamma, gs) == [1, 0, 0, 0, 1, 1, R - 1, 1]             # 0^0 = 1; gamma = r + 1 is 1; r - 1 alternates
    a = [[j + 1, M.TOP - j] for j in range(8)]
    w = [M.TOP, R, 1, 0, R - 1, 2, 3, 4]
    out = M.lincomb(a, w, gs)
    assert out[0] == [0, 0] and out[3] == [0, 0]                           # empty groups give zeros
    assert out[2] == [(R - 1) * 5 % R, (R - 1) * ((M.TOP - 4) % R) % R]
    assert out[1] == [((M.TOP % R) * 1 + 3) % R, ((M.TOP % R) * (M.TOP % R) + (M.TOP - 2)) % R]


def test_folded_quotient_is_the_fold_of_the_quotients():
    polys, gs, z, gamma = instance(1)
    y, F, qF, yF = M.open_multi(polys, gs, z, gamma)
    pw = M.powers(gamma, gs)
    for g, js in M.groups_of(gs):
        qs = [KP.quotient(polys[j], z[g])[0] for j in js]
        want = [sum(pw[j] * q[k] for j, q in zip(js, qs)) % R for k in range(len(polys[0]))]
        assert qF[g] == want, g
        assert yF[g] == sum(pw[j] * y[j] for j in js) % R
        assert all(y[j] == KP.quotient(polys[j], z[g])[1] for j in js)
    assert qF[0] == [0] * 9 and yF[0] == 0 and F[3] == [0] * 9             # an empty group: F = 0, q = 0, y_F = 0


def test_folded_row_satisfies_the_relation_and_an_altered_value_does_not():
    polys, gs, z, gamma = instance(2)
    y, F, qF, yF = M.open_multi(polys, gs, z, gamma)
    c_logs = [KP.evaluate([c % R for c in f], TAU) for f in polys]
    pi_logs = [KP.evaluate(q, TAU) for q in qF]
    cf, yf = M.combine_logs(c_logs, y, gs, gamma)
    assert yf == yF and cf == [KP.evaluate(f, TAU) for f in F]
    assert all(M.row_holds(cf[g], z[g] % R, yf[g], pi_logs[g], TAU) for g in range(len(gs) - 1))
    assert cf[0] == 0 and pi_logs[0] == 0                                  # the empty group's row: identity, 0, identity
    bad = list(y)
    bad[gs[4] + 2] = (bad[gs[4] + 2] + 1) % R                              # one y_j of group 4
    cf2, yf2 = M.combine_logs(c_logs, bad, gs, gamma)
    holds = [M.row_holds(cf2[g], z[g] % R, yf2[g], pi_logs[g], TAU) for g in range(len(gs) - 1)]
    assert holds == [g != 4 for g in range(len(gs) - 1)]


def test_gamma_zero_keeps_the_first_polynomial_and_a_cancelling_fold_is_zero():
    polys, gs, z, _ = instance(3, sizes=[3, 2])
    polys[4] = list(polys[3])
    y, F, qF, yF = M.open_multi(polys, gs, z, [0, R - 1])
    assert F[0] == [c % R for c in polys[0]] and yF[0] == y[0]             # gamma = 0: F is the group's first polynomial
    assert F[1] == [0] * 9 and qF[1] == [0] * 9 and yF[1] == 0             # gamma = -1 over two equal polynomials


def test_group_offsets_of_the_python_layer():
    from sylow_amd import api
    assert api.group_offsets([0, 3, 1], 4).tolist() == [0, 0, 3, 4] and api.group_offsets([], 0).tolist() == [0]
    for bad, m in (([2, 1], 4), ([5, -1], 4)):
        with pytest.raises(ValueError):
            api.group_offsets(bad, m)
    assert api.group_offsets([2, 2], 4).dtype == np.uint64
