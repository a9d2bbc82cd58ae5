"""The input contract (tests/test_gpu_input_contract.py) for the entry points of the folded KZG openings (kzg_multi.hip).  The two Fr calls
have only Fr-valued arguments and are exempt from the Fp rows; the four KZG calls take coordinate words (the SRS, the commitments, the
proofs, tau_g2) and optional flag arrays.  The rows and the cases are registered in that file's tables when the suite is collected, so its
CPU completeness tests see them.  Beside that: every entry point takes its SCALARS mod r -- the same words out for v and v + k r -- and a bad
group_start (decreasing, not starting at 0, not ending at m) is SYLOW_HIP_E_ARG with nothing written."""
import numpy as np
import pytest

import groth16_model as G
import kzg_evals_model as E
import kzg_multi_model as M
import kzg_prove_model as KP
import test_gpu_input_contract as T

R = M.R
FR_ONLY = "Fr-valued arguments: tested with their own edge values (test_gpu_fr_lincomb.py)"
ROWS = {
    "sylow_hip_fr_lincomb_batch": T.ex(FR_ONLY),
    "sylow_hip_fr_group_powers_batch": T.ex(FR_ONLY),
    "sylow_hip_kzg_open_multi_batch": T.Row({"srs_g1_xy": T.G1A}),
    "sylow_hip_kzg_open_multi_evals_batch": T.Row({"srs_lagrange_xy": T.G1A}),
    "sylow_hip_kzg_combine_openings_batch": T.Row({"c_xy": T.G1A}, ["c_inf"]),
    "sylow_hip_kzg_verify_multi_batch": T.Row({"tau_g2_xy": T.G2A, "c_xy": T.G1A, "pi_xy": T.G1A}, ["c_inf", "pi_inf"]),
}
T.CONTRACT.update(ROWS)
TAU = 0xC0FFEE0DDBA11
LOG_N, SIZES = 4, [5, 0, 4, 3]
N, GS = 1 << LOG_N, M.offsets(SIZES)
E_ARG = -2
SENTINEL = 0x5A5A5A5A5A5A5A5A
_DATA = []


def data():
    """one valid instance: polynomials, points, challenges, the model's values, and every point the calls take, from the oracle"""
    if not _DATA:
        rng = T.Xoshiro(T.SEED + 0x4D)
        m = GS[-1]
        polys = [[rng.u256() % R for _ in range(N)] for _ in range(m)]
        z = [rng.u256() % R for _ in SIZES]
        z[2] = pow(E.omega(LOG_N), 5, R)                            # a group inside the domain
        gamma = [rng.u256() % R for _ in SIZES]
        y, F, qF, yF = M.open_multi(polys, GS, z, gamma)
        d = dict(polys=polys, z=z, gamma=gamma, y=y)
        d["srs"] = KP.srs_points(TAU, N)
        d["lagrange"], inf = G.g1_gen_mul(E.lagrange_at(LOG_N, TAU))
        assert not inf.any()
        w = E.omega(LOG_N)
        d["evals"] = [[KP.evaluate(f, pow(w, i, R)) for i in range(N)] for f in polys]
        d["c"], _ = M.expected_points([KP.evaluate(f, TAU) for f in polys])
        d["pi"], d["pi_inf"] = M.expected_points([KP.evaluate(q, TAU) for q in qF])
        d["tau_g2"] = G.g2_gen_mul([TAU])[0]
        d["weights"] = [rng.u256() % R for _ in range(m)]
        _DATA.append(d)
    return _DATA[0]


def lift(vals, largest=False):
    """v + k r for every value: another word for the same element of Fr (k = 1, 2, ... in turn, or the largest that fits 256 bits)"""
    return [v + ((M.TOP - v) // R if largest else 1 + i % ((M.TOP - v) // R)) * R for i, v in enumerate(vals)]


@T.case("kzg_open_multi_batch")
def _open(eng, c, pool, nm):
    d = data()
    return list(eng.kzg_open_multi(c.fp("srs_g1_xy", d["srs"]), KP.poly_words(d["polys"]), GS, M.limbs(d["z"]), M.limbs(d["gamma"])))


@T.case("kzg_open_multi_evals_batch")
def _open_evals(eng, c, pool, nm):
    d = data()
    return list(eng.kzg_open_multi_evals(c.fp("srs_lagrange_xy", d["lagrange"]), KP.poly_words(d["evals"]), GS, M.limbs(d["z"]), M.limbs(d["gamma"])))


@T.case("kzg_combine_openings_batch")
def _combine(eng, c, pool, nm):
    d = data()
    return list(eng.kzg_combine_openings(c.fp("c_xy", d["c"]), M.limbs(d["y"]), GS, M.limbs(d["gamma"]), c.flag("c_inf", T._flags(GS[-1], 1, 13))))


@T.case("kzg_verify_multi_batch")
def _verify(eng, c, pool, nm):
    d = data()
    return [eng.kzg_verify_multi(c.fp("tau_g2_xy", d["tau_g2"]), c.fp("c_xy", d["c"]), M.limbs(d["y"]), GS, M.limbs(d["z"]), M.limbs(d["gamma"]),
                                 c.fp("pi_xy", d["pi"]), c.flag("c_inf", T._flags(GS[-1], 1, 13)), c.flag("pi_inf", d["pi_inf"]))]


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
@pytest.mark.parametrize("name", sorted(n for n, r in ROWS.items() if not r.exempt))
def test_kzg_multi_reduces_representatives(engine, name):
    base = T.check_row(engine, name, lambda eng, c: T.CASES[name](eng, c, None))
    assert any(np.asarray(b).any() for b in base), f"{name}: the canonical call produced nothing but zeros"
    d = data()
    if "open_multi" in name:                                        # both forms: the model's y, the oracle's proofs
        assert np.array_equal(base[0], M.limbs(d["y"])) and np.array_equal(base[1], d["pi"]) and np.array_equal(base[2], d["pi_inf"])
    if "verify" in name:
        assert list(base[0]) == [1, 1, 1, 0]                        # commitment 11 is flagged away: its group fails, the others hold


@pytest.mark.gpu
@pytest.mark.parametrize("largest", [False, True])
def test_scalars_are_taken_mod_r(engine, largest):
    """every Fr-valued argument of the six entry points as v and as v + k r: the same words out, the model's words"""
    d = data()
    up = lambda v: M.limbs(lift(v, largest))
    pw, lpolys, levals = M.powers(d["gamma"], GS), [lift(f, largest) for f in d["polys"]], [lift(f, largest) for f in d["evals"]]
    assert np.array_equal(engine.fr_group_powers(up(d["gamma"]), GS, GS[-1]), M.limbs(pw))
    want = np.stack([M.limbs(row) for row in M.lincomb(d["polys"], d["weights"], GS)])
    assert np.array_equal(engine.fr_lincomb(KP.poly_words(lpolys), up(d["weights"]), GS), want)
    y, pi, pi_inf = engine.kzg_open_multi(d["srs"], KP.poly_words(lpolys), GS, up(d["z"]), up(d["gamma"]))
    assert np.array_equal(y, M.limbs(d["y"])) and np.array_equal(pi, d["pi"]) and np.array_equal(pi_inf, d["pi_inf"])
    y, pi, pi_inf = engine.kzg_open_multi_evals(d["lagrange"], KP.poly_words(levals), GS, up(d["z"]), up(d["gamma"]))
    assert np.array_equal(y, M.limbs(d["y"])) and np.array_equal(pi, d["pi"]) and np.array_equal(pi_inf, d["pi_inf"])
    plain = engine.kzg_combine_openings(d["c"], M.limbs(d["y"]), GS, M.limbs(d["gamma"]))
    lifted = engine.kzg_combine_openings(d["c"], up(d["y"]), GS, up(d["gamma"]))
    wcf, wyf = M.combine_logs([KP.evaluate(f, TAU) for f in d["polys"]], d["y"], GS, d["gamma"])
    assert all(np.array_equal(a, b) for a, b in zip(plain, lifted)) and np.array_equal(lifted[2], M.limbs(wyf))
    assert np.array_equal(lifted[0], M.expected_points(wcf)[0])
    ok = engine.kzg_verify_multi(d["tau_g2"], d["c"], up(d["y"]), GS, up(d["z"]), up(d["gamma"]), d["pi"], None, d["pi_inf"])
    assert ok.all()


@pytest.mark.gpu
def test_bad_group_start_writes_nothing(engine):
    lib, d = engine.lib, data()
    m, G = GS[-1], len(SIZES)
    fill = lambda *shape: engine.to_device(np.full(shape, SENTINEL, dtype=np.uint64))
    flags = lambda n: engine.to_device(np.full(n, 7, dtype=np.uint8))
    dsrs, dpolys = engine.to_device_soa(d["srs"], 8), engine.to_device(np.ascontiguousarray(KP.poly_words(d["polys"]).transpose(0, 2, 1)))
    dz, dg, dy_in = (engine.to_device_soa(M.limbs(d[k]), 4) for k in ("z", "gamma", "y"))
    dc, dtau = engine.to_device_soa(d["c"], 8), engine.to_device_soa(d["tau_g2"], 16)
    dpi_in, dw = engine.to_device_soa(d["pi"], 8), engine.to_device_soa(M.limbs(d["weights"]), 4)
    out_f, out_pw, out_y, out_pi, out_cf, out_yf = fill(G, 4, N), fill(4, m), fill(4, m), fill(8, G), fill(8, G), fill(4, G)
    out_pi_inf, out_cf_inf, out_ok = flags(G), flags(G), flags(G)
    bad = [[0, 5, 4, 9, 12], [1, 5, 5, 9, 12], [0, 5, 5, 9, 11], [0, 5, 5, 9, 13]]      # decreasing, not from 0, ending short of m, past m
    for offsets in bad:
        gs = np.array(offsets, dtype=np.uint64)
        p, st = gs.ctypes.data, engine.stream
        rcs = [lib.sylow_hip_fr_lincomb_batch(dpolys.ptr, N, m, dw.ptr, p, G, out_f.ptr, st),
               lib.sylow_hip_fr_group_powers_batch(dg.ptr, p, G, m, out_pw.ptr, st),
               lib.sylow_hip_kzg_open_multi_batch(dsrs.ptr, dpolys.ptr, N, m, p, G, dz.ptr, dg.ptr, out_y.ptr, out_pi.ptr, out_pi_inf.ptr, st),
               lib.sylow_hip_kzg_open_multi_evals_batch(dsrs.ptr, dpolys.ptr, LOG_N, m, p, G, dz.ptr, dg.ptr, out_y.ptr, out_pi.ptr, out_pi_inf.ptr, st),
               lib.sylow_hip_kzg_combine_openings_batch(dc.ptr, None, dy_in.ptr, m, p, G, dg.ptr, out_cf.ptr, out_cf_inf.ptr, out_yf.ptr, st),
               lib.sylow_hip_kzg_verify_multi_batch(dtau.ptr, dc.ptr, None, dy_in.ptr, m, p, G, dz.ptr, dg.ptr, dpi_in.ptr, None, out_ok.ptr, st)]
        assert rcs == [E_ARG] * 6, (offsets, rcs)
        assert b"bad argument" in lib.sylow_hip_last_error()
    # a required pointer as NULL, log_n out of range, and the empty batch
    st, p = engine.stream, np.array(GS, dtype=np.uint64)
    assert lib.sylow_hip_kzg_open_multi_batch(dsrs.ptr, dpolys.ptr, N, m, None, G, dz.ptr, dg.ptr, out_y.ptr, out_pi.ptr, out_pi_inf.ptr, st) == E_ARG
    assert lib.sylow_hip_kzg_open_multi_batch(dsrs.ptr, dpolys.ptr, 0, m, p.ctypes.data, G, dz.ptr, dg.ptr, out_y.ptr, out_pi.ptr, out_pi_inf.ptr, st) == E_ARG
    assert lib.sylow_hip_kzg_open_multi_batch(dsrs.ptr, dpolys.ptr, N, m, p.ctypes.data, G, dz.ptr, None, out_y.ptr, out_pi.ptr, out_pi_inf.ptr, st) == E_ARG
    assert lib.sylow_hip_kzg_open_multi_evals_batch(dsrs.ptr, dpolys.ptr, 29, m, p.ctypes.data, G, dz.ptr, dg.ptr, out_y.ptr, out_pi.ptr, out_pi_inf.ptr, st) == E_ARG
    assert lib.sylow_hip_kzg_open_multi_evals_batch(dsrs.ptr, dpolys.ptr, -1, 0, p.ctypes.data, G, dz.ptr, dg.ptr, out_y.ptr, out_pi.ptr, out_pi_inf.ptr, st) == E_ARG
    assert lib.sylow_hip_kzg_combine_openings_batch(dc.ptr, None, None, m, p.ctypes.data, G, dg.ptr, out_cf.ptr, out_cf_inf.ptr, out_yf.ptr, st) == E_ARG
    assert lib.sylow_hip_kzg_verify_multi_batch(None, dc.ptr, None, dy_in.ptr, m, p.ctypes.data, G, dz.ptr, dg.ptr, dpi_in.ptr, None, out_ok.ptr, st) == E_ARG
    assert lib.sylow_hip_kzg_verify_multi_batch(dtau.ptr, dc.ptr, None, dy_in.ptr, m, p.ctypes.data, G, dz.ptr, dg.ptr, dpi_in.ptr, None, None, st) == E_ARG
    assert lib.sylow_hip_kzg_open_multi_batch(dsrs.ptr, dpolys.ptr, N, 0, p.ctypes.data, G, dz.ptr, dg.ptr, out_y.ptr, out_pi.ptr, out_pi_inf.ptr, st) == 0
    assert lib.sylow_hip_kzg_open_multi_batch(None, None, N, m, None, 0, None, None, None, None, None, st) == 0
    assert lib.sylow_hip_kzg_open_multi_evals_batch(None, None, LOG_N, 0, None, G, None, None, None, None, None, st) == 0
    assert lib.sylow_hip_kzg_combine_openings_batch(None, None, None, 0, None, G, None, None, None, None, st) == 0
    assert lib.sylow_hip_kzg_verify_multi_batch(None, None, None, None, m, None, 0, None, None, None, None, None, st) == 0
    engine.sync()
    for dev in (out_f, out_pw, out_y, out_pi, out_cf, out_yf):
        assert (dev.download() == SENTINEL).all(), "nothing written"
    for dev in (out_pi_inf, out_cf_inf, out_ok):
        assert (dev.download() == 7).all(), "nothing written"
