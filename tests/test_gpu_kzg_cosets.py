"""GPU: the KZG proofs of a polynomial on every coset of its domain and their verifier -- the entry points of include/sylow_hip_kzg_cosets.h
(kzg_cosets.hip) -- word for word against the model of tests/kzg_cosets_model.py (long division by X^l - v^i on discrete logarithms, then
the oracle's fixed-base product; Lagrange interpolation in integers), against the routes that existed before (kzg_open_all at l = 1,
kzg_open_points of the polynomial repeated c times), under every plane count and three grid caps, at 2^10 points against g1_generator_mul of
the model's logarithms, and through the three verifiers.  The inputs and expectations of a (shape, tau) are made once per module and shared.

Planted among the polynomials: coefficients >= r and 2^256 - 1, the zero polynomial and one of degree below l (every proof flagged),
X^(n-1), a zero top coefficient, and X^l - v^3 (the quotient on coset 3 is the constant 1 and its R is zero).  Planted among the taus: a cube
root of unity and w_n^3."""
import random

import numpy as np
import pytest

import kzg_cosets_model as M
import kzg_prove_model as KP
import ntt_model as N
from groth16_model import g2_gen_mul, ints, limbs
from ntt_model import R

pytestmark = pytest.mark.gpu
IDENTITY = limbs([0, 1]).reshape(8)
GARBAGE = np.array([0xDEADBEEF00000001, 2, 3, 0x1111111111111111, 0xFFFFFFFFFFFFFFFF, 5, 6, 0x2FFFFFFFFFFFFFFF], dtype=np.uint64)
TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
U256 = (1 << 256) - 1
NAMES = ["wide", "zero", "low", "top", "no_top", "vanish"]
SMALL = [(0, 0), (0, 3), (1, 0), (1, 2), (2, 1), (3, 2)]
SHAPES = SMALL + [(2, 4), (5, 3), (4, 6)]
_CASES = {}


def tau_of(kind, log_n):
    return {"random": TAU, "cube_root": M.CUBE_ROOT, "in_domain": pow(N.omega(log_n), 3, R)}[kind]


def polynomials(log_c, log_l):
    """the six of NAMES, as lists of n ints"""
    n, l, c = 1 << (log_c + log_l), 1 << log_l, 1 << log_c
    rng = random.Random(0x0C05 + 16 * log_c + log_l)
    rnd = lambda: [rng.randrange(R) for _ in range(n)]
    wide = rnd()
    wide[0] = R + 5
    wide[n // 2] = U256
    vanish = [0] * n
    vanish[0] = -pow(M.roots(log_c, log_l)[1], 3 % c, R) % R
    vanish[l % n] = (vanish[l % n] + 1) % R                   # c = 1: X^l = 1 on the domain
    return [wide, [0] * n, [R + 9] + rnd()[1:l] + [0] * (n - l), [0] * (n - 1) + [1], rnd()[:n - 1] + [0], vanish]


def points(engine, logs):
    """q(tau) G1gen for the model's logarithms: the oracle's fixed-base product up to eight of them, g1_generator_mul beyond"""
    if len(logs) <= 8:
        return M.points(logs)
    return KP.canonical_identity(*engine.g1_generator_mul(limbs([v % R for v in logs])))


def case(engine, log_c, log_l, kind="random"):
    """tau, the SRS points, the polynomials with their values and proofs by the model: {name: (f, y ints, (pi words, pi flags))}"""
    key = (log_c, log_l, kind)
    if key not in _CASES:
        n = 1 << (log_c + log_l)
        tau = tau_of(kind, log_c + log_l)
        srs, sinf = engine.g1_generator_mul(limbs(KP.srs_logs(tau, n)))
        assert not sinf.any()
        polys = {}
        for name, f in zip(NAMES, polynomials(log_c, log_l)):
            logs = M.proof_logs(f, tau, log_c, log_l)
            polys[name] = (f, M.values(f, log_c, log_l), points(engine, logs), logs)
        _CASES[key] = dict(tau=tau, srs=srs, polys=polys, table=engine.kzg_open_cosets_prepare(srs, log_l), shape=(log_c, log_l))
    return _CASES[key]


def host(tab):
    """([l, 2c, 8] words, [l, 2c] flags)"""
    return np.ascontiguousarray(tab[0].download().transpose(0, 2, 1)), tab[1].download()


def check(got, want, what):
    (gxy, ginf), (wxy, winf) = got, want
    assert np.array_equal(np.asarray(ginf).astype(np.uint8), np.asarray(winf).astype(np.uint8)), f"{what}: flags {list(ginf)[:16]} against {list(winf)[:16]}"
    bad = np.flatnonzero((np.asarray(gxy) != np.asarray(wxy)).any(axis=-1).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} points differ, first at {bad[:8]}"


def check_polys(c, names, got, what):
    y, pxy, pinf = got
    cc = 1 << c["shape"][0]
    assert pxy.shape == (len(names), cc, 8) and pinf.shape == (len(names), cc)
    for j, name in enumerate(names):
        f, wy, wpi, _ = c["polys"][name]
        if y is not None:
            assert ints(y[j]) == wy, f"{what}: the values of {name}"
        check((pxy[j], pinf[j]), wpi, f"{what}: the proofs of {name}")
        if name in ("zero", "low"):
            assert pinf[j].all() and all(np.array_equal(row, IDENTITY) for row in pxy[j])


def words(c, names):
    return KP.poly_words([c["polys"][k][0] for k in names])


@pytest.mark.parametrize("log_c,log_l", SMALL)
def test_prepare_is_the_model_and_the_transform_of_x(engine, log_c, log_l):
    c, l, cc = case(engine, log_c, log_l), 1 << log_l, 2 << log_c
    xy, inf = host(c["table"])
    assert xy.shape == (l, cc, 8) and inf.shape == (l, cc)
    logs = [M.x_logs(c["tau"], a, log_c, log_l) for a in range(l)]
    want = M.table_logs(c["tau"], log_c, log_l)
    x_xy, x_inf = np.tile(IDENTITY, (l, cc, 1)), np.ones((l, cc), dtype=np.uint8)
    for a in range(l):
        assert [k for k, v in enumerate(logs[a]) if v] == list(range(cc // 2 + 1, cc))
        for u in range(cc // 2 - 1):                                 # x^(a)_(2c-1-u) = s_(a + l u)
            assert logs[a][cc - 1 - u] == pow(c["tau"], a + l * u, R)
            x_xy[a, cc - 1 - u], x_inf[a, cc - 1 - u] = c["srs"][a + l * u], 0
    got = engine.g1_ntt(x_xy, x_inf)
    for a in range(l):
        check((xy[a], inf[a]), M.points(want[a]), f"the model, array {a}")
        check((xy[a], inf[a]), (got[0][a], got[1][a]), f"g1_ntt of x, array {a}")
    if log_l == 0:
        oxy, oinf = engine.kzg_open_all_prepare(c["srs"])
        check((xy[0], inf[0]), (np.ascontiguousarray(oxy.download().T), oinf.download()), "kzg_open_all_prepare")


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("log_c,log_l", SHAPES)
def test_against_the_model(engine, log_c, log_l, m):
    from sylow_amd import api
    api.set_engine(engine)
    c = case(engine, log_c, log_l)
    for names in ([NAMES[:1]] if m == 1 else [NAMES[:3], NAMES[3:]]):
        polys = words(c, names)
        y, pxy, pinf = engine.kzg_open_cosets(c["table"], polys, log_l)
        check_polys(c, names, (y, pxy, pinf), f"m = {m}")
        assert np.array_equal(y, api.ntt(polys))


@pytest.mark.parametrize("log_c,log_l", [(1, 2), (3, 2), (2, 4), (5, 3)])
def test_every_plane_count_and_grid_cap_gives_the_same_words(engine, log_c, log_l):
    c = case(engine, log_c, log_l)
    polys = words(c, NAMES)
    base = engine.kzg_open_cosets(c["table"], polys, log_l)
    check_polys(c, NAMES, base, "default")
    for planes_log in range(log_l + 1):
        for mb in (1, 3, -1):
            got = engine.kzg_open_cosets(c["table"], polys, log_l, want_y=False, max_blocks=mb, planes_log=planes_log)
            assert got[0] is None and np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2]), (planes_log, mb)


def test_cells_of_the_api_are_the_strided_values(engine):
    from sylow_amd import api
    api.set_engine(engine)
    log_c, log_l = 3, 2
    c = case(engine, log_c, log_l)
    prover = api.KzgProver(api.G1Affine(c["srs"]))
    cells, pis = prover.open_cosets(words(c, NAMES), log_l)
    assert cells.shape == (len(NAMES), 8, 4, 4) and len(pis) == len(NAMES) and log_l in prover._open_cosets_tables
    for j, name in enumerate(NAMES):
        f, wy, wpi, _ = c["polys"][name]
        assert [ints(cells[j, i]) for i in range(8)] == M.cells(wy, log_c, log_l), name
        check((pis[j].xy, pis[j].infinity), wpi, name)
    with pytest.raises(ValueError):
        prover.open_cosets(words(c, NAMES), 6)


@pytest.mark.parametrize("log_n", [0, 1, 3, 5])
def test_single_point_cosets_are_open_all(engine, log_n):
    c = case(engine, log_n, 0)
    polys = words(c, NAMES)
    want = engine.kzg_open_all(engine.kzg_open_all_prepare(c["srs"]), polys)
    got = engine.kzg_open_cosets(c["table"], polys, 0)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("kind,log_c,log_l", [("random", 1, 2), ("random", 3, 2), ("random", 2, 4), ("random", 4, 6), ("cube_root", 2, 1), ("in_domain", 3, 2)])
def test_against_open_points_of_the_polynomial_repeated(engine, kind, log_c, log_l):
    """the route that existed before: c openings of c copies at the points of each coset"""
    c, cc = case(engine, log_c, log_l, kind), 1 << log_c
    names = ["wide", "low", "vanish"]
    y, pxy, pinf = engine.kzg_open_cosets(c["table"], words(c, names), log_l)
    z = limbs([x for i in range(cc) for x in M.coset(i, log_c, log_l)]).reshape(cc, 1 << log_l, 4)
    for j, name in enumerate(names):
        wy, wpi, winf = engine.kzg_open_points(c["srs"], KP.poly_words([c["polys"][name][0]] * cc), z)
        check((pxy[j], pinf[j]), (wpi, winf), f"open_points of {name} repeated")
        assert [ints(v) for v in wy] == M.cells(ints(y[j]), log_c, log_l), name


@pytest.mark.parametrize("kind,log_c,log_l", [("cube_root", 2, 0), ("cube_root", 2, 2), ("cube_root", 3, 1), ("in_domain", 3, 2), ("in_domain", 2, 3)])
def test_special_taus(engine, kind, log_c, log_l):
    c = case(engine, log_c, log_l, kind)
    xy, inf = host(c["table"])
    want = M.table_logs(c["tau"], log_c, log_l)
    assert [[int(v) for v in row] for row in inf] == [[int(v == 0) for v in t] for t in want]
    if kind == "cube_root" and log_l == 0:
        assert inf[0][0] == 1                                              # 1 + tau + tau^2 = 0
    check_polys(c, NAMES, engine.kzg_open_cosets(c["table"], words(c, NAMES), log_l), kind)


def test_table_without_flags_and_a_flagged_entry_with_garbage_words(engine):
    log_c, log_l = 2, 0
    c = case(engine, log_c, log_l, "cube_root")
    xy, inf = host(c["table"])
    polys = words(c, NAMES)
    assert inf[0][0] and np.array_equal(xy[0][0], IDENTITY)
    check_polys(c, NAMES, engine.kzg_open_cosets((xy, None), polys, log_l), "table_inf = NULL: (0, 1) is the identity")
    junk = xy.copy()
    junk[0][0] = GARBAGE
    check_polys(c, NAMES, engine.kzg_open_cosets((junk, inf), polys, log_l), "a flagged entry with garbage words")
    c = case(engine, 2, 2)
    xy, inf = host(c["table"])
    assert not inf.any()
    check_polys(c, NAMES, engine.kzg_open_cosets((xy, None), words(c, NAMES), 2), "table_inf = NULL at (2, 2)")


@pytest.mark.parametrize("log_c,log_l", SMALL + [(2, 4), (1, 7)])
def test_interpolation_is_lagrange(engine, log_c, log_l):
    cc, l = 1 << log_c, 1 << log_l
    rng = random.Random(0x0C0A + 16 * log_c + log_l)
    idx = list(range(cc)) + [cc, cc + 1, 5 * cc + (cc - 1), (1 << 64) - 1]
    vals = [[rng.randrange(R) for _ in range(l)] for _ in idx]
    vals[0][0], vals[1 % len(idx)][l - 1] = R + 3, U256
    r, ok = engine.kzg_coset_interp(idx, KP.poly_words(vals), log_c, log_l)
    assert [int(v) for v in ok] == [int(i < cc) for i in idx]
    for j, i in enumerate(idx):
        want = M.interp_lagrange(vals[j], i, log_c, log_l) if l <= 16 else M.interp_twist(vals[j], i, log_c, log_l)
        assert ints(r[j]) == want, (j, i)


# ---- through the verifiers ---------------------------------------------------------------------------------------------------------------
def rows_of(engine, log_c, log_l):
    """every coset of "wide" and of "vanish" (coset 3 mod c of it has R = 0 and the constant quotient), and of "low" (every proof flagged)"""
    from sylow_amd import api
    api.set_engine(engine)
    c, cc = case(engine, log_c, log_l), 1 << log_c
    names = ["wide", "vanish", "low"]
    commits = engine.g1_generator_mul(limbs([M.evaluate([v % R for v in c["polys"][k][0]], c["tau"]) for k in names]))
    cxy, cinf, idx, cells, pxy, pinf = [], [], [], [], [], []
    for j, name in enumerate(names):
        f, wy, (wxy, winf), _ = c["polys"][name]
        for i in range(cc):
            cxy.append(commits[0][j]); cinf.append(commits[1][j]); idx.append(i); cells.append(M.cells(wy, log_c, log_l)[i]); pxy.append(wxy[i]); pinf.append(winf[i])
    tau_l = np.asarray(g2_gen_mul([pow(c["tau"], 1 << log_l, R)])[0], dtype=np.uint64)
    verifier = api.KzgCosetVerifier(api.G1Affine(c["srs"][:1 << log_l]), api.G2Affine(tau_l), log_c, log_l)
    return c, verifier, api.G1Affine(np.array(cxy), np.array(cinf)), idx, np.array([limbs(v) for v in cells]), api.G1Affine(np.array(pxy), np.array(pinf))


@pytest.mark.parametrize("log_c,log_l", [(0, 3), (1, 0), (2, 1), (3, 2), (2, 4)])
def test_every_row_verifies(engine, log_c, log_l):
    from sylow_amd import api
    c, verifier, cs, idx, cells, pis = rows_of(engine, log_c, log_l)
    rows, l = len(idx), 1 << log_l
    weights = [random.Random(0x0C0B).randrange(1, 1 << 128) for _ in range(rows)]
    assert verifier.verify(cs, idx, cells, pis).all() and verifier.verify_line_table(cs, idx, cells, pis).all()
    assert verifier.verify_weighted(cs, idx, cells, pis, weights)
    cred, z, ok = verifier.reduce(cs, idx, cells)
    assert ok.all() and ints(z) == [pow(M.roots(log_c, log_l)[1], i, R) for i in idx]
    if l <= 8:                                                       # the same rows under the several-point verifier with the model's G2 powers
        g2 = np.asarray(g2_gen_mul(KP.srs_logs(c["tau"], l + 1))[0], dtype=np.uint64)
        points = api.KzgPointsVerifier(api.G1Affine(c["srs"][:l]), api.G2Affine(g2))
        zs = limbs([x for i in idx for x in M.coset(i, log_c, log_l)]).reshape(rows, l, 4)
        assert points.verify(cs, zs, cells, pis).all()


def test_altered_rows_are_rejected_alone(engine):
    log_c, log_l = 3, 2
    c, verifier, cs, idx, cells, pis = rows_of(engine, log_c, log_l)
    cc, rows = 1 << log_c, len(idx)
    weights = [random.Random(0x0C0C).randrange(1, 1 << 128) for _ in range(rows)]

    def run(idx=idx, cells=cells, pis=pis, bad=None):
        want = [j != bad for j in range(rows)]
        assert list(verifier.verify(cs, idx, cells, pis)) == want and list(verifier.verify_line_table(cs, idx, cells, pis)) == want, bad
        assert verifier.verify_weighted(cs, idx, cells, pis, weights) == (bad is None), bad
        if bad is not None:
            assert verifier.verify_weighted(cs, idx, cells, pis, [0 if j == bad else w for j, w in enumerate(weights)]), bad

    run()
    from sylow_amd import api
    plus = cells.copy()
    plus[2, 1] = limbs([(ints(cells[2, 1:2])[0] + 1) % R])[0]
    run(cells=plus, bad=2)                                           # one cell value + 1
    run(idx=[i if j != 4 else 5 for j, i in enumerate(idx)], bad=4)  # the index of another coset
    other = pis.xy.copy()
    other[1] = pis.xy[6]
    run(pis=api.G1Affine(other, pis.infinity), bad=1)                # the proof of another coset
    run(idx=[i if j != 7 else cc for j, i in enumerate(idx)], bad=7)  # idx = c: the words of coset 0, out of range
    # idx = c + 7 names coset 7's words and is refused by its range alone
    run(idx=[i if j != 7 else cc + 7 for j, i in enumerate(idx)], bad=7)
    flagged = pis.infinity.copy()
    assert not flagged[3]
    flagged[3] = 1
    run(pis=api.G1Affine(pis.xy, flagged), bad=3)                    # a flagged pi on a non-constant quotient
    assert pis.infinity[2 * cc:].all()                               # while the flagged proofs of "low" are what its rows need


def test_a_larger_shape_against_the_generator_products(engine):
    """2^10 points, 256 cosets of 4, two polynomials: against g1_generator_mul of the model's logarithms"""
    log_c, log_l, n = 8, 2, 1 << 10
    rng = random.Random(0x0C0D)
    fs = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    srs, sinf = engine.g1_generator_mul(limbs(KP.srs_logs(TAU, n)))
    assert not sinf.any()
    y, pxy, pinf = engine.kzg_open_cosets(engine.kzg_open_cosets_prepare(srs, log_l), KP.poly_words(fs), log_l)
    for j, f in enumerate(fs):
        want = engine.g1_generator_mul(limbs(M.proof_logs(f, TAU, log_c, log_l)))
        assert ints(y[j]) == M.values(f, log_c, log_l) and not want[1].any()
        check((pxy[j], pinf[j]), want, f"polynomial {j}")


def test_argument_errors_and_the_empty_batch(engine):
    lib, st = engine.lib, engine.stream
    E_ARG, SENTINEL = -2, 0x5A5A5A5A5A5A5A5A
    log_c, log_l, m = 2, 1, 2
    c = case(engine, log_c, log_l)
    n, cc, l = 8, 4, 2
    fill = lambda *shape: engine.to_device(np.full(shape, SENTINEL, dtype=np.uint64))
    flags = lambda count: engine.to_device(np.full(count, 7, dtype=np.uint8))
    dt, dti = c["table"]
    dsrs = engine.to_device_soa(c["srs"], 8)
    dpolys = engine.to_device(np.ascontiguousarray(words(c, NAMES[:m]).transpose(0, 2, 1)))
    didx = engine.to_device(np.arange(m, dtype=np.uint64))
    dg2 = engine.to_device_soa(np.asarray(g2_gen_mul([TAU])[0], dtype=np.uint64), 16)
    out_t, out_ti, out_y, out_pi, out_pf, out_r, out_g, out_z, out_ok = fill(l, 8, 2 * cc), flags(l * 2 * cc), fill(m, 4, n), fill(m, 8, cc), flags(m * cc), fill(m, 4, l), flags(m), fill(4, m), flags(m)
    prep = lambda s=dsrs.ptr, lc=log_c, ll=log_l, t=out_t.ptr, ti=out_ti.ptr: lib.sylow_hip_kzg_open_cosets_prepare(s, lc, ll, t, ti, st)
    opn = lambda t=dt.ptr, co=dpolys.ptr, lc=log_c, ll=log_l, mm=m, mb=-1, pl=-1, y=out_y.ptr, pi=out_pi.ptr, pf=out_pf.ptr: \
        lib.sylow_hip_kzg_open_cosets_batch_tuned(t, dti.ptr, co, lc, ll, mm, mb, pl, y, pi, pf, st)
    itp = lambda v=dpolys.ptr, ix=didx.ptr, lc=log_c, ll=log_l, rr=m, r=out_r.ptr: lib.sylow_hip_kzg_coset_interp_batch(v, ix, lc, ll, rr, r, out_g.ptr, st)
    red = lambda s=dsrs.ptr, cx=out_pi.ptr, lc=log_c, ll=log_l, rr=m, o=out_t.ptr, oi=out_ti.ptr, z=out_z.ptr: \
        lib.sylow_hip_kzg_cosets_reduce_batch(s, cx, None, didx.ptr, dpolys.ptr, lc, ll, rr, o, oi, z, None, st)
    ver = lambda g2=dg2.ptr, lc=log_c, ll=log_l, rr=m, ok=out_ok.ptr: lib.sylow_hip_kzg_verify_cosets_batch(dsrs.ptr, g2, dsrs.ptr, None, didx.ptr, dpolys.ptr, lc, ll, rr, dsrs.ptr, None, ok, st)
    for call in (prep, opn, itp, red, ver):
        assert call(lc=-1) == E_ARG and call(ll=-1) == E_ARG and call(lc=14, ll=14) == E_ARG and call(lc=28, ll=0) == E_ARG
        assert b"bad argument" in lib.sylow_hip_last_error()
    assert prep(s=None) == E_ARG and prep(t=None) == E_ARG and prep(ti=None) == E_ARG
    assert opn(t=None) == E_ARG and opn(co=None) == E_ARG and opn(pi=None) == E_ARG and opn(pf=None) == E_ARG
    assert opn(mb=0) == E_ARG and opn(pl=log_l + 1) == E_ARG
    assert opn(y=dpolys.ptr) == E_ARG and opn(pi=dpolys.ptr + 8) == E_ARG and opn(pi=dt.ptr) == E_ARG, "outputs overlapping inputs"
    assert itp(v=None) == E_ARG and itp(ix=None) == E_ARG and itp(r=None) == E_ARG and itp(r=dpolys.ptr) == E_ARG
    assert red(s=None) == E_ARG and red(cx=None) == E_ARG and red(o=None) == E_ARG and red(oi=None) == E_ARG and red(z=None) == E_ARG and red(o=out_pi.ptr) == E_ARG
    assert ver(g2=None) == E_ARG and ver(ok=None) == E_ARG
    # the empty batch: OK, nothing launched, nothing written, whatever the pointers are
    assert opn(mm=0) == 0 and itp(rr=0) == 0 and red(rr=0) == 0 and ver(rr=0) == 0
    assert lib.sylow_hip_kzg_open_cosets_batch(None, None, None, log_c, log_l, 0, None, None, None, st) == 0
    assert lib.sylow_hip_kzg_coset_interp_batch(None, None, log_c, log_l, 0, None, None, st) == 0
    assert lib.sylow_hip_kzg_cosets_reduce_batch(None, None, None, None, None, log_c, log_l, 0, None, None, None, None, st) == 0
    assert lib.sylow_hip_kzg_verify_cosets_batch(None, None, None, None, None, None, log_c, log_l, 0, None, None, None, st) == 0
    engine.sync()
    for dev in (out_t, out_y, out_pi, out_r, out_z):
        assert (dev.download() == SENTINEL).all(), "nothing written"
    for dev in (out_ti, out_pf, out_g, out_ok):
        assert (dev.download() == 7).all(), "nothing written"
    y, pxy, pinf = engine.kzg_open_cosets(c["table"], np.zeros((0, n, 4), dtype=np.uint64), log_l)
    assert y.shape == (0, n, 4) and pxy.shape == (0, cc, 8) and pinf.shape == (0, cc)


def test_the_planted_cases_are_what_they_claim():
    """CPU side of the inputs"""
    for log_c, log_l in ((3, 2), (2, 4)):
        n, l, c = 1 << (log_c + log_l), 1 << log_l, 1 << log_c
        wide, zero, low, top, no_top, vanish = polynomials(log_c, log_l)
        assert wide[0] >= R and wide[n // 2] == U256 and not any(zero) and low[0] >= R and any(low[1:l]) and not any(low[l:])
        assert top == [0] * (n - 1) + [1] and no_top[n - 1] == 0 and any(no_top)
        q, rem = M.divide(vanish, 3 % c, log_c, log_l)
        assert q == [1] + [0] * (n - 1) and rem == [0] * l
        assert M.proof_logs(low, TAU, log_c, log_l) == [0] * c and M.proof_logs(vanish, TAU, log_c, log_l)[3 % c] == 1
    assert M.table_logs(M.CUBE_ROOT, 2, 0)[0][0] == 0
