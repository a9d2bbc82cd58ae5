"""GPU: the KZG proofs of a polynomial at every point of its domain -- sylow_hip_kzg_open_all_prepare and sylow_hip_kzg_open_all_batch(_tuned)
(kzg_open_all.hip) -- word for word against the model of tests/kzg_open_all_model.py (synthetic division on discrete logarithms, then the
oracle's fixed-base product), against the route that existed before (KzgProver.open of the polynomial repeated n times at z_i = w^i), at
2^10 against g1_generator_mul of the model's logarithms under three grid caps, and through the verifier.  The inputs and expectations of a
(size, tau) are made once per module and shared.

Planted among the polynomials of every size: coefficients >= r and 2^256 - 1, the zero polynomial and a constant (every proof flagged),
X^(n-1), a zero top coefficient, and X - w_2n^3 (F_3 = 0: an identity out of the pointwise product).  Planted among the taus: a cube root of
unity (T_0 is the identity at log_n = 2 and 4) and w_n^3 (a proof at the point equal to tau)."""
import random

import numpy as np
import pytest

import g1_ntt_model as G1M
import kzg_open_all_model as M
import kzg_prove_model as KP
import ntt_model as N
from groth16_model import ints, limbs
from ntt_model import R

pytestmark = pytest.mark.gpu
IDENTITY = limbs([0, 1]).reshape(8)
GARBAGE = np.array([0xDEADBEEF00000001, 2, 3, 0x1111111111111111, 0xFFFFFFFFFFFFFFFF, 5, 6, 0x2FFFFFFFFFFFFFFF], dtype=np.uint64)
TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
U256 = (1 << 256) - 1
NAMES = ["wide", "zero", "constant", "top", "no_top", "root"]
_CASES = {}


def tau_of(kind, log_n):
    return {"random": TAU, "cube_root": M.CUBE_ROOT, "in_domain": pow(N.omega(log_n), 3, R)}[kind]


def polynomials(log_n):
    """the six of NAMES, as lists of n ints"""
    n, rng = 1 << log_n, random.Random(0x0A11 + log_n)
    rnd = lambda: [rng.randrange(R) for _ in range(n)]
    wide = rnd()
    wide[0] = R + 5
    wide[n // 2] = U256
    root = [0] * n
    root[0] = -pow(N.omega(log_n + 1), 3, R) % R
    root[1 % n] = (root[1 % n] + 1) % R                       # n = 1: X = 1 on the domain, a constant
    return [wide, [0] * n, [R + 9] + [0] * (n - 1), [0] * (n - 1) + [1], rnd()[:n - 1] + [0], root]


def case(log_n, kind="random"):
    """tau, the SRS points, the polynomials with their values and proofs by the model: {name: (f, y ints, (pi words, pi flags))}"""
    key = (log_n, kind)
    if key not in _CASES:
        tau = tau_of(kind, log_n)
        polys = {}
        for name, f in zip(NAMES, polynomials(log_n)):
            polys[name] = (f, M.values(f, log_n), M.points(M.proof_logs(f, tau, log_n)))
        _CASES[key] = dict(tau=tau, srs=KP.srs_points(tau, 1 << log_n), polys=polys, tables={})
    return _CASES[key]


def table(engine, c):
    """the device table of a case, built once"""
    if id(engine) not in c["tables"]:
        c["tables"][id(engine)] = engine.kzg_open_all_prepare(c["srs"])
    return c["tables"][id(engine)]


def host(tab):
    return np.ascontiguousarray(tab[0].download().T), tab[1].download()


def check(got, want, what):
    (gxy, ginf), (wxy, winf) = got, want
    assert np.array_equal(np.asarray(ginf).astype(np.uint8), np.asarray(winf).astype(np.uint8)), f"{what}: flags {list(ginf)[:16]} against {list(winf)[:16]}"
    bad = np.flatnonzero((np.asarray(gxy) != np.asarray(wxy)).any(axis=-1).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} points differ, first at {bad[:8]}"


def check_polys(c, names, got, what):
    y, pxy, pinf = got
    assert y.shape == (len(names), pxy.shape[1], 4) and pxy.shape[2] == 8 and pinf.shape == pxy.shape[:2]
    for j, name in enumerate(names):
        f, wy, wpi = c["polys"][name]
        assert ints(y[j]) == wy, f"{what}: the values of {name}"
        check((pxy[j], pinf[j]), wpi, f"{what}: the proofs of {name}")
        if name in ("zero", "constant"):
            assert pinf[j].all() and all(np.array_equal(row, IDENTITY) for row in pxy[j])


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5])
def test_prepare_is_the_model_and_the_transform_of_x(engine, log_n):
    c, n = case(log_n), 1 << log_n
    got = host(table(engine, c))
    assert got[0].shape == (2 * n, 8) and got[1].shape == (2 * n,)
    logs = M.x_logs(c["tau"], log_n)
    assert [i for i, v in enumerate(logs) if v] == list(range(n + 1, 2 * n)) and (n == 1 or logs[2 * n - 1] == 1)
    check(got, M.points(M.table_logs(c["tau"], log_n)), "the model")
    xy, inf = M.points(logs)
    check(got, engine.g1_ntt(xy, inf), "g1_ntt of x")
    assert np.array_equal(xy[n + 1:][::-1], c["srs"][:n - 1])           # x_(2n-1-t) = s_t


def test_prepare_flags_the_identity_of_a_cube_root_tau(engine):
    c = case(2, "cube_root")
    xy, inf = host(table(engine, c))
    assert inf[0] == 1 and np.array_equal(xy[0], IDENTITY)
    check((xy, inf), M.points(M.table_logs(c["tau"], 2)), "the model")


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 8])
def test_against_the_model(engine, log_n, m):
    c = case(log_n)
    for names in ([NAMES[:1]] if m == 1 else [NAMES[:3], NAMES[3:]]):
        polys = KP.poly_words([c["polys"][k][0] for k in names])
        check_polys(c, names, engine.kzg_open_all(table(engine, c), polys), f"m = {m}")


def test_the_values_are_the_fr_transform(engine):
    from sylow_amd import api
    api.set_engine(engine)
    c = case(5)
    polys = KP.poly_words([c["polys"][k][0] for k in NAMES])
    y, _, _ = engine.kzg_open_all(table(engine, c), polys)
    assert np.array_equal(y, api.ntt(polys))
    _, pxy, pinf = engine.kzg_open_all(table(engine, c), polys, want_y=False)               # y_out = NULL
    check_polys(c, NAMES, (y, pxy, pinf), "without y_out")


@pytest.mark.parametrize("kind,log_n", [("random", 0), ("random", 1), ("random", 2), ("random", 3), ("random", 5), ("cube_root", 4), ("in_domain", 3)])
def test_against_open_of_the_polynomial_repeated(engine, kind, log_n):
    """the route that existed before: n openings of n copies, z_i = w^i"""
    from sylow_amd import api
    api.set_engine(engine)
    c, n = case(log_n, kind), 1 << log_n
    prover = api.KzgProver(api.G1Affine(c["srs"]))
    zs = [pow(N.omega(log_n), i, R) for i in range(n)]
    names = ["wide", "constant", "root"]
    y, pis = prover.open_all(KP.poly_words([c["polys"][k][0] for k in names]))
    assert len(pis) == len(names) and y.shape == (len(names), n, 4)
    for j, name in enumerate(names):
        wy, wpi = prover.open(KP.poly_words([c["polys"][name][0]] * n), zs)
        assert np.array_equal(y[j], wy), name
        check((pis[j].xy, pis[j].infinity), (wpi.xy, wpi.infinity), f"open of {name} repeated")


@pytest.mark.parametrize("kind,log_n", [("cube_root", 2), ("cube_root", 4), ("in_domain", 3), ("in_domain", 5)])
def test_special_taus(engine, kind, log_n):
    c = case(log_n, kind)
    xy, inf = host(table(engine, c))
    assert bool(inf[0]) == (kind == "cube_root") and int(inf.sum()) == (1 if kind == "cube_root" else 0)
    polys = KP.poly_words([c["polys"][k][0] for k in NAMES])
    check_polys(c, NAMES, engine.kzg_open_all(table(engine, c), polys), kind)
    if kind == "in_domain":                                                  # the proof at the point equal to tau is there and is no identity
        assert not c["polys"]["wide"][2][1][3 % (1 << log_n)]


def test_table_without_flags_and_a_flagged_entry_with_garbage_words(engine):
    c = case(2, "cube_root")
    xy, inf = host(table(engine, c))
    polys = KP.poly_words([c["polys"][k][0] for k in NAMES])
    assert inf[0] and np.array_equal(xy[0], IDENTITY)
    check_polys(c, NAMES, engine.kzg_open_all((xy, None), polys), "table_inf = NULL: (0, 1) is the identity")
    junk = xy.copy()
    junk[0] = GARBAGE
    check_polys(c, NAMES, engine.kzg_open_all((junk, inf), polys), "a flagged entry with garbage words")
    check_polys(c, NAMES, engine.kzg_open_all((xy, np.zeros_like(inf)), polys), "all-zero flags")


# ---- 2^10 points under three grid caps, against g1_generator_mul of the model's logarithms ------------------------------------------------
_LARGE = []


def large(engine):
    if not _LARGE:
        log_n = 10
        rng = random.Random(0x0A12)
        f = [rng.randrange(R) for _ in range(1 << log_n)]
        srs, sinf = engine.g1_generator_mul(limbs(KP.srs_logs(TAU, 1 << log_n)))
        want = engine.g1_generator_mul(limbs(M.proof_logs(f, TAU, log_n)))
        assert not sinf.any() and not want[1].any()
        _LARGE.append((engine.kzg_open_all_prepare(srs), KP.poly_words([f]), M.values(f, log_n), want))
    return _LARGE[0]


def test_the_grid_stride_walk_gives_the_same_words(engine):
    """256 lanes per block: 2^10 butterflies of the fused stage are 4 blocks, so max_blocks = 1 and 3 stride"""
    tab, polys, wy, want = large(engine)
    got = {mb: engine.kzg_open_all(tab, polys, max_blocks=mb) for mb in (1, 3, -1)}
    for mb, (y, pxy, pinf) in got.items():
        assert ints(y[0]) == wy, mb
        check((pxy[0], pinf[0]), want, f"max_blocks = {mb}")
    for mb in (1, 3):
        assert all(np.array_equal(a, b) for a, b in zip(got[mb], got[-1])), mb


def test_every_row_verifies(engine):
    from groth16_model import g2_gen_mul
    from sylow_amd import api
    api.set_engine(engine)
    log_n = 5
    c, n = case(log_n), 1 << log_n
    prover, verifier = api.KzgProver(api.G1Affine(c["srs"])), api.KzgVerifier(api.G2Affine(g2_gen_mul([TAU])[0]))
    f = c["polys"]["wide"][0]
    y, (pi,) = prover.open_all([f])
    commit = prover.commit([f])
    cs = api.G1Affine(np.repeat(commit.xy, n, 0), np.repeat(commit.infinity, n))
    zs = [pow(N.omega(log_n), i, R) for i in range(n)]
    weights = [random.Random(0x0A13).randrange(1, 1 << 128) for _ in range(n)]
    assert verifier.verify((cs, zs, y[0], pi)).all() and verifier.verify_weighted((cs, zs, y[0], pi), weights)
    bad = [(v + 1) % R for v in ints(y[0])]
    assert not verifier.verify((cs, zs, bad, pi)).any() and not verifier.verify_weighted((cs, zs, bad, pi), weights)


def test_the_planted_cases_are_what_they_claim():
    """CPU side of the inputs"""
    for log_n in (2, 5):
        n = 1 << log_n
        wide, zero, const, top, no_top, root = polynomials(log_n)
        assert wide[0] >= R and wide[n // 2] == U256 and not any(zero) and const[0] >= R and not any(const[1:])
        assert top == [0] * (n - 1) + [1] and no_top[n - 1] == 0 and any(no_top)
        assert N.ntt_radix2(root + [0] * n, log_n + 1)[3] == 0
    assert M.table_logs(M.CUBE_ROOT, 2)[0] == 0 and M.table_logs(M.CUBE_ROOT, 4)[0] == 0 and all(M.table_logs(M.CUBE_ROOT, 4)[1:])
    assert G1M.monomial_logs(tau_of("in_domain", 3), 8)[1] == pow(N.omega(3), 3, R)
