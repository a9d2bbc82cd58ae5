"""GPU: one KZG polynomial opened at several points under one proof -- the five entry points of include/sylow_hip_kzg_points.h
(kzg_points.hip) -- against the integer model of tests/kzg_points_model.py.  Everything is exact: the quotient, y, the weights, Z and R word
for word against the model; the quotient word for word against the composition of the calls that were there before (coefficients replicated
k times, sylow_hip_kzg_quotient_batch, sylow_hip_fr_lincomb_batch under the weights); the proofs word for word against the oracle's
q(tau) G1gen; the verifier's flags against the model's decision.  L and CH are the scan's lane run and chunk (kzg_prove_plan.hpp): CH + 1
takes the three-launch route, 257 chunks cross a tile of the carry level."""
import random

import numpy as np
import pytest

import groth16_model as G
import kzg_points_model as M
import kzg_prove_model as KP
from kzg_points_model import R, TOP

pytestmark = pytest.mark.gpu
PLAN = M.plan_constants()
L, CH, BLOCK, KMAX = PLAN["KZG_POLY_LANE_COEFFS"], PLAN["KZG_POLY_CHUNK"], PLAN["KZG_POLY_BLOCK"], PLAN["KZGPT_MAX_POINTS"]
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
N_SRS = 261
E_ARG = -2
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def srs():
    return KP.srs_points(TAU, N_SRS)


@pytest.fixture(scope="module")
def srs_g2():
    xy, inf = G.g2_gen_mul(KP.srs_logs(TAU, 9))
    assert not np.asarray(inf).any()
    return np.asarray(xy, dtype=np.uint64)


def rand_poly(rng, n):
    f = [rng.randrange(R) for _ in range(n)]
    for i, w in enumerate(M.EDGE_WORDS):
        if 2 * i < n:
            f[(i * 37) % n if i % 2 else n - 1 - (i * 11) % n] = w
    return f


def alias(v):
    """another 256-bit word for the same element of Fr"""
    return v + R if v < R else v % R


def rand_rows(rng, m, k):
    return [[rng.randrange(1 << 256) for _ in range(k)] for _ in range(m)]


def check_quotient(engine, polys, rows):
    """q and y of one call, word for word against the model"""
    want = [M.quotient_points(f, zs) for f, zs in zip(polys, rows)]
    q, y = engine.kzg_quotient_points(KP.poly_words(polys), M.row_words(rows))
    assert np.array_equal(y, M.row_words([wy for _, wy in want])), "y against the integer evaluation"
    assert np.array_equal(q, KP.poly_words([wq for wq, _ in want])), "q against the model's sum_i a_i q_i"
    return q, y


@pytest.mark.parametrize("k", [3, 8])
def test_quotient_lengths_against_the_model(engine, k):
    rng = random.Random(0xA0 + k)
    for n in sorted({1, 2, k - 1, k, k + 1, L, CH - 1, CH, CH + 1, 3 * CH + L + 1}):
        polys = [rand_poly(rng, n), [rng.randrange(1 << 256) for _ in range(n)]]
        q, _ = check_quotient(engine, polys, rand_rows(rng, 2, k))
        assert not q[:, max(n - k, 0):].any(), f"len {n}: the top k coefficients of f div Z are zero"


def test_quotient_across_a_tile_of_the_carry_level(engine):
    """257 chunks at k = 2: the running carry passes from the second tile of BLOCK chunks into the first"""
    n = BLOCK * CH + 1
    rng = random.Random(0xA1)
    words = np.frombuffer(rng.randbytes(32 * n), dtype=np.uint64).reshape(1, n, 4).copy()
    rows = rand_rows(rng, 1, 2)
    wq, wy = M.quotient_points(M.ints(words[0]), rows[0])
    q, y = engine.kzg_quotient_points(words, M.row_words(rows))
    assert np.array_equal(y, M.row_words([wy])) and np.array_equal(q[0], M.limbs(wq))


@pytest.mark.parametrize("k", [1, 2, 3, 8, 17, 64])
def test_quotient_point_counts_against_the_model(engine, k):
    """five polynomials of two chunks: (polynomial, point) items mix in the totals and carry passes"""
    rng = random.Random(0xA2 + k)
    polys = [rand_poly(rng, CH + 1) for _ in range(5)]
    check_quotient(engine, polys, rand_rows(rng, 5, k))


def edge_instance(rng, n):
    """row 0: the edge words as points, distinct mod r; row 1: r and r + 1 for 0 and 1; row 2: 7 and 7 + r collide, 9 and 2^256 - 1 stay;
    row 3: every point the same"""
    rows = [[0, 1, R - 1, M.P, TOP], [R, R + 1, 5, 2 * R - 1, 3 * R + 2], [7, 9, 7 + R, TOP, 11], [R - 1, 2 * R - 1, 3 * R - 1, R - 1, R - 1]]
    return [rand_poly(rng, n) for _ in rows], rows


@pytest.mark.parametrize("n", [4, 40, CH + 1])
def test_edge_values_and_repeated_points(engine, n):
    rng = random.Random(0xA3 + n)
    polys, rows = edge_instance(rng, n)
    polys[1] = [M.EDGE_WORDS[i % len(M.EDGE_WORDS)] for i in range(n)]
    check_quotient(engine, polys, rows)
    a, distinct = engine.kzg_points_weights(M.row_words(rows))
    want = [M.weights(zs) for zs in rows]
    assert np.array_equal(a, M.row_words([w for w, _ in want])) and list(distinct) == [1, 1, 0, 0] == [int(d) for _, d in want]
    assert not a[3].any() and a[2][0].sum() == 0 and a[2][2].sum() == 0 and a[2][1].any()       # the colliding points drop out


def test_weights_of_one_point_and_many_rows(engine):
    rng = random.Random(0xA4)
    a, distinct = engine.kzg_points_weights(M.row_words(rand_rows(rng, 3, 1)))
    assert np.array_equal(a, M.row_words([[1]] * 3)) and distinct.all()
    rows = rand_rows(rng, 70, KMAX)                                # 4480 pairs: more than one chunk of the shared inversion
    rows[69][63] = alias(rows[69][0])
    a, distinct = engine.kzg_points_weights(M.row_words(rows))
    want = [M.weights(zs) for zs in rows]
    assert np.array_equal(a, M.row_words([w for w, _ in want])) and list(distinct) == [1] * 69 + [0]


def test_either_output_alone(engine):
    rng = random.Random(0xA5)
    for n in (33, CH + 1):
        polys, rows = [rand_poly(rng, n) for _ in range(3)], rand_rows(rng, 3, 4)
        q, y = check_quotient(engine, polys, rows)
        q_only, none = engine.kzg_quotient_points(KP.poly_words(polys), M.row_words(rows), want_y=False)
        assert none is None and np.array_equal(q_only, q)
        none, y_only = engine.kzg_quotient_points(KP.poly_words(polys), M.row_words(rows), want_q=False)
        assert none is None and np.array_equal(y_only, y)


@pytest.mark.parametrize("n", [1, 2, CH, CH + 1])
def test_one_point_is_the_single_point_call(engine, n):
    rng = random.Random(0xA6 + n)
    polys, rows = [rand_poly(rng, n) for _ in range(3)], rand_rows(rng, 3, 1)
    q, y = engine.kzg_quotient_points(KP.poly_words(polys), M.row_words(rows))
    q1, y1 = engine.kzg_quotient(KP.poly_words(polys), M.limbs([r[0] for r in rows]))
    assert np.array_equal(q, q1) and np.array_equal(y[:, 0], y1)


@pytest.mark.parametrize("k,n", [(2, 9), (5, CH + 1), (17, 300), (64, 70)])
def test_quotient_equals_the_composition(engine, k, n):
    """coefficients replicated k times, sylow_hip_kzg_quotient_batch, then sylow_hip_fr_lincomb_batch under the weights: the same words"""
    rng = random.Random(0xA7 + k)
    m = 3
    polys, rows = [rand_poly(rng, n) for _ in range(m)], rand_rows(rng, m, k)
    rows[2][k - 1] = alias(rows[2][0])                                # a row with a repeat goes the same way on both sides
    q, y = engine.kzg_quotient_points(KP.poly_words(polys), M.row_words(rows))
    a, _ = engine.kzg_points_weights(M.row_words(rows))
    rep = np.repeat(KP.poly_words(polys), k, axis=0)
    qi, yi = engine.kzg_quotient(rep, M.row_words(rows).reshape(m * k, 4))
    folded = engine.fr_lincomb(qi, a.reshape(m * k, 4), [j * k for j in range(m + 1)])
    assert np.array_equal(y.reshape(m * k, 4), yi) and np.array_equal(q, folded)


@pytest.mark.parametrize("k", [1, 4, 8])
def test_open_points_against_the_oracle(engine, srs, k):
    rng = random.Random(0xB0 + k)
    for n in sorted({1, k, k + 1, 40, N_SRS}):
        polys = [rand_poly(rng, n), rand_poly(rng, n), [rng.randrange(R)] + [0] * (n - 1), [rng.randrange(R) for _ in range(min(n, k))] + [0] * (n - min(n, k))]
        polys[0][-1], polys[1][-1] = rng.randrange(1, R), R + 1     # a top coefficient that is not zero: the quotient of len = k + 1 is it
        rows = rand_rows(rng, len(polys), k)
        wy, wpi, winf = M.expected_open(polys, rows, TAU)
        y, pi, pi_inf = engine.kzg_open_points(srs[:n], KP.poly_words(polys), M.row_words(rows))
        assert np.array_equal(y, M.row_words(wy)), "y against the integer evaluation"
        assert np.array_equal(pi_inf, winf) and np.array_equal(pi, wpi), "pi against the oracle's q(tau) G1gen"
        # a constant polynomial and one of degree below k have a zero quotient; so has every polynomial of len <= k
        assert list(pi_inf) == ([1] * 4 if n <= k else [0, 0, 1, 1])


@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_fr_half_against_the_model(engine, k):
    rng = random.Random(0xB1 + k)
    rows, ys = rand_rows(rng, 5, k), rand_rows(rng, 5, k)
    if k > 1:
        rows[3][k - 1] = alias(rows[3][0])
    rows[4][0], ys[4][0] = TOP, TOP
    Z, Rp, distinct = engine.kzg_points_polys(M.row_words(rows), M.row_words(ys))
    assert np.array_equal(Z, KP.poly_words([M.vanishing(zs) for zs in rows])), "Z against the model's product"
    assert np.array_equal(Z[:, k], M.limbs([1] * 5)), "Z is monic"
    assert np.array_equal(Rp, KP.poly_words([M.remainder_points(zs, y) for zs, y in zip(rows, ys)])), "R against the model"
    assert list(distinct) == [1, 1, 1, int(k == 1), 1]
    f = [rng.randrange(R) for _ in range(k + 3)]                   # R is the interpolant: f mod Z from the values of f
    _, Rf, _ = engine.kzg_points_polys(M.row_words(rows[:1]), M.row_words([[KP.evaluate(f, z % R) for z in rows[0]]]))
    assert np.array_equal(Rf[0], M.limbs(M.long_division(f, M.vanishing(rows[0]))[1]))


def verifier_instance(engine, srs, k, n=40):
    """six rows opened by the library: row 4 has a zero quotient (degree below k), row 5 a repeated point whose other data is consistent"""
    rng = random.Random(0xB2 + k)
    polys = [rand_poly(rng, n) for _ in range(6)]
    polys[4] = [rng.randrange(R) for _ in range(k)] + [0] * (n - k)
    rows = rand_rows(rng, 6, k)
    if k > 1:
        rows[5][k - 1] = alias(rows[5][0])
    y, pi, pi_inf = engine.kzg_open_points(srs[:n], KP.poly_words(polys), M.row_words(rows))
    c, c_inf = KP.expected_commit(polys, TAU)
    logs = dict(c=[KP.evaluate([v % R for v in f], TAU) for f in polys], pi=[KP.evaluate(M.quotient_points(f, zs)[0], TAU) for f, zs in zip(polys, rows)])
    return polys, rows, y, pi, pi_inf, c, c_inf, logs


def model_flags(logs, rows, y, pi_logs=None, c_logs=None):
    ys = [M.ints(r) for r in np.asarray(y)]
    return [int(M.row_holds((c_logs or logs["c"])[j], rows[j], ys[j], (pi_logs or logs["pi"])[j], TAU)) for j in range(len(rows))]


def test_verifier_accepts_openings_and_rejects_altered_rows(engine, srs, srs_g2):
    k = 4
    polys, rows, y, pi, pi_inf, c, c_inf, logs = verifier_instance(engine, srs, k)
    z = M.row_words(rows)
    verify = lambda **kw: list(engine.kzg_verify_points(srs[:k], srs_g2[:k + 1], kw.get("c", c), kw.get("z", z), kw.get("y", y), kw.get("pi", pi),
                                                      kw.get("c_inf", c_inf), kw.get("pi_inf", pi_inf)))
    assert list(pi_inf) == [0, 0, 0, 0, 1, 0] and not c_inf.any()
    assert verify() == [1, 1, 1, 1, 1, 0] == model_flags(logs, rows, y), "the library's openings; the zero-quotient row; the repeated point"
    for pos in (0, k // 2, k - 1):                                 # one altered y_i at the first, a middle and the last position
        bad = y.copy()
        bad[1, pos, 0] ^= 1
        bad[4, pos, 0] ^= 1                                        # the row whose pi is the identity: C = R(tau) G1gen no longer holds
        assert verify(y=bad) == [1, 0, 1, 1, 0, 0] == model_flags(logs, rows, bad), pos
    other, other_inf = M.expected_points([logs["pi"][0] + 1, 5, logs["pi"][2], logs["pi"][3], 0, logs["pi"][5]])
    assert verify(pi=other, pi_inf=other_inf) == [0, 0, 1, 1, 1, 0], "an altered pi, and a point for pi where the model has another"
    other, other_inf = M.expected_points([logs["c"][0], logs["c"][1], logs["c"][2] + 1, 0, logs["c"][4], logs["c"][5]])
    assert verify(c=other, c_inf=other_inf) == [1, 1, 0, 0, 1, 0], "an altered C, and the identity for C"
    swapped = z.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert verify(z=swapped) == [0, 0, 1, 1, 1, 0], "the points of two rows exchanged"


def test_verifier_at_one_point_is_the_single_point_verifier(engine, srs, srs_g2):
    polys, rows, y, pi, pi_inf, c, c_inf, logs = verifier_instance(engine, srs, 1)
    z = M.row_words(rows)
    bad = y.copy()
    bad[2, 0, 3] ^= 1 << 7
    other, other_inf = M.expected_points([logs["pi"][0], logs["pi"][1] + 9] + logs["pi"][2:])
    for yy, pp, pf in ((y, pi, pi_inf), (bad, pi, pi_inf), (y, other, other_inf)):
        got = engine.kzg_verify_points(srs[:1], srs_g2[:2], c, z, yy, pp, c_inf, pf)
        single = engine.kzg_verify(srs_g2[1:2], c, z[:, 0], yy[:, 0], pp, c_inf, pf)
        assert np.array_equal(got, single)
    assert list(engine.kzg_verify_points(srs[:1], srs_g2[:2], c, z, y, pi, c_inf, pi_inf)) == [1] * 6


@pytest.mark.parametrize("k", [3, 8])
def test_verifier_in_chunks_under_a_scratch_limit(engine, srs, srs_g2, k):
    polys, rows, y, pi, pi_inf, c, c_inf, logs = verifier_instance(engine, srs, k)
    bad = y.copy()
    bad[3, k - 1, 1] ^= 1
    want = [1, 1, 1, 0, 1, 0]
    assert list(engine.kzg_verify_points(srs[:k], srs_g2[:k + 1], c, M.row_words(rows), bad, pi, c_inf, pi_inf)) == want == model_flags(logs, rows, bad)
    try:
        engine.set_scratch_limit(4 * (k + 1) * PLAN["KZGPT_G2_BYTES_PER_TERM"])        # four of the six rows per chunk of the G2 half
        assert list(engine.kzg_verify_points(srs[:k], srs_g2[:k + 1], c, M.row_words(rows), bad, pi, c_inf, pi_inf)) == want
        engine.set_scratch_limit(1)                                                   # one row per chunk
        assert list(engine.kzg_verify_points(srs[:k], srs_g2[:k + 1], c, M.row_words(rows), bad, pi, c_inf, pi_inf)) == want
    finally:
        engine.set_scratch_limit(0)


def test_api_prover_and_verifier(engine, srs, srs_g2):
    from sylow_amd import api
    rng = random.Random(0xB5)
    n, k = 24, 3
    polys, rows = [rand_poly(rng, n) for _ in range(2)], rand_rows(rng, 2, k)
    prover = api.KzgProver(api.G1Affine(srs[:n]))
    verifier = api.KzgPointsVerifier(api.G1Affine(srs[:8]), api.G2Affine(srs_g2))
    y, pi = prover.open_points(polys, rows)
    assert np.array_equal(y, M.row_words([M.quotient_points(f, zs)[1] for f, zs in zip(polys, rows)]))
    c = prover.commit(polys)
    assert list(verifier.verify(c, rows, y, pi)) == [True, True]
    y[1, 2, 0] ^= 1
    assert list(verifier.verify(c, rows, y, pi)) == [True, False]
    with pytest.raises(ValueError):
        api.KzgPointsVerifier(api.G1Affine(srs[:8]), api.G2Affine(srs_g2[:8]))


def test_argument_errors_and_the_empty_batch(engine, srs, srs_g2):
    lib, st = engine.lib, engine.stream
    n, m, k = 12, 2, 3
    rng = random.Random(0xB6)
    fill = lambda *shape: engine.to_device(np.full(shape, SENTINEL, dtype=np.uint64))
    flags = lambda count: engine.to_device(np.full(count, 7, dtype=np.uint8))
    dsrs, dg2 = engine.to_device_soa(srs[:n], 8), engine.to_device_soa(srs_g2[:k + 1], 16)
    dpolys = engine.to_device(np.ascontiguousarray(KP.poly_words([rand_poly(rng, n) for _ in range(m)]).transpose(0, 2, 1)))
    dz = engine.to_device_soa(M.row_words(rand_rows(rng, m, k)).reshape(m * k, 4), 4)
    dc = engine.to_device_soa(srs[:m], 8)
    out_a, out_q, out_y, out_pi, out_zp, out_rp = fill(4, m * k), fill(m, 4, n), fill(4, m * k), fill(8, m), fill(m, 4, k + 1), fill(m, 4, k)
    out_d, out_pi_inf, out_ok = flags(m), flags(m), flags(m)
    weights = lambda z=dz.ptr, kk=k, mm=m, a=out_a.ptr: lib.sylow_hip_kzg_points_weights_batch(z, kk, mm, a, out_d.ptr, st)
    quot = lambda co=dpolys.ptr, ln=n, mm=m, z=dz.ptr, kk=k, q=out_q.ptr, y=out_y.ptr: lib.sylow_hip_kzg_quotient_points_batch(co, ln, mm, z, kk, q, y, st)
    opn = lambda s=dsrs.ptr, ln=n, mm=m, kk=k, y=out_y.ptr, pf=out_pi_inf.ptr: lib.sylow_hip_kzg_open_points_batch(s, dpolys.ptr, ln, mm, dz.ptr, kk, y, out_pi.ptr, pf, st)
    pol = lambda z=dz.ptr, kk=k, nn=m, d=out_d.ptr: lib.sylow_hip_kzg_points_polys_batch(z, dz.ptr, kk, nn, out_zp.ptr, out_rp.ptr, d, st)
    ver = lambda g2=dg2.ptr, kk=k, nn=m, ok=out_ok.ptr: lib.sylow_hip_kzg_verify_points_batch(dsrs.ptr, g2, dc.ptr, None, dz.ptr, dz.ptr, kk, nn, dc.ptr, None, ok, st)
    for call in (weights, quot, opn, pol, ver):
        assert call(kk=0) == E_ARG and call(kk=KMAX + 1) == E_ARG
        assert b"bad argument" in lib.sylow_hip_last_error()
    assert weights(z=None) == E_ARG and weights(a=None) == E_ARG
    assert quot(co=None) == E_ARG and quot(z=None) == E_ARG and quot(q=None, y=None) == E_ARG and quot(ln=0) == E_ARG
    assert quot(q=dpolys.ptr) == E_ARG and quot(q=dpolys.ptr + 32 * n * m - 8) == E_ARG, "q_out overlapping coeffs"
    assert opn(s=None) == E_ARG and opn(y=None) == E_ARG and opn(pf=None) == E_ARG and opn(ln=0) == E_ARG
    assert pol(z=None) == E_ARG and pol(d=None) == E_ARG
    assert ver(g2=None) == E_ARG and ver(ok=None) == E_ARG
    # the empty batch: OK, nothing launched, nothing written, whatever the pointers are
    assert weights(mm=0) == 0 and quot(mm=0) == 0 and opn(mm=0) == 0 and pol(nn=0) == 0 and ver(nn=0) == 0
    assert lib.sylow_hip_kzg_points_weights_batch(None, k, 0, None, None, st) == 0
    assert lib.sylow_hip_kzg_quotient_points_batch(None, n, 0, None, k, None, None, st) == 0
    assert lib.sylow_hip_kzg_open_points_batch(None, None, n, 0, None, k, None, None, None, st) == 0
    assert lib.sylow_hip_kzg_points_polys_batch(None, None, k, 0, None, None, None, st) == 0
    assert lib.sylow_hip_kzg_verify_points_batch(None, None, None, None, None, None, k, 0, None, None, None, st) == 0
    engine.sync()
    for dev in (out_a, out_q, out_y, out_pi, out_zp, out_rp):
        assert (dev.download() == SENTINEL).all(), "nothing written"
    for dev in (out_d, out_pi_inf, out_ok):
        assert (dev.download() == 7).all(), "nothing written"
    empty = engine.kzg_quotient_points(np.zeros((0, n, 4), dtype=np.uint64), np.zeros((0, k, 4), dtype=np.uint64))
    assert empty[0].shape == (0, n, 4) and empty[1].shape == (0, k, 4)
