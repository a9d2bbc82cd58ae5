"""GPU: the Lagrange-basis KZG SRS from the monomial one -- sylow_hip_kzg_srs_lagrange (g1_ntt.hip) and KzgProver.lagrange_srs / eval_prover --
against the closed formula L_i(tau) of tests/kzg_evals_model.py through the oracle's fixed-base product, and as a prover: what
KzgProver(srs).eval_prover() commits and opens from values is word for word what KzgProver commits and opens from the interpolated
coefficients under the monomial SRS, and KzgVerifier accepts it.  A tau inside the domain gives an SRS with identities: flagged, and refused
by the Python layer."""
import random

import numpy as np
import pytest

import groth16_model as G
import kzg_evals_model as E
import kzg_prove_model as KP
from groth16_model import ints, limbs
from kzg_evals_model import R

pytestmark = pytest.mark.gpu
TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R
IDENTITY = limbs([0, 1]).reshape(8)
G1_GEN = limbs([1, 2]).reshape(8)
_SRS = {}


def monomial(log_n):
    if log_n not in _SRS:
        _SRS[log_n] = KP.srs_points(TAU, 1 << log_n)
    return _SRS[log_n]


@pytest.mark.parametrize("log_n", [0, 3, 6])
def test_against_the_closed_formula(engine, log_n):
    xy, inf = engine.kzg_srs_lagrange(monomial(log_n))
    wxy, winf = G.g1_gen_mul(E.lagrange_at(log_n, TAU))
    assert not winf.any() and not inf.any() and inf.shape == (1 << log_n,)
    assert np.array_equal(xy, wxy), f"points {list(np.flatnonzero((xy != wxy).any(axis=1)))[:8]} differ"
    # the forward transform of the Lagrange SRS returns the monomial SRS
    back, binf = engine.g1_ntt(xy, None)
    assert np.array_equal(back, monomial(log_n)) and not binf.any()


@pytest.mark.parametrize("log_n", [3, 6])
def test_eval_prover_is_the_coefficient_prover(engine, log_n):
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0x5125 + log_n)
    n, w = 1 << log_n, E.omega(log_n)
    by_coeffs = api.KzgProver(api.G1Affine(monomial(log_n)))
    by_evals = by_coeffs.eval_prover()
    assert isinstance(by_evals, api.KzgEvalProver) and len(by_evals.srs_lagrange) == n
    evals = [[rng.randrange(1 << 256) for _ in range(n)], [R + 9] * n, [0] * n]            # a constant and the zero array among them
    words = KP.poly_words(evals)
    c, c_mono = by_evals.commit(evals), by_coeffs.commit_evals(evals)
    assert np.array_equal(c.xy, c_mono.xy) and np.array_equal(c.infinity, c_mono.infinity) and list(c.infinity) == [0, 0, 1]
    verifier = api.KzgVerifier(api.G2Affine(G.g2_gen_mul([TAU])[0]))
    for zs in ([rng.randrange(R) for _ in evals], [w] * len(evals)):                        # outside the domain, and at z = w^1
        assert all(E.hit_index(log_n, z) == (1 if z == w else None) for z in zs)
        y, pi = by_evals.open(evals, zs)
        wy, wpi = by_coeffs.open(api.intt(words), zs)
        assert np.array_equal(y, wy) and np.array_equal(pi.xy, wpi.xy) and np.array_equal(pi.infinity, wpi.infinity)
        assert list(pi.infinity) == [0, 1, 1] and ints(y)[1:] == [9, 0]
        assert verifier.verify((c, zs, y, pi)).all()
        assert not verifier.verify((c, zs, [(v + 1) % R for v in ints(y)], pi)).any()


def test_tau_inside_the_domain(engine):
    """tau = w_8^3: L_i(tau) is 1 at i = 3 and 0 elsewhere"""
    from sylow_amd import api
    api.set_engine(engine)
    srs = KP.srs_points(pow(E.omega(3), 3, R), 8)
    xy, inf = engine.kzg_srs_lagrange(srs)
    assert list(inf) == [1, 1, 1, 0, 1, 1, 1, 1]
    assert np.array_equal(xy[3], G1_GEN) and all(np.array_equal(xy[i], IDENTITY) for i in range(8) if i != 3)
    with pytest.raises(ValueError, match="tau lies in the domain"):
        api.KzgProver(api.G1Affine(srs)).lagrange_srs()
    with pytest.raises(ValueError, match="power of two"):
        api.KzgProver(api.G1Affine(srs[:6])).lagrange_srs()
