"""GPU: PLONK's permutation grand product -- sylow_hip_plonk_identity_batch and sylow_hip_plonk_permutation_batch(_tuned) (fr_scan.hip) -- word
for word against the integer model of tests/fr_scan_model.py: z, z_n and the status of two instances with different (beta, gamma) over one
permutation; a satisfied mapping closes with status 0, one changed wire sets bit 1 in that instance alone, a denominator forced to 0 sets
bit 0; then z through the API into a KZG commitment that opens at x and w x to values that satisfy z(w x) den = z(x) num."""
import random

import numpy as np
import pytest

import fr_scan_model as M
import kzg_prove_model as KP
from groth16_model import ints, limbs

pytestmark = pytest.mark.gpu
R = M.R
K = M.plan_constants()
CH, WIRES_MAX = K["SCAN_CHUNK"], K["PLONK_WIRES_MAX"]
LOG_CH = CH.bit_length() - 1
TAU = 0x1F3A5C7E9B2D4F6081A3C5E7092B4D6F8A1C3E507294B6D8FA1C3E5072940B6D % R
SHIFTS = [1] + [pow(5, j, R) * 7 % R for j in range(1, WIRES_MAX)]          # representatives of distinct cosets of every domain up to 2^28, whp


def words(rows):
    """nested lists of ints [..][n] -> [.., n, 4] words"""
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


def instance(rng, n_wires, log_n):
    n = 1 << log_n
    mapping = list(range(n_wires * n))
    rng.shuffle(mapping)
    shifts = SHIFTS[:n_wires]
    return shifts, mapping, M.sigma_from_mapping(shifts, log_n, mapping), M.satisfying_wires(mapping, n_wires, log_n, rng)


def test_identity_columns_are_the_transform_s_root(engine):
    for log_n, n_wires in ((0, 1), (1, 3), (3, 2), (9, 3), (LOG_CH + 1, WIRES_MAX)):
        got = engine.plonk_identity(limbs([s + R for s in SHIFTS[:n_wires]]), log_n)
        assert np.array_equal(got, words(M.identity(SHIFTS[:n_wires], log_n))), (log_n, n_wires)
    # w is the root of fr_ntt: the transform of X is its values w^i
    log_n = 5
    x = limbs([0, 1] + [0] * ((1 << log_n) - 2))
    assert np.array_equal(engine.fr_ntt(x), engine.plonk_identity(limbs([1]), log_n)[0])


@pytest.mark.parametrize("n_wires", [1, 3, WIRES_MAX])
@pytest.mark.parametrize("log_n", [0, 1, 3, LOG_CH, LOG_CH + 1])
def test_z_and_status_against_the_model(engine, log_n, n_wires):
    rng = random.Random(0x9100 + 64 * log_n + n_wires)
    n = 1 << log_n
    shifts, mapping, sigma, good = instance(rng, n_wires, log_n)
    bad = [list(col) for col in good]
    long = [c for c in M.cycles(mapping) if len(c) >= 2]
    if long:
        p = long[0][-1]
        bad[p // n][p % n] = (bad[p // n][p % n] + 1) % R
    beta, gamma = [rng.randrange(R), rng.randrange(1 << 256)], [rng.randrange(1 << 256), rng.randrange(R)]
    z, total, status = engine.plonk_permutation(words([good, bad]), words(sigma), limbs(shifts), limbs(beta), limbs(gamma))
    for j, wires in enumerate((good, bad)):
        want, want_total, want_status = M.permutation(wires, sigma, shifts, beta[j] % R, gamma[j] % R, log_n)
        assert np.array_equal(z[j], limbs(want)) and np.array_equal(total[j], limbs([want_total])[0]) and status[j] == want_status, (log_n, n_wires, j)
    assert list(status) == [0, 2 if long else 0], "a satisfied mapping closes; one changed wire sets bit 1 in that instance alone"
    assert ints(z[:, 0]) == [1, 1] and ints(total[:1]) == [1]
    if log_n == LOG_CH + 1 and n_wires == 3:
        pinned = engine.plonk_permutation(words([good, bad]), words(sigma), limbs(shifts), limbs(beta), limbs(gamma), max_blocks=1, totals_tile=1)
        assert all(np.array_equal(x, y) for x, y in zip(pinned, (z, total, status))), "the words depend on neither pin"


def test_a_denominator_forced_to_zero_sets_bit_0(engine):
    rng = random.Random(0x9101)
    log_n, n_wires = 3, 3
    shifts, mapping, sigma, wires = instance(rng, n_wires, log_n)
    beta = [rng.randrange(R), rng.randrange(R)]
    gamma = [rng.randrange(R), -(wires[2][5] + beta[1] * sigma[2][5]) % R]
    z, total, status = engine.plonk_permutation(words([wires, wires]), words(sigma), limbs(shifts), limbs(beta), limbs(gamma))
    assert status[0] == 0 and status[1] & 1 and not z[1, 6:].any() and not total[1].any()
    for j in range(2):
        want, want_total, want_status = M.permutation(wires, sigma, shifts, beta[j], gamma[j], log_n)
        assert np.array_equal(z[j], limbs(want)) and np.array_equal(total[j], limbs([want_total])[0]) and status[j] == want_status


def test_api_grand_product_commits_and_opens(engine):
    from sylow_amd import api
    api.set_engine(engine)
    rng = random.Random(0x9102)
    log_n, n_wires = 3, 3
    n, w = 1 << log_n, M.omega(log_n)
    shifts, mapping, sigma, wires = instance(rng, n_wires, log_n)
    perm = api.PlonkPermutation.from_mapping(log_n, shifts, mapping)
    assert np.array_equal(perm.sigma, words(sigma))
    beta, gamma = rng.randrange(R), rng.randrange(R)
    z, status = perm.grand_product(words(wires), [beta], [gamma])
    want, _, _ = M.permutation(wires, sigma, shifts, beta, gamma, log_n)
    assert z.shape == (1, n, 4) and np.array_equal(z[0], limbs(want)) and list(status) == [0]
    mono, inf = engine.g1_generator_mul(limbs(KP.srs_logs(TAU, n)))
    assert not inf.any()
    prover = api.KzgProver(api.G1Affine(mono))
    c = prover.commit_evals(z)                                   # z goes straight in
    by_evals = prover.eval_prover()
    assert np.array_equal(c.xy, by_evals.commit(z).xy) and not c.infinity.any()
    # z(w x) den = z(x) num at the domain point x = w^i, both values through openings the verifier accepts
    i = 2
    xs = [pow(w, i, R), pow(w, i + 1, R)]
    y, pi = by_evals.open(np.concatenate([z, z]), xs)
    import groth16_model as G
    verifier = api.KzgVerifier(api.G2Affine(G.g2_gen_mul([TAU])[0]))
    cc = api.G1Affine(np.concatenate([c.xy, c.xy]), np.concatenate([c.infinity, c.infinity]))
    assert verifier.verify((cc, xs, y, pi)).all()
    num, den = M.terms(wires, sigma, shifts, beta, gamma, log_n)
    zx, zwx = ints(y)
    assert (zx, zwx) == (want[i], want[i + 1]) and zwx * den[i] % R == zx * num[i] % R
    with pytest.raises(ValueError):
        api.PlonkPermutation.from_mapping(log_n, shifts, [0] * (n_wires * n))
