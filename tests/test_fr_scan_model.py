"""CPU: the model of the scans over Fr and of PLONK's permutation grand product (tests/fr_scan_model.py) against itertools.accumulate and
pow(v, -1, R), and on the fact that makes the feature meaningful: for a random permutation of the positions of a W x n table and random beta
and gamma, z closes to 1 when the wires are constant on every cycle, and does not close once one wire value on a cycle of length >= 2 is
changed."""
import itertools
import operator
import random

import fr_scan_model as M
import kzg_evals_model as E

R = M.R


def test_plan_constants_are_the_chunk_of_the_shared_inversion():
    c, e = M.plan_constants(), E.plan_constants()
    assert (c["SCAN_BLOCK"], c["SCAN_LANE_ELEMS"], c["SCAN_CHUNK"]) == (e["EVALS_BLOCK"], e["EVALS_LANE_ELEMS"], e["EVALS_CHUNK"])
    assert 1 <= c["SCAN_TOTALS_TILE_DEFAULT"] <= c["SCAN_TOTALS_TILE_MAX"] <= c["SCAN_BLOCK"]
    assert c["PLONK_WIRES_MAX"] == 32 and c["PLONK_LOG_N_MAX"] == 28 and M.omega(5) == E.omega(5) and M.R == E.R


def test_scan_is_accumulate():
    rng = random.Random(0x5CA9)
    a = [rng.randrange(1 << 256) for _ in range(37)] + E.EDGE_WORDS
    red = [v % R for v in a]
    for op, fn, e in ((M.SUM, lambda x, y: (x + y) % R, 0), (M.PRODUCT, lambda x, y: x * y % R, 1)):
        inc = list(itertools.accumulate(red, fn))
        assert M.scan(a, op) == (inc, inc[-1])
        assert M.scan(a, op, exclusive=True) == ([e] + inc[:-1], inc[-1])
    assert M.scan([], M.PRODUCT) == ([], 1) and M.scan([], M.SUM, True) == ([], 0)
    assert M.scan([R + 2], M.PRODUCT, True) == ([1], 2)


def test_ratio_scan_is_accumulate_over_pow():
    rng = random.Random(0x7A71)
    num = [rng.randrange(1 << 256) for _ in range(29)]
    den = [rng.randrange(1, R) + R * rng.randrange(2) for _ in range(29)]
    t = [n % R * pow(d, -1, R) % R for n, d in zip(num, den)]
    for op, fn, e in ((M.SUM, operator.add, 0), (M.PRODUCT, operator.mul, 1)):
        inc = [v % R for v in itertools.accumulate(t, fn)]
        assert M.ratio_scan(num, den, op) == ([e] + inc[:-1], inc[-1], 0)
    ones = M.ratio_scan(None, den, M.PRODUCT)
    assert ones == M.ratio_scan([1] * 29, den, M.PRODUCT) and ones[1] == pow(M.scan(den, M.PRODUCT)[1], -1, R)
    # a zero denominator: its own term is 0 and nobody else's moves
    den[11] = 2 * R
    out, total, status = M.ratio_scan(num, den, M.PRODUCT)
    clean = M.ratio_scan(num[:11], den[:11], M.PRODUCT)
    assert status == 1 and out[:11] == clean[0] and out[11] == clean[1] and not any(out[12:]) and total == 0
    out, total, status = M.ratio_scan(num, den, M.SUM)
    assert status == 1 and total == (sum(t) - t[11]) % R and out[12] == out[11]


def test_identity_columns_are_cosets_of_the_domain():
    cols = M.identity([1, 5, R + 7], 3)
    w = M.omega(3)
    assert [c[0] for c in cols] == [1, 5, 7] and all(c[i + 1] == c[i] * w % R for c in cols for i in range(7))
    assert len({v for c in cols for v in c}) == 24 and pow(w, 8, R) == 1 and pow(w, 4, R) != 1
    assert M.identity([3], 0) == [[3]]


def test_z_closes_exactly_when_the_wires_are_constant_on_every_cycle():
    rng = random.Random(0x910C)
    for n_wires, log_n in ((1, 3), (3, 3), (4, 2), (2, 0)):
        n, shifts = 1 << log_n, [1, 5, 7, 10][:n_wires]
        mapping = list(range(n_wires * n))
        rng.shuffle(mapping)
        sigma = M.sigma_from_mapping(shifts, log_n, mapping)
        wires = M.satisfying_wires(mapping, n_wires, log_n, rng)
        beta, gamma = rng.randrange(R), rng.randrange(R)
        z, total, status = M.permutation(wires, sigma, shifts, beta, gamma, log_n)
        assert z[0] == 1 and total == 1 and status == 0
        num, den = M.terms(wires, sigma, shifts, beta, gamma, log_n)
        assert all(z[i + 1] * den[i] % R == z[i] * num[i] % R for i in range(n - 1)) and total * den[-1] % R == z[-1] * num[-1] % R
        long = [c for c in M.cycles(mapping) if len(c) >= 2]
        if not long:
            continue
        p = long[0][0]
        wires[p // n][p % n] = (wires[p // n][p % n] + 1) % R
        z, total, status = M.permutation(wires, sigma, shifts, beta, gamma, log_n)
        assert total != 1 and status == 2
    # the identity permutation closes for any wires
    wires = [[rng.randrange(R) for _ in range(8)] for _ in range(3)]
    assert M.permutation(wires, M.identity([1, 5, 7], 3), [1, 5, 7], 11, 13, 3)[1:] == (1, 0)


def test_a_forced_zero_denominator_sets_bit_0():
    rng = random.Random(0xDE20)
    shifts, log_n = [1, 5], 2
    mapping = [1, 0, 3, 2, 5, 4, 7, 6]
    sigma = M.sigma_from_mapping(shifts, log_n, mapping)
    wires = M.satisfying_wires(mapping, 2, log_n, rng)
    beta = rng.randrange(R)
    gamma = -(wires[1][2] + beta * sigma[1][2]) % R
    z, total, status = M.permutation(wires, sigma, shifts, beta, gamma, log_n)
    assert status & 1 and z[3] == 0 and total == 0 and status == 3
