"""CPU: the model of the G1 transform (tests/g1_ntt_model.py) against independent definitions -- the inverse transform of the monomial SRS's
logarithms tau^k is the Lagrange basis at tau (tests/kzg_evals_model.py, a closed formula that knows no transform), the stage-by-stage
Stockham addressing of g1_ntt.hip with its skipped unit twiddles reproduces the O(n^2) definition, and the products it makes are as many as
the plan's formula says."""
import random

import pytest

import g1_ntt_model as M
import kzg_evals_model as E
import ntt_model as N
from ntt_model import R

TAU = 0x2B1D0C5A7E3B92F4861C0DE5EED0FACADE0123456789ABCDEF0FEDCBA98765432 % R


@pytest.mark.parametrize("log_n", range(7))
def test_inverse_of_the_monomial_logs_is_the_lagrange_basis(log_n):
    n = 1 << log_n
    want = E.lagrange_at(log_n, TAU)
    assert M.logs_ntt(M.monomial_logs(TAU, n), log_n, inverse=True) == want
    assert M.logs_ntt(M.monomial_logs(TAU, n), log_n, inverse=True, direct=True) == want
    assert M.logs_ntt(want, log_n) == M.monomial_logs(TAU, n)        # and forward again
    assert sum(want) % R == 1                                         # the basis sums to one


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("log_n", range(8))
def test_stockham_stages_with_the_skip_are_the_definition(log_n, inverse):
    rng = random.Random(0x61 + 2 * log_n + inverse)
    s = [rng.randrange(R) for _ in range(1 << log_n)]
    got, made = M.stockham(s, log_n, inverse)
    assert got == N.ntt_direct(s, log_n, inverse=inverse)
    assert made == M.multiplications(log_n)


def test_multiplication_count_matches_the_plan_header():
    """the header's loop, read from the source, is the formula; and its closed form (n/2)(log_n - 2) + 1 for log_n >= 1"""
    src = open(M.PLAN).read()
    assert "for (int p = 1; p < log_n; ++p) s += half(log_n) - (half(log_n) >> p);" in src
    assert M.multiplications(0) == 0 and M.multiplications(1) == 0 and M.multiplications(2) == 1 and M.multiplications(3) == 5
    for log_n in range(1, 29):
        assert M.multiplications(log_n) == (1 << (log_n - 1)) * (log_n - 2) + 1
    k = M.plan_constants()
    assert k["G1_NTT_BLOCK"] == 256 and k["G1_NTT_GRID_DEFAULT"] == 512 and k["G1_NTT_TABLE_BYTES_PER_LANE"] == 1024
