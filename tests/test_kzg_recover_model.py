"""CPU: tests/kzg_recover_model.py, the model the GPU tests of the cell recovery compare against, checked against long-hand arithmetic: its
fast transform against the sums of the definition, the vanishing values against the expanded polynomial Z, the five steps against
Lagrange interpolation of the held values, and the three status cases."""
import random

import pytest

import kzg_recover_model as M
from kzg_recover_model import R

SMALL = [(1, 0), (2, 2), (3, 1), (3, 0), (1, 3)]


def blob(rng, log_c, log_l):
    n = 1 << (log_c + log_l)
    f = [rng.randrange(R) for _ in range(n // 2)] + [0] * (n // 2)
    return f, M.dft_slow(f, log_c + log_l)


def masks(rng, log_c):
    c = 1 << log_c
    out = [[1] * c]
    for k in sorted({1, c // 2} - {0}):
        miss = rng.sample(range(c), k)
        out.append([0 if i in miss else 1 for i in range(c)])
    out.append([0] * (c // 2) + [1] * (c - c // 2))
    out.append([i & 1 ^ 1 for i in range(c)] if c > 1 else [1])
    return out


def test_the_root_and_the_shift():
    assert M.omega(28) == 0x2A3C09F0A58A7E8500E0A7EB8EF62ABC402D111E41112ED49BD61B6E725B19F0
    assert pow(M.omega(28), 1 << 27, R) == R - 1
    for k in range(29):
        assert pow(M.S, 1 << k, R) != 1                                   # s^l v^k is never a power of v


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5])
def test_fast_transform_is_the_definition(log_n):
    rng = random.Random(log_n)
    a = [rng.randrange(R) for _ in range(1 << log_n)]
    for shift in (1, M.S, 12345):
        assert M.fft(a, log_n, False, shift) == M.dft_slow(a, log_n, shift)
        assert M.fft(a, log_n, True, shift) == M.idft_slow(a, log_n, shift)
        assert M.fft(M.fft(a, log_n, False, shift), log_n, True, shift) == a


@pytest.mark.parametrize("log_c,log_l", SMALL)
def test_vanishing_values(log_c, log_l):
    rng = random.Random(log_c * 8 + log_l)
    c = 1 << log_c
    for present in masks(rng, log_c):
        zd, zc, status = M.vanish(present, log_c, log_l)
        assert status == M.OK
        assert (zd, zc) == M.vanish_slow(present, log_c, log_l)
        assert [z == 0 for z in zd] == [not p for p in present]           # zero exactly on M
        assert all(zc)                                                    # never zero on the coset
    present = [0] * (c // 2 + 1) + [1] * (c - c // 2 - 1)
    assert M.vanish(present, log_c, log_l) == ([0] * c, [1] * c, M.TOO_FEW)


@pytest.mark.parametrize("log_c,log_l", SMALL)
def test_recover_against_interpolation_and_the_status_cases(log_c, log_l):
    rng = random.Random(100 + log_c * 8 + log_l)
    c, n = 1 << log_c, 1 << (log_c + log_l)
    f, y = blob(rng, log_c, log_l)
    for present in masks(rng, log_c):
        miss = M.missing(present)
        yy = [rng.randrange(1 << 256) if not present[j % c] else y[j] for j in range(n)]
        assert M.recover(yy, present, log_c, log_l) == (M.OK, f)
        assert M.recover_slow(yy, present, log_c, log_l) == (M.OK, f)
        held = [j for j in range(n) if present[j % c]]
        j = rng.choice(held)
        yy[j] = (yy[j] + 1) % R
        status, g = M.recover(yy, present, log_c, log_l)
        assert (status, g) == M.recover_slow(yy, present, log_c, log_l)
        if len(miss) < c // 2:
            assert status == M.INCONSISTENT and any(g[n // 2:])            # a changed value is detected
        else:                                                              # exactly half: every input is some blob's
            assert status == M.OK and g != f and not any(g[n // 2:])
            w = M.omega(log_c + log_l)
            assert g[:n // 2] == M.interpolate([pow(w, k, R) for k in held], [yy[k] for k in held])
    present = [0] * (c // 2 + 1) + [1] * (c - c // 2 - 1)
    assert M.recover(y, present, log_c, log_l) == (M.TOO_FEW, [0] * n)


def test_exactly_half_is_lagrange_interpolation():
    rng = random.Random(7)
    log_c, log_l = 2, 1
    f, y = blob(rng, log_c, log_l)
    present = [0, 1, 1, 0]
    xs = [x for i in (1, 2) for x in M.cell_points(i, log_c, log_l)]
    ys = [y[i + 4 * j] for i in (1, 2) for j in range(2)]
    assert M.interpolate(xs, ys) == f[:4]
    assert M.recover(y, present, log_c, log_l) == (M.OK, f)


def test_a_real_blob_runs_in_seconds():
    rng = random.Random(9)
    log_c, log_l = 7, 6
    n, c = 1 << 13, 1 << 7
    f = [rng.randrange(R) for _ in range(n // 2)] + [0] * (n // 2)
    y = M.fft(f, 13)
    miss = set(rng.sample(range(c), c // 2))
    present = [0 if i in miss else 1 for i in range(c)]
    assert M.recover([0 if j % c in miss else y[j] for j in range(n)], present, log_c, log_l) == (M.OK, f)
