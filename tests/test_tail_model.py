"""CPU: tests/tail_model.py against Euler's criterion and tools/safegcd_model.py, and the conditions the GPU tests of
tests/test_gpu_tails.py rely on: that the family holds the long Jacobi tails and both sides of safegcd's early exits.  Run with -s to
print the counts quoted in tail_model's docstring."""
import os
import random
import sys

import pytest

import tail_model as T
from tail_model import P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import safegcd_model as S  # noqa: E402


def euler(v):
    return pow(v, (P - 1) // 2, P) in (0, 1)


def span(xs):
    xs = list(xs)
    return f"{min(xs)} .. {max(xs)}"


@pytest.fixture(scope="module")
def randoms():
    rnd = random.Random(T.SEED + 1)
    return [rnd.randrange(P) for _ in range(5000)]


def test_rep_to_value_round_trip():
    for a in (0, 1, 2, P - 1, 1 << 253, 0xDEADBEEF):
        assert T.value_to_rep(T.rep_to_value(a)) == a and 0 <= T.rep_to_value(a) < P
    assert T.rep_to_value((1 << 256) % P) == 1


def test_jacobi_binary_is_eulers_criterion(randoms):
    """on the representative and on the value alike: 2^256 is a square"""
    for a in list(T.family()) + randoms:
        sq, steps = T.jacobi_binary(a)
        assert sq == euler(a), hex(a)
        assert 0 <= steps <= 507
    assert all(euler(a) == euler(T.rep_to_value(a)) for a in randoms[:200])
    assert T.jacobi_binary(0) == (True, 0)


def test_jacobi_tails_are_in_the_family(randoms):
    steps = T.jacobi_steps()
    structured, by_limbs = T.families()
    assert steps[1 << 253] == 507 and steps[1] == 254
    assert max(steps.values()) == 507                                    # one step inside the kernel's bound of 508
    assert sum(1 for a in T.family() if steps[a] > 401) >= 200
    assert sum(1 for a in T.family() if steps[a] >= 500) >= 8            # a wavefront of them repeats none more than 8 times
    rs = [T.jacobi_binary(a)[1] for a in randoms]
    assert max(rs) <= 420                                                # chance does not reach the tail: that is why the family exists
    print()
    print("jacobi steps: 5000 random", span(rs))
    print("  2^b as a value, b = 1..253", span(T.jacobi_binary(T.value_to_rep(1 << b))[1] for b in range(1, 254)))
    print("  representative 2^b, b = 200..253", span(steps[1 << b] for b in range(200, 254)), "2^253:", steps[1 << 253])
    print("  representative p - 2^b", span(steps[P - (1 << b)] for b in range(1, 254)))
    print("  representative 1:", steps[1])
    print("  1..8 random limbs", span(steps[a] for nl in by_limbs for a in by_limbs[nl]))
    nz = [steps[a] for a in structured if a]
    print(f"  {len(structured)} structured: non-zero", span(nz), "above 401:", sum(s > 401 for s in nz), "at or above 500:", sum(s >= 500 for s in nz))
    print(f"  family of {len(T.family())}: above 401:", sum(1 for a in T.family() if steps[a] > 401))


def test_safegcd_model_inverts_the_family_with_its_assertions_live():
    if not __debug__:
        pytest.fail("run without -O: the model's assertions are the test")
    for a in T.family():
        if a:
            assert S.modinv(a) == pow(a, P - 2, P), hex(a)
    assert S.modinv(0) == 0


def test_divsteps_both_sides_of_the_early_exits(randoms):
    """the kernel leaves before batch 18 only when all 64 lanes have g = 0 after 510 divsteps: the family has enough of both kinds"""
    ds = T.divsteps()
    structured, by_limbs = T.families()
    fast = [a for a in T.family() if a and ds[a] <= 510]
    slow = [a for a in T.family() if ds[a] >= 511]
    assert len(fast) >= 300 and len(slow) >= 300
    assert sum(1 for a in T.family() if ds[a] >= 520) >= 2
    assert max(ds.values()) <= 590 and ds[0] == 0
    rs = [T.divsteps_needed(a) for a in randoms]
    print()
    print("divsteps: 5000 random", span(rs), "at or below 510:", sum(s <= 510 for s in rs))
    print("  representative 1:", ds[1])
    print("  1..8 random limbs", span(ds[a] for nl in by_limbs for a in by_limbs[nl]))
    print(f"  {len(structured)} structured: non-zero", span(ds[a] for a in structured if a))
    print(f"  family of {len(T.family())}: at or below 510 (zero left out): {len(fast)}, at or above 511: {len(slow)}, maximum {max(ds.values())}")


def test_divsteps_needed_is_the_batch_the_model_reaches_zero_in():
    """the count agrees with the limb model: g is non-zero before batch ceil(steps / 30) and zero after it"""
    ds = T.divsteps()
    for a in list(T.family())[::37] + [1, 1 << 253, P - 1]:
        f, g, zeta = list(S.PL), S.to30(a), -1
        d, e = [0] * 9, [1] + [0] * 8
        for it in range(20):
            assert (S.val(g) != 0) == (30 * it < ds[a]), (hex(a), it)
            zeta, t = S.divsteps_30(zeta, f[0], g[0])
            d, e = S.update_de(d, e, t)
            f, g = S.update_fg(f, g, t)


def test_wavefront_layouts():
    runs = [[(r, l) for l in range(64)] for r in range(3)]
    flat = T.wavefronts(runs, "thread", tail=["t"] * 5)
    assert len(flat) == 197 and all(flat[64 * r + l] == (r, l) for r in range(3) for l in range(64)) and flat[192:] == ["t"] * 5
    flat = T.wavefronts(runs, "pair", tail=["t"] * 65)
    assert len(flat) == 4 * 64 + 65
    for l in range(64):                                              # thread t = 64 w + l: elements 2 t and 2 t + 1
        assert flat[2 * l] == (0, l) and flat[2 * l + 1] == (1, l)
        assert flat[128 + 2 * l] == (2, l) and flat[128 + 2 * l + 1] == (2, l)
    assert T.run_of([1, 2, 3], 7) == [1, 2, 3, 1, 2, 3, 1]


def test_fr_sparse_is_canonical_and_non_zero():
    xs = T.fr_sparse()
    assert len(set(xs)) == len(xs) and all(0 < x < T.R_ORDER for x in xs)
