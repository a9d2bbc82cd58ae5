"""Big-integer restatement of the two Fp routines whose running time depends on their input, and the inputs that drive their tails.

fp_is_square (bn254_hash.hpp) is the binary Jacobi symbol, at most 508 steps in blocks of 4, narrowing from 8 limbs to 1, every exit a
wavefront-wide vote.  fp_inv (bn254_f29.hpp) is safegcd: 20 batches of 30 divsteps, left early once g = 0 in every lane, not before
batch 16.  Both iterate on the Montgomery representative a = x 2^256 mod p of the value x the caller passes, so a value with structure
(a power of two, a small number) reaches them as an ordinary 254-bit word.  This module steers by REPRESENTATIVE: rep_to_value(a) is
the value to pass so that the kernel iterates on a.  The step rules below are the ones the kernels' comments state, on Python integers:
no limbs, no masks.

Counts, as tests/test_tail_model.py prints them (pytest -s) and asserts their bounds:

  input, as the kernel sees it                        Jacobi steps                          divsteps until g = 0
  5000 random                                         319 .. 398                            497 .. 527, 1729 at or below 510
  2^b as a VALUE, b = 1..253 (the older test)         257 .. 381                            -
  representative 2^b, b = 200..253                    454 .. 507 (2^253: exactly 507)       -
  representative p - 2^b, b = 1..253                  255 .. 506                            -
  representative 1                                    254                                   512
  representatives of 1..8 random limbs (2400)         259 .. 384                            499 .. 523
  the 1267 structured representatives                 0 (zero), 254 .. 507;                 0 (zero), 498 .. 524
                                                      317 above 401, 23 at or above 500
  the whole family (3667)                             317 above 401                         1513 at or below 510 (zero left out),
                                                                                            2153 at or above 511

Limits.  No input is known that keeps g alive into safegcd's batches 19 and 20 (more than 540 divsteps): the maximum here is 527 at
random and 524 in the family, and this module does not search for one.  The count of steps is a property of the input; which block or batch a wavefront left its loop at
cannot be observed from outside the kernel.
"""
import functools
import random

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R_ORDER = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
RINV = pow(1 << 256, -1, P)
SEED = 0x7A11


def rep_to_value(a):
    """the value x with x 2^256 = a mod p: load_fp hands the kernel a when the caller passes x"""
    return a * RINV % P


def value_to_rep(x):
    return (x << 256) % P


def jacobi_binary(a):
    """(is_square, steps) for the representative a, 0 <= a < p.  n = p is odd throughout.  A step halves an even a, and the sign flips
    when n = 3, 5 mod 8; for an odd a it first orders the pair (a flip when both are 3 mod 4) and subtracts, which leaves an even a to
    halve.  Steps are counted until a = 0; then n is the gcd, 1 unless a was 0 from the start, and zero counts as a square."""
    assert 0 <= a < P
    n, flips, steps = P, 0, 0
    while a:
        if a & 1:
            if a < n:
                flips ^= (a & 3 == 3) and (n & 3 == 3)
                a, n = n, a
            a -= n
        flips ^= n & 7 in (3, 5)
        a >>= 1
        steps += 1
    return (n != 1 or not flips), steps


def divsteps_needed(g):
    """divsteps until g = 0 from (zeta, f, g) = (-1, p, g), the half-delta start, with the three branches of tools/safegcd_model.py:
    zeta < 0 and g odd: (-zeta - 2, g, (g - f) / 2); g odd: (zeta - 1, f, (g + f) / 2); g even: (zeta - 1, f, g / 2)"""
    assert 0 <= g < P
    zeta, f, steps = -1, P, 0
    while g:
        if g & 1:
            if zeta < 0:
                zeta, f, g = -zeta - 2, g, (g - f) >> 1
            else:
                zeta, g = zeta - 1, (g + f) >> 1
        else:
            zeta, g = zeta - 1, g >> 1
        steps += 1
        assert steps <= 600
    return steps


def _unique(xs):
    return list(dict.fromkeys(xs))


def sparse(m, top=253):
    """the sparse words modulo m: the small ones, the ends, the halves, and around every power of two"""
    out = [0, 1, 2, 3, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2]
    for b in range(1, top + 1):
        out += [1 << b, (1 << b) - 1, (1 << b) + 1, m - (1 << b)]
        if 3 << b < m:
            out.append(3 << b)
    return _unique(out)


@functools.lru_cache(maxsize=None)
def families():
    """(structured, by_limbs): the structured representatives, without repeats, and for nl = 1..8 a list of 300 seeded random
    representatives of exactly nl 32-bit limbs (the top one non-zero)"""
    rnd = random.Random(SEED)
    by_limbs = {}
    for nl in range(1, 9):
        out = []
        while len(out) < 300:
            v = rnd.getrandbits(32 * nl)
            if v >> (32 * (nl - 1)) and v < P:
                out.append(v)
        by_limbs[nl] = tuple(out)
    return tuple(sparse(P)), by_limbs


@functools.lru_cache(maxsize=None)
def family():
    """every member once, structured first"""
    structured, by_limbs = families()
    return tuple(_unique(list(structured) + [v for nl in range(1, 9) for v in by_limbs[nl]]))


@functools.lru_cache(maxsize=None)
def jacobi_steps():
    """{representative: steps} over the family"""
    return {a: jacobi_binary(a)[1] for a in family()}


@functools.lru_cache(maxsize=None)
def divsteps():
    """{representative: divsteps until g = 0} over the family"""
    return {a: divsteps_needed(a) for a in family()}


def fr_sparse():
    """Fr is kept canonical, so the value is what the inversion iterates on: the sparse words modulo r, zero left out"""
    r = R_ORDER
    out = [1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2]
    for b in range(1, 254):
        out += [1 << b, (1 << b) - 1, (1 << b) + 1, r - (1 << b)]
    return _unique(out)


# How the kernels of runtime.hip map element index to lane (blocks are 256 threads, a multiple of the 64-lane wavefront):
#   k_fp_sqrt (fp_sqrt_batch, fp_is_square_batch), k_f29_hook, k_svdw_map: thread t handles element t, so elements 64 w .. 64 w + 63 are
#       wavefront w, element 64 w + l its lane l                                                                        -> "thread"
#   k_fp_unop<OP_INV> (fp_inv_batch): thread t handles elements 2 t and 2 t + 1, one after the other, for even and for odd n alike.  A
#       wavefront covers 128 consecutive elements and calls fp_inv twice: on its 64 even elements, lane l holding element 128 w + 2 l,
#       then on its 64 odd ones                                                                                         -> "pair"
LANES = 64


def wavefronts(runs, mapping, tail=()):
    """One flat list of elements in which every run of 64 is one wavefront-wide call under `mapping` ("thread" or "pair"), lane l of
    the call holding run[l].  tail: fewer than 64 (thread) or 128 (pair) further elements, the ragged last wavefront.  Under "pair" an
    odd number of runs is completed by a second copy of the last one, so that no call mixes two runs."""
    runs = [list(r) for r in runs]
    assert all(len(r) == LANES for r in runs)
    if mapping == "thread":
        assert len(tail) < LANES
        out = [x for r in runs for x in r]
    else:
        assert mapping == "pair" and len(tail) < 2 * LANES
        if len(runs) % 2:
            runs.append(runs[-1])
        out = []
        for even, odd in zip(runs[0::2], runs[1::2]):
            for l in range(LANES):
                out += [even[l], odd[l]]
    return out + list(tail)


def run_of(pool, lanes=LANES):
    """`lanes` elements drawn round-robin from a non-empty pool"""
    pool = list(pool)
    assert pool
    return [pool[i % len(pool)] for i in range(lanes)]
