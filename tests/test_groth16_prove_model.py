"""CPU: the Groth16 prover's model (tests/groth16_prove_model.py) against itself -- the coset route is exact polynomial division, the proof's
discrete logarithms satisfy the verification equation, and the generated table of (5^(2^k) - 1)^-1 is what pow gives."""
import os
import random
import re

import pytest

import groth16_prove_model as M
import ntt_model as N

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("log_n", range(6))
def test_coset_route_is_exact_division(log_n):
    rng = random.Random(100 + log_n)
    n = 1 << log_n
    a, b = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
    c = [x * y % R for x, y in zip(a, b)]
    h, rem = M.quotient_exact(a, b, c, log_n)
    assert rem == [0] * n and len(h) == n and h[n - 1] == 0
    assert M.quotient_coset(a, b, c, log_n) == h
    # the division is the definition of a quotient: a b - c = h (X^n - 1) as polynomials, checked at a point off the domain
    x = rng.randrange(R)
    ev = lambda f: sum(v * pow(x, k, R) for k, v in enumerate(f)) % R
    fa, fb, fc = (N.ntt_radix2(v, log_n, inverse=True) for v in (a, b, c))
    assert (ev(fa) * ev(fb) - ev(fc)) % R == ev(h) * (pow(x, n, R) - 1) % R


def test_transform_product_is_the_schoolbook_product():
    rng = random.Random(7)
    f, g = [rng.randrange(R) for _ in range(128)], [rng.randrange(R) for _ in range(128)]
    want = [0] * 256
    for i, x in enumerate(f):
        for j, y in enumerate(g):
            want[i + j] = (want[i + j] + x * y) % R
    assert M.poly_mul(f, g) == want


def test_unsatisfied_input_has_a_remainder_and_the_coset_route_still_interpolates():
    log_n, rng = 3, random.Random(5)
    n = 1 << log_n
    a, b, c = ([rng.randrange(R) for _ in range(n)] for _ in range(3))
    _, rem = M.quotient_exact(a, b, c, log_n)
    assert any(rem)
    h = M.quotient_coset(a, b, c, log_n)
    ca, cb, cc = (N.ntt_radix2(N.ntt_radix2(v, log_n, inverse=True), log_n, shift=M.SHIFT) for v in (a, b, c))
    ch = N.ntt_radix2(h, log_n, shift=M.SHIFT)
    zh = (pow(M.SHIFT, n, R) - 1) % R
    assert all((x * y - w) % R == v * zh % R for x, y, w, v in zip(ca, cb, cc, ch))


@pytest.mark.parametrize("shape", [(0, 1, 3, 1), (3, 8, 7, 2), (6, 64, 50, 3), (4, 14, 20, 4)])
def test_proof_logarithms_satisfy_the_verification_equation(shape):
    log_n, n_cons, n_vars, l = shape
    ct, z = M.make_circuit(log_n, n_cons, n_vars, l, seed=sum(shape))
    st = M.Setup(ct, seed=11)
    rng = random.Random(3)
    for r, s in ((0, 0), (rng.randrange(R), rng.randrange(R)), (R + 1, (1 << 256) - 1)):
        proof = st.proof_dlogs(z, r, s)
        assert st.verifies(proof, z[1:l + 1])
        assert not st.verifies(proof, [z[1] + 1] + z[2:l + 1])
    # the exact quotient and the coset route give the same proof
    h, rem = M.quotient_exact(M.matvec(ct.a, z, ct.n), M.matvec(ct.b, z, ct.n), M.matvec(ct.c, z, ct.n), log_n)
    assert not any(rem) and st.proof_dlogs(z, 5, 6, h=h) == st.proof_dlogs(z, 5, 6)
    # a free variable may take any value; the witness that is zero but for z_0 satisfies the circuit; a broken one does not verify
    z2 = z[:-1] + [(z[-1] + 1) % R]
    assert ct.satisfied(z2) and st.verifies(st.proof_dlogs(z2, 1, 2), z2[1:l + 1])
    z0 = [1] + [0] * (n_vars - 1)
    assert st.verifies(st.proof_dlogs(z0, 3, 4), z0[1:l + 1])
    bad = list(z)
    bad[l + 1] = (bad[l + 1] + 1) % R
    if not ct.satisfied(bad):
        assert not st.verifies(st.proof_dlogs(bad, 1, 2), bad[1:l + 1])


def test_generated_zinv_table_is_what_pow_gives():
    text = open(os.path.join(ROOT, "sylow_amd", "csrc", "bn254_groth16_zinv.hpp")).read()
    rows = re.findall(r"\{(0x[0-9a-f]+ull), (0x[0-9a-f]+ull), (0x[0-9a-f]+ull), (0x[0-9a-f]+ull)\}", text)
    assert len(rows) == 29
    for k, row in enumerate(rows):
        value = sum(int(w[:-3], 16) << (64 * i) for i, w in enumerate(row))
        zh = (pow(5, 1 << k, R) - 1) % R
        assert zh != 0 and value == pow(zh, R - 2, R) == M.zinv(k) and value * zh % R == 1
