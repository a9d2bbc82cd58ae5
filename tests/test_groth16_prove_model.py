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


# ---- what tests/test_gpu_groth16_prove_routes.py leans on --------------------------------------------------------------------------------
def test_a_free_key_s_proof_is_the_formula_written_out():
    ct, z = M.make_circuit(1, 2, 4, 1, seed=21)
    st = M.free_key(ct, seed=22)
    assert len(st.u) == len(st.v) == 4 and len(st.lq) == 2 and len(st.hq) == 1
    assert len(set(st.u + st.v + st.lq + st.hq)) == 11 and st.u != M.Setup(ct, seed=22).u, "independent values, not the circuit's"
    rng = random.Random(23)
    w = [1] + [rng.randrange(1 << 256) for _ in range(3)]            # unsatisfied, words past r
    r, s = rng.randrange(R), rng.randrange(R)
    a, b, c = st.proof_dlogs(w, r, s)
    h = M.quotient_coset(M.matvec(ct.a, [x % R for x in w], 2), M.matvec(ct.b, [x % R for x in w], 2), M.matvec(ct.c, [x % R for x in w], 2), 1)
    wa = (st.alpha + st.u[0] * w[0] + st.u[1] * w[1] + st.u[2] * w[2] + st.u[3] * w[3] + r * st.delta) % R
    wb = (st.beta + st.v[0] * w[0] + st.v[1] * w[1] + st.v[2] * w[2] + st.v[3] * w[3] + s * st.delta) % R
    wc = (st.lq[0] * w[2] + st.lq[1] * w[3] + st.hq[0] * h[0] + s * wa + r * wb - r * s * st.delta) % R
    assert (a, b, c) == (wa, wb, wc)


def test_witness_mix_holds_the_three_kinds_and_no_two_neighbours_alike():
    ct, z = M.make_circuit(3, 8, 7, 2, seed=31, free=2)
    z0 = M.zero_witness(ct)
    for m, planted in ((7, ()), (513, (7, 255, 300, 512))):
        zs = M.witness_mix(ct, z, m, seed=32, zero_rows=planted)
        assert len(zs) == m and all(len(w) == 7 and w[0] == 1 for w in zs) and all(zs[j] != zs[j + 1] for j in range(m - 1))
        kinds = [0 if w == z else 1 if w == z0 else 2 for w in zs]
        assert {0, 1, 2} == set(kinds) and all(kinds[j] == 1 for j in planted)
        assert all(ct.satisfied([v % R for v in w]) == (k != 2) for w, k in zip(zs, kinds))
        assert zs == M.witness_mix(ct, z, m, seed=32, zero_rows=planted)


def test_planted_randomness_makes_the_zero_witness_s_point_the_identity():
    ct, z = M.make_circuit(3, 8, 7, 2, seed=41, free=2)
    z0, rng = M.zero_witness(ct), random.Random(42)
    for st in (M.Setup(ct, seed=43), M.free_key(ct, seed=44)):
        assert st.proof_dlogs(z0, 0, 0)[2] == 0 and all(st.proof_dlogs(z0, 0, 0)[:2])
        for k, what in enumerate("ABC"):
            proof = st.proof_dlogs(z0, *M.planted_randomness(st, what, rng))
            assert [v == 0 for v in proof] == [k == j for j in range(3)], what
    st = M.Setup(ct, seed=43)                                        # under the circuit's own key such a proof still verifies
    assert all(st.verifies(st.proof_dlogs(z0, *M.planted_randomness(st, what, rng)), z0[1:3]) for what in "ABC")


def test_degenerate_circuits_no_private_variable_no_constraint_and_a_short_one():
    rng = random.Random(51)
    ct, z = M.make_circuit(2, 3, 4, 3, seed=52, free=0)              # every variable but z_0 is public
    st = M.Setup(ct, seed=53)
    assert len(st.lq) == 0 and len(st.ic) == 4 and st.verifies(st.proof_dlogs(z, rng.randrange(R), rng.randrange(R)), z[1:4])
    for log_n in (0, 1):                                             # no constraint: u = v = 0 and h = 0
        ct, z = M.make_circuit(log_n, 0, 3, 1, seed=54)
        st = M.Setup(ct, seed=55)
        assert ct.n_cons == 0 and not any(st.u) and not any(st.v) and not any(st.lq) and len(st.hq) == (1 << log_n) - 1
        r, s = rng.randrange(R), rng.randrange(R)
        a, b, c = st.proof_dlogs(z, r, s)
        assert a == (st.alpha + r * st.delta) % R and b == (st.beta + s * st.delta) % R and st.verifies((a, b, c), z[1:2])
    ct, z = M.make_circuit(3, 5, 7, 2, seed=56)                      # three padding rows
    st = M.Setup(ct, seed=57)
    assert st.verifies(st.proof_dlogs(z, 1, 2), z[1:3])
    w = [1] + [rng.randrange(1 << 256) for _ in range(6)]
    assert not ct.satisfied([v % R for v in w]) and not st.verifies(st.proof_dlogs(w, 1, 2), w[1:3])


def test_the_sparse_product_s_accumulator_holds_27_products_and_not_28():
    """what makes rows of 28 and 29 entries per lane the ones that matter: 16 products between two folds are far inside 512 bits, 28 are not"""
    top = (R - 1) ** 2
    assert 27 * top < 1 << 512 <= 28 * top and top % R == 1
    assert (R - 1) + 16 * top < 1 << 512, "a fold's residue and SPMV_FLUSH products more"
