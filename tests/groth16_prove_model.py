"""A CPU model of the Groth16 prover on BN254.  Not collected by pytest, integers only plus the C oracle for points (through
tests/groth16_model.py's generator multiples), and it shares nothing with sylow_amd.

A circuit is an R1CS over Fr: rows of A, B, C as lists of (column, value); variable 0 is the constant 1, variables 1 .. l are public.  The
setup is made from KNOWN tau, alpha, beta, gamma, delta, so every key element is a generator multiple whose discrete logarithm is a value in
Fr (through the Lagrange values at tau), and so are the three points of a proof:

    A = alpha + sum_i z_i u_i(tau) + r delta            B = beta + sum_i z_i v_i(tau) + s delta
    C = sum_{i > l} z_i lq_i + sum_{k < n - 1} h_k hq_k + s A + r B - r s delta
    lq_i = (beta u_i + alpha v_i + w_i)(tau) / delta,   hq_k = tau^k (tau^n - 1) / delta,   IC_j = (beta u_j + alpha v_j + w_j)(tau) / gamma

with h = (a b - c) / (X^n - 1) by exact polynomial division.  They satisfy A B = alpha beta + vk_x gamma + C delta."""
import random

import ntt_model as N

R = N.R
SHIFT = 5
EDGE_WORDS = [0, 1, R - 1, R, R + 1, 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47, (1 << 256) - 1]     # 0, 1, r - 1, r, r + 1, p, 2^256 - 1


def inv(x):
    return pow(x % R, R - 2, R)


# ---- sparse matrices -----------------------------------------------------------------------------------------------------------------
def csr(rows):
    """rows: lists of (column, value) -> (row_ptr, col, val) as lists of ints"""
    row_ptr, col, val = [0], [], []
    for row in rows:
        for c, v in row:
            col.append(c)
            val.append(v)
        row_ptr.append(len(col))
    return row_ptr, col, val


def matvec(rows, z, n_out=None):
    """(M z)_i mod r, an entry whose column is past the vector contributing zero; padded with zeros to n_out"""
    out = [sum(v * z[c] for c, v in row if c < len(z)) % R for row in rows]
    return out + [0] * ((len(out) if n_out is None else n_out) - len(out))


class Circuit:
    def __init__(self, log_n, n_vars, l, a, b, c):
        self.log_n, self.n, self.n_vars, self.l, self.a, self.b, self.c = log_n, 1 << log_n, n_vars, l, a, b, c
        self.n_cons = len(a)
        assert len(b) == len(c) == self.n_cons <= self.n and l < n_vars

    def satisfied(self, z):
        return all(x * y % R == w for x, y, w in zip(matvec(self.a, z), matvec(self.b, z), matvec(self.c, z)))


def make_circuit(log_n, n_cons, n_vars, l, seed, free=1, density=3):
    """Random sparse A and B and a witness; every row of C is a single entry that makes the row hold.  A has no entry in column 0 and C's
    entry is never there, so the witness (1, 0, 0, ...) satisfies the circuit too; the last `free` variables are in no row (their query
    points are the identity), so a witness may take any value there.  -> (Circuit, z)"""
    rng = random.Random(seed)
    used = n_vars - free
    assert used >= 2 and l < n_vars
    z = [1] + [rng.randrange(1, R) for _ in range(n_vars - 1)]
    a, b, c = [], [], []
    assert l + 1 <= used
    for i in range(n_cons):
        ra = [(rng.randrange(1, used), rng.randrange(1, R)) for _ in range(rng.randrange(1, 2 * density))]
        rb = [(rng.randrange(0, used), rng.randrange(1, R)) for _ in range(rng.randrange(1, 2 * density))]
        if i == 0:                                           # the constant and every public variable are in some row: no IC_j is the identity
            ra += [(j, rng.randrange(1, R)) for j in range(1, l + 1)]
            rb += [(0, rng.randrange(1, R))]
        col = rng.randrange(1, used)
        va, vb = sum(v * z[k] for k, v in ra) % R, sum(v * z[k] for k, v in rb) % R
        a.append(ra)
        b.append(rb)
        c.append([(col, va * vb * inv(z[col]) % R)])
    ct = Circuit(log_n, n_vars, l, a, b, c)
    assert ct.satisfied(z) and ct.satisfied([1] + [0] * (n_vars - 1))
    return ct, z


# ---- the quotient ---------------------------------------------------------------------------------------------------------------------
def poly_mul(f, g):
    """the product of two polynomials of n = 2^k coefficients each, 2 n coefficients: schoolbook for short ones, else through the model's own
    transform on the domain of 2 n points"""
    n = len(f)
    assert len(g) == n and n & (n - 1) == 0
    if n <= 64:
        out = [0] * (2 * n)
        for i, x in enumerate(f):
            for j, y in enumerate(g):
                out[i + j] = (out[i + j] + x * y) % R
        return out
    lg = n.bit_length()                                  # log2(2 n)
    ef, eg = N.ntt_radix2(list(f) + [0] * n, lg), N.ntt_radix2(list(g) + [0] * n, lg)
    return N.ntt_radix2([x * y % R for x, y in zip(ef, eg)], lg, inverse=True)


def divide_by_vanishing(p, n):
    """(quotient, remainder) of p by X^n - 1, long division from the top coefficient down"""
    rem, q = [v % R for v in p], [0] * max(len(p) - n, 0)
    for k in range(len(rem) - 1, n - 1, -1):
        q[k - n] = rem[k]
        rem[k - n] = (rem[k - n] + rem[k]) % R
        rem[k] = 0
    return q, rem[:n]


def quotient_exact(a, b, c, log_n):
    """h with a b - c = h (X^n - 1) for the polynomials of degree < n whose values on <w_n> are a, b, c: n coefficients (h[n - 1] = 0) and
    the remainder, which is zero exactly when a_i b_i = c_i on the whole domain"""
    n = 1 << log_n
    fa, fb, fc = (N.ntt_radix2([v % R for v in x], log_n, inverse=True) for x in (a, b, c))
    p = poly_mul(fa, fb)
    for k in range(n):
        p[k] = (p[k] - fc[k]) % R
    return divide_by_vanishing(p, n)


def zinv(log_n):
    zh = (pow(SHIFT, 1 << log_n, R) - 1) % R
    assert zh
    return inv(zh)


def quotient_coset(a, b, c, log_n):
    """THE DEFINITION: the coefficients of the polynomial of degree < n that equals (a b - c) / (X^n - 1) on the coset 5 <w_n>"""
    ca, cb, cc = (N.ntt_radix2(N.ntt_radix2([v % R for v in x], log_n, inverse=True), log_n, shift=SHIFT) for x in (a, b, c))
    zi = zinv(log_n)
    return N.ntt_radix2([(x * y - w) * zi % R for x, y, w in zip(ca, cb, cc)], log_n, inverse=True, shift=SHIFT)


# ---- setup and proof, in discrete logarithms ---------------------------------------------------------------------------------------------
def lagrange_at(log_n, tau):
    """L_i(tau) for the domain <w_n>: (tau^n - 1) w^i / (n (tau - w^i))"""
    n, w = 1 << log_n, N.omega(log_n)
    zt, ni = (pow(tau, n, R) - 1) % R, N.n_inverse(log_n)
    out, wi = [], 1
    for _ in range(n):
        out.append(zt * ni % R * wi % R * inv(tau - wi) % R)
        wi = wi * w % R
    return out


class Setup:
    """the discrete logarithms of a proving key and its verifying key for one circuit"""

    def __init__(self, ct, seed):
        rng = random.Random(seed)
        self.ct = ct
        self.tau, self.alpha, self.beta, self.gamma, self.delta = (rng.randrange(2, R) for _ in range(5))
        lag = lagrange_at(ct.log_n, self.tau)
        u, v, w = ([0] * ct.n_vars for _ in range(3))
        for acc, rows in ((u, ct.a), (v, ct.b), (w, ct.c)):
            for i, row in enumerate(rows):
                for col, val in row:
                    acc[col] = (acc[col] + val * lag[i]) % R
        self.u, self.v = u, v
        mix = [(self.beta * u[i] + self.alpha * v[i] + w[i]) % R for i in range(ct.n_vars)]
        di, gi, zt = inv(self.delta), inv(self.gamma), (pow(self.tau, ct.n, R) - 1) % R
        self.ic = [x * gi % R for x in mix[:ct.l + 1]]
        self.lq = [x * di % R for x in mix[ct.l + 1:]]
        self.hq = [pow(self.tau, k, R) * zt % R * di % R for k in range(ct.n - 1)]
        # an entry flagged as the identity enters every sum as zero, whatever its words hold: {query name: set of flagged indices}
        self.flagged = {"a_query": set(), "b_g1_query": set(), "b_g2_query": set(), "h_query": set(), "l_query": set()}

    def query(self, name):
        d = {"a_query": self.u, "b_g1_query": self.v, "b_g2_query": self.v, "h_query": self.hq, "l_query": self.lq}[name]
        return [0 if i in self.flagged[name] else x for i, x in enumerate(d)]

    def proof_dlogs(self, z, r, s, h=None):
        """(A, B, C) for the witness z and the randomness r, s (any integers, taken mod r); h: the quotient's coefficients (default: by the
        definition on the coset, which is the exact quotient for a satisfied witness)"""
        ct = self.ct
        z, r, s = [x % R for x in z], r % R, s % R
        if h is None:
            h = quotient_coset(matvec(ct.a, z, ct.n), matvec(ct.b, z, ct.n), matvec(ct.c, z, ct.n), ct.log_n)
        dot = lambda q, x: sum(a * b for a, b in zip(q, x)) % R
        a = (self.alpha + dot(self.query("a_query"), z) + r * self.delta) % R
        b2 = (self.beta + dot(self.query("b_g2_query"), z) + s * self.delta) % R
        b1 = (self.beta + dot(self.query("b_g1_query"), z) + s * self.delta) % R
        c = (dot(self.query("l_query"), z[ct.l + 1:]) + dot(self.query("h_query"), h[:ct.n - 1]) + s * a + r * b1 - r * s % R * self.delta) % R
        return a, b2, c

    def verifies(self, proof, inputs):
        """A B = alpha beta + vk_x gamma + C delta in Fr, vk_x = IC_0 + sum_j x_j IC_j"""
        a, b, c = proof
        vk_x = (self.ic[0] + sum(x % R * w for x, w in zip(inputs, self.ic[1:]))) % R
        return (a * b - self.alpha * self.beta - vk_x * self.gamma - c * self.delta) % R == 0


def free_key(ct, seed):
    """a Setup whose query logarithms u, v, lq, hq are independent random values in Fr for every index.  The prover never checks a key against
    its circuit, so proof_dlogs is still "the formulas' points" -- at any number of variables, without the Lagrange sums; ic keeps the
    circuit's values, so `verifies` means nothing under such a key"""
    st = Setup(ct, seed)
    rng = random.Random(seed * 0x9E3779B1 + 1)
    st.u, st.v = ([rng.randrange(R) for _ in range(ct.n_vars)] for _ in range(2))
    st.lq = [rng.randrange(R) for _ in range(ct.n_vars - ct.l - 1)]
    st.hq = [rng.randrange(R) for _ in range(ct.n - 1)]
    return st


def zero_witness(ct):
    """zero but for z_0 = 1: every sum of the proof is empty (make_circuit keeps column 0 out of A and C)"""
    return [1] + [0] * (ct.n_vars - 1)


def witness_mix(ct, z, m, seed, zero_rows=()):
    """m witnesses, each one of: z; the zero witness; a vector of random 256-bit words with z_0 = 1 (unsatisfied: its proof is the one by
    the definition on the coset).  Adjacent rows never hold the same witness, so no two neighbouring rows share a proof; the rows in
    zero_rows hold the zero witness."""
    rng = random.Random(seed)
    kinds = []
    for j in range(m):
        near = {kinds[j - 1]} if j else set()
        if j + 1 in zero_rows:
            near.add(1)
        kinds.append(1 if j in zero_rows else rng.choice([k for k in (0, 1, 2) if k == 2 or k not in near]))
    assert not any(j in zero_rows and j + 1 in zero_rows for j in range(m)), "two planted rows side by side would share a witness"
    out = [list(z) if k == 0 else zero_witness(ct) if k == 1 else [1] + [rng.randrange(1 << 256) for _ in range(ct.n_vars - 1)] for k in kinds]
    assert all(out[j] != out[j + 1] for j in range(m - 1))
    return out


def planted_randomness(st, what, rng):
    """(r, s) under which the point `what` ("A", "B" or "C") of the ZERO witness's proof is the identity.  With z = (1, 0, ...) the sums
    leave A = a0 + r delta, B = b0 + s delta and C = s A + r B - r s delta = s (a0 + r delta) + r b0, a0 = alpha + u_0, b0 = beta + v_0:
    A = 0 at r = -a0 / delta, B = 0 at s = -b0 / delta, C = 0 at s = -r b0 / (a0 + r delta) for any r that leaves A != 0"""
    a0, b0 = (st.alpha + st.query("a_query")[0]) % R, (st.beta + st.query("b_g1_query")[0]) % R
    assert st.query("b_g2_query")[0] == st.query("b_g1_query")[0]
    if what == "A":
        return -a0 * inv(st.delta) % R, rng.randrange(1, R)
    if what == "B":
        return rng.randrange(1, R), -b0 * inv(st.delta) % R
    assert what == "C"
    r = rng.randrange(1, R)
    assert (a0 + r * st.delta) % R
    return r, -r * b0 * inv(a0 + r * st.delta) % R


# ---- the same as points (the C oracle's generator multiples) -----------------------------------------------------------------------------
def key_points(setup, g1_mul=None, g2_mul=None):
    """{name: (affine words, flags)}: the proving key as arrays.  A zero logarithm is the identity, flagged; so is a flagged entry.
    g1_mul / g2_mul: [logarithms] -> (words, flags), by default the oracle's (4 ms a point: a caller with thousands of points brings its own)"""
    import numpy as np

    import groth16_model as G
    g1_mul, g2_mul = g1_mul or G.g1_gen_mul, g2_mul or G.g2_gen_mul
    out = {}
    for name, d in (("alpha_g1", [setup.alpha]), ("beta_g1", [setup.beta]), ("delta_g1", [setup.delta])):
        out[name] = G.g1_gen_mul(d)
    for name, d in (("beta_g2", [setup.beta]), ("delta_g2", [setup.delta])):
        out[name] = G.g2_gen_mul(d)
    for name in ("a_query", "b_g1_query", "h_query", "l_query", "b_g2_query"):
        mul, w = (g2_mul, 16) if name == "b_g2_query" else (g1_mul, 8)
        full = {"a_query": setup.u, "b_g1_query": setup.v, "b_g2_query": setup.v, "h_query": setup.hq, "l_query": setup.lq}[name]
        if full:
            xy, inf = mul(full)                              # a flagged entry keeps the words of its true point: the flag alone must count
            inf = np.array(inf, dtype=np.uint8)
            inf[sorted(setup.flagged[name])] = 1
        else:
            xy, inf = np.zeros((0, w), dtype=np.uint64), np.zeros(0, dtype=np.uint8)
        out[name] = (xy, inf)
    return out


def vk_points(setup):
    """(alpha, beta, gamma, delta, ic) affine words, as tests/groth16_model.py's Instance.vk() gives them"""
    import groth16_model as G
    return (G.g1_gen_mul([setup.alpha])[0], G.g2_gen_mul([setup.beta])[0], G.g2_gen_mul([setup.gamma])[0], G.g2_gen_mul([setup.delta])[0],
            G.g1_gen_mul(setup.ic)[0])


def proof_points(dlogs):
    """[(A, B, C) logarithms] -> ((A words, flags), (B words, flags), (C words, flags))"""
    import groth16_model as G
    return G.g1_gen_mul([d[0] for d in dlogs]), G.g2_gen_mul([d[1] for d in dlogs]), G.g1_gen_mul([d[2] for d in dlogs])
