"""A CPU model of the recovery of a KZG polynomial from any half of the cells of its domain (kzg_recover.hip): n = c l points, c = 2^log_c
cells of l = 2^log_l values, cell i the values y[i + c j], j < l; a polynomial f of degree below n / 2; M the missing cells, |M| <= c / 2.
Not collected by pytest, and it shares nothing with sylow_amd.  Plain Python integers.

    Z(X) = prod_(i in M) (X^l - v^i), v = w^l, is a polynomial in X^l: c values zd on the domain, c values zc on the coset s <w>, s = 5.
    1. t[i + c j] = y[i + c j] zd[i]      2. P = INTT(t) = f Z      3. e = NTT_s(P)      4. q[t] = e[t] / zc[t mod c]      5. f = INTT_s(q)

recover() is those five steps with an O(n log n) transform of its own (fft), so that n = 8192 runs in a second or two.  The EXPECTED side
knows no transform: evaluate() is Horner's rule, dft_slow / idft_slow the sums of the definition, interpolate() Lagrange's formula, and
vanish_slow() expands Z into its coefficients and evaluates them."""
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
S = 5                      # the coset generator; also a generator of the multiplicative group, so the 2^28-th root below is primitive
LOG_C_MAX, LOG_N_MAX = 12, 27
OK, TOO_FEW, INCONSISTENT = 0, 1, 2


def inv(a):
    return pow(a % R, R - 2, R)


def omega(log_n):
    """the n-th root of the library's transforms: 5^((r - 1) / 2^28) squared down"""
    w = pow(5, (R - 1) >> 28, R)
    for _ in range(28 - log_n):
        w = w * w % R
    return w


def evaluate(p, x):
    acc = 0
    for v in reversed(p):
        acc = (acc * x + v) % R
    return acc


def dft_slow(a, log_n, shift=1):
    w = omega(log_n)
    return [evaluate(a, shift * pow(w, k, R) % R) for k in range(1 << log_n)]


def idft_slow(v, log_n, shift=1):
    n, wi, si = 1 << log_n, inv(omega(log_n)), inv(shift)
    ni = inv(n)
    return [ni * pow(si, k, R) * evaluate(v, pow(wi, k, R)) % R for k in range(n)]


def fft(a, log_n, inverse=False, shift=1):
    """forward: out_i = sum_k a_k (shift w^i)^k; inverse: out_k = n^-1 shift^-k sum_i a_i w^(-ik); natural order both ways"""
    n = 1 << log_n
    a = [x % R for x in a]
    assert len(a) == n
    if not inverse and shift != 1:
        p = 1
        for k in range(n):
            a[k], p = a[k] * p % R, p * shift % R
    rev = [0] * n
    for i in range(n):
        rev[i] = (rev[i >> 1] >> 1) | ((i & 1) << (log_n - 1)) if log_n else 0
    a = [a[rev[i]] for i in range(n)]
    w = omega(log_n)
    if inverse:
        w = inv(w)
    for s in range(log_n):
        half = 1 << s
        step = pow(w, n >> (s + 1), R)
        tw = [1] * half
        for j in range(1, half):
            tw[j] = tw[j - 1] * step % R
        for base in range(0, n, 2 * half):
            for j in range(half):
                u, v = a[base + j], a[base + j + half] * tw[j] % R
                a[base + j], a[base + j + half] = (u + v) % R, (u - v) % R
    if inverse:
        c, g, p = inv(n), inv(shift), 1
        for k in range(n):
            a[k], p = a[k] * c % R * p % R, p * g % R
    return a


def missing(present):
    return [i for i, p in enumerate(present) if not p]


def vanish(present, log_c, log_l):
    """(zd, zc, status): the c values of Z on the domain and on the coset; status 1 with zd = 0, zc = 1 when more than c / 2 cells miss"""
    c = 1 << log_c
    assert len(present) == c
    miss = missing(present)
    if len(miss) > c // 2:
        return [0] * c, [1] * c, TOO_FEW
    v = pow(omega(log_c + log_l), 1 << log_l, R)
    sl = pow(S, 1 << log_l, R)
    vp = [pow(v, k, R) for k in range(c)]
    zd, zc = [1] * c, [1] * c
    for k in range(c):
        for i in miss:
            zd[k] = zd[k] * (vp[k] - vp[i]) % R
            zc[k] = zc[k] * (sl * vp[k] - vp[i]) % R
    return zd, zc, OK


def vanish_slow(present, log_c, log_l):
    """the same values from the coefficients of Z, expanded factor by factor and evaluated at the points themselves"""
    c, l = 1 << log_c, 1 << log_l
    w = omega(log_c + log_l)
    z = [1]
    for i in missing(present):
        vi = pow(w, l * i, R)
        z = [(a - vi * b) % R for a, b in zip([0] * l + z, z + [0] * l)]     # times (X^l - v^i)
    return [evaluate(z, pow(w, k, R)) for k in range(c)], [evaluate(z, S * pow(w, k, R) % R) for k in range(c)]


def recover(y, present, log_c, log_l, transform=fft):
    """(status, the n coefficients of step 5): the five steps; words of y in missing cells are never part of the result"""
    c, L = 1 << log_c, log_c + log_l
    n = 1 << L
    assert len(y) == n and L >= 1
    zd, zc, status = vanish(present, log_c, log_l)
    if status == TOO_FEW:
        return TOO_FEW, [0] * n
    t = [(y[k] % R) * zd[k % c] % R for k in range(n)]
    p = transform(t, L, True)
    e = transform(p, L, False, S)
    zci = [inv(z) for z in zc]
    q = [e[k] * zci[k % c] % R for k in range(n)]
    f = transform(q, L, True, S)
    return (INCONSISTENT if any(f[n // 2:]) else OK), f


def recover_slow(y, present, log_c, log_l):
    slow = lambda a, log_n, inverse=False, shift=1: idft_slow(a, log_n, shift) if inverse else dft_slow(a, log_n, shift)
    return recover(y, present, log_c, log_l, transform=slow)


def interpolate(xs, ys):
    """the coefficients of the polynomial of degree below len(xs) through (x_j, y_j): Lagrange's formula in integers"""
    k = len(xs)
    out = [0] * k
    for j in range(k):
        num, den = [1], 1
        for t in range(k):
            if t != j:
                num = [(a - xs[t] * b) % R for a, b in zip([0] + num, num + [0])]
                den = den * (xs[j] - xs[t]) % R
        s = (ys[j] % R) * inv(den) % R
        for e, a in enumerate(num):
            out[e] = (out[e] + s * a) % R
    return out


def cell_points(i, log_c, log_l):
    w = omega(log_c + log_l)
    return [pow(w, i + (j << log_c), R) for j in range(1 << log_l)]


def words(v):
    return [(v >> (64 * k)) & ((1 << 64) - 1) for k in range(4)]
