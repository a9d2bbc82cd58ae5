"""A CPU model of the radix-2 transform over BN254's Fr.  Not collected by pytest, integer arithmetic only, and it shares nothing with
sylow_amd.  With w = w_n = W^(2^(28 - log_n)) and the coset shift g (None: 1), natural order in and out:

    forward:  out_i = sum_k a_k (g w^i)^k            inverse:  out_k = n^-1 g^-k sum_i a_i w^(-ik)

Inputs and g are any 256-bit integers, taken mod r; an inverse with g = 0 mod r uses inv(0) = 0."""
import os
import re

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
TWO_ADICITY = 28
W = pow(5, (R - 1) >> TWO_ADICITY, R)
assert W == 0x2A3C09F0A58A7E8500E0A7EB8EF62ABC402D111E41112ED49BD61B6E725B19F0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = os.path.join(ROOT, "sylow_amd", "csrc", "ntt_plan.hpp")


def plan_constants():
    """the named integer constants of sylow_amd/csrc/ntt_plan.hpp, read from the source (one may name an earlier one)"""
    src = open(PLAN).read()
    out = {}
    for name, value in re.findall(r"constexpr (?:int|size_t) (NTT_[A-Z_]+) = ([^;]+);", src):
        value = re.sub(r"\((?:size_t|int)\)", "", value)
        out[name] = int(eval(value, {"__builtins__": {}}, dict(out)))
    return out


def omega(log_n):
    assert 0 <= log_n <= TWO_ADICITY
    return pow(W, 1 << (TWO_ADICITY - log_n), R)


def n_inverse(log_n):
    """n^-1 the way the plan header forms it: r - ((r - 1) >> log_n)"""
    return R - ((R - 1) >> log_n)


def inv(x):
    return pow(x % R, R - 2, R)                  # inv(0) = 0


def ntt_direct(a, log_n, inverse=False, shift=None):
    """the O(n^2) definition"""
    n, w = 1 << log_n, omega(log_n)
    assert len(a) == n
    a = [v % R for v in a]
    g = 1 if shift is None else shift % R
    if not inverse:
        return [sum(a[k] * pow(g * pow(w, i, R), k, R) for k in range(n)) % R for i in range(n)]
    gi, wi, ni = inv(g), inv(w), n_inverse(log_n)
    return [ni * pow(gi, k, R) * sum(a[i] * pow(wi, i * k, R) for i in range(n)) % R for k in range(n)]


def _radix2(a, w):
    n = len(a)
    if n == 1:
        return list(a)
    ev, od = _radix2(a[0::2], w * w % R), _radix2(a[1::2], w * w % R)
    out, t = [0] * n, 1
    for i in range(n // 2):
        out[i], out[i + n // 2] = (ev[i] + t * od[i]) % R, (ev[i] - t * od[i]) % R
        t = t * w % R
    return out


def _scale(a, c, s):
    """the element-wise kernel: c s^k a_k"""
    out, p = [], c % R
    for v in a:
        out.append(p * (v % R) % R)
        p = p * s % R
    return out


def ntt_radix2(a, log_n, inverse=False, shift=None):
    """the textbook recursive radix-2 transform, the shift and the scale as element-wise products"""
    assert len(a) == 1 << log_n
    g = 1 if shift is None else shift % R
    if not inverse:
        return _radix2(_scale(a, 1, g), omega(log_n))
    return _scale(_radix2([v % R for v in a], inv(omega(log_n))), n_inverse(log_n), inv(g))


def pass_plan(log_n, stages):
    """[(stages of pass p, log2 of the length finished before it)]: every pass has `stages` but the last, which has what is left"""
    out, done = [], 0
    while done < log_n:
        s = min(stages, log_n - done)
        out.append((s, done))
        done += s
    return out


def _bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def _pass(src, log_n, s, done, table, inverse):
    """one Stockham pass as k_ntt_pass runs it: for j < n / R, R = 2^s, Ns = 2^done:
    v_r = src[j + r n/R] w^(r (j mod Ns) n/(Ns R)); s decimation-in-frequency stages in place; dst[(j div Ns) Ns R + j mod Ns + r' Ns] = v[bitrev r']"""
    n, half = 1 << log_n, 1 << (log_n - 1)

    def tw(e):                                   # w^e (inverse: w^-e) from the table of the first half
        if inverse:
            e = (n - e) & (n - 1)
        return table[e] if e < half else (R - table[e - half]) % R

    dst = [None] * n
    for j in range(n >> s):
        k = j & ((1 << done) - 1)
        v = [src[j + (r << (log_n - s))] * (tw((r * k) << (log_n - done - s)) if r * k else 1) % R for r in range(1 << s)]
        for hl in range(s - 1, -1, -1):
            h = 1 << hl
            for q in range(1 << (s - 1)):
                lo = q & (h - 1)
                i0 = ((q >> hl) << (hl + 1)) | lo
                u, x = v[i0], v[i0 + h]
                v[i0] = (u + x) % R
                v[i0 + h] = (u - x) * (tw(lo << (log_n - hl - 1)) if hl else 1) % R
        for r in range(1 << s):
            dst[((j >> done) << (done + s)) + k + (r << done)] = v[_bitrev(r, s)]
    assert None not in dst
    return dst


def ntt_passes(a, log_n, stages, inverse=False, shift=None, trace=None):
    """the transform by the decomposition of ntt.hip: the table w^e, e < n/2; the forward shift as the element-wise step BEFORE the passes, the
    inverse's scale AFTER them; ceil(log_n / stages) passes; the steps ping-pong between `out` and one buffer so that the last writes `out`.
    trace (a list) receives the name of the buffer each step wrote."""
    n = 1 << log_n
    assert len(a) == n and stages >= 1
    w, g = omega(log_n), (1 if shift is None else shift % R)
    table = [pow(w, e, R) for e in range(n // 2)]
    plan = pass_plan(log_n, stages)
    scales = inverse or shift is not None or log_n == 0
    n_steps = len(plan) + (1 if scales else 0)
    bufs = {"out": None, "buf": None}
    src, step = [v % R for v in a], 0

    def write(values):
        nonlocal src, step
        name = "out" if (n_steps - 1 - step) % 2 == 0 else "buf"
        bufs[name] = values
        if trace is not None:
            trace.append(name)
        src, step = values, step + 1

    if scales and not inverse:
        write(_scale(src, 1, g))
    for s, done in plan:
        write(_pass(src, log_n, s, done, table, inverse))
    if inverse:
        write(_scale(src, n_inverse(log_n), inv(g)))
    assert step == n_steps and (n_steps == 0 or bufs["out"] is src)
    return src
