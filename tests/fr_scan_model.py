"""A CPU model of the scans over BN254's Fr and of PLONK's permutation grand product (include/sylow_hip_fr_scan.h).  Not collected by pytest,
plain integers with Python's pow only, and it shares nothing with sylow_amd.  Inputs are any 256-bit integers, taken mod r; inv(0) = 0.

    scan:         out[k] = a[0] o .. o a[k]  (exclusive: a[0] o .. o a[k-1], the identity at k = 0);  op 0 is +, op 1 is *
    ratio scan:   t[i] = num[i] / den[i], out = the exclusive scan of t, total = t[0] o .. o t[len-1], status bit 0 = some den[i] = 0
    identity:     out[j][i] = shifts[j] w^i,  w = w_n of tests/ntt_model.py
    permutation:  z[0] = 1,  z[i+1] = z[i] prod_j (w_j[i] + beta shifts[j] w^i + gamma) / prod_j (w_j[i] + beta sigma_j[i] + gamma);
                  status bit 0 = a zero denominator, bit 1 = z[n] != 1"""
import os
import re

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
TOP = (1 << 256) - 1
W = pow(5, (R - 1) >> 28, R)
SUM, PRODUCT = 0, 1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_constants():
    """the named constants of sylow_amd/csrc/fr_scan_plan.hpp, read from the source"""
    src = open(os.path.join(ROOT, "sylow_amd", "csrc", "fr_scan_plan.hpp")).read()
    out = {name: int(re.search(r"constexpr (?:int|size_t) " + name + r" = (\d+);", src).group(1))
           for name in ("SCAN_BLOCK", "SCAN_LANE_ELEMS", "SCAN_CHUNK", "SCAN_TOTALS_TILE_MAX", "SCAN_TOTALS_TILE_DEFAULT", "PLONK_WIRES_MAX", "PLONK_LOG_N_MAX")}
    assert out["SCAN_CHUNK"] == out["SCAN_BLOCK"] * out["SCAN_LANE_ELEMS"]
    return out


def omega(log_n):
    assert 0 <= log_n <= 28
    return pow(W, 1 << (28 - log_n), R)


def inv(x):
    return pow(x % R, R - 2, R)                  # inv(0) = 0


def combine(op, a, b):
    assert op in (SUM, PRODUCT)
    return a * b % R if op == PRODUCT else (a + b) % R


def scan(a, op, exclusive=False):
    """(out, total)"""
    out, run = [], (1 if op == PRODUCT else 0)
    for v in a:
        if exclusive:
            out.append(run)
        run = combine(op, run, v % R)
        if not exclusive:
            out.append(run)
    return out, run


def ratio_scan(num, den, op):
    """(out, total, status); num None: all ones"""
    num = [1] * len(den) if num is None else num
    assert len(num) == len(den)
    out, total = scan([n % R * inv(d) % R for n, d in zip(num, den)], op, exclusive=True)
    return out, total, int(any(d % R == 0 for d in den))


def identity(shifts, log_n):
    w, out = omega(log_n), []
    for k in shifts:
        col, x = [], k % R
        for _ in range(1 << log_n):
            col.append(x)
            x = x * w % R
        out.append(col)
    return out


def sigma_from_mapping(shifts, log_n, mapping):
    """sigma[j][i] = the identity value of position mapping[j n + i]; mapping a permutation of the W n positions, position j n + i = (j, i)"""
    n = 1 << log_n
    flat = [v for col in identity(shifts, log_n) for v in col]
    assert sorted(mapping) == list(range(len(flat)))
    return [[flat[mapping[j * n + i]] for i in range(n)] for j in range(len(shifts))]


def terms(wires, sigma, shifts, beta, gamma, log_n):
    """(num, den) of one instance: wires [W][n], sigma [W][n]"""
    ident = identity(shifts, log_n)
    num, den = [], []
    for i in range(1 << log_n):
        a = b = 1
        for j in range(len(shifts)):
            a = a * (wires[j][i] + beta * ident[j][i] + gamma) % R
            b = b * (wires[j][i] + beta * sigma[j][i] + gamma) % R
        num.append(a)
        den.append(b)
    return num, den


def permutation(wires, sigma, shifts, beta, gamma, log_n):
    """(z, z_n, status) of one instance"""
    num, den = terms(wires, sigma, shifts, beta, gamma, log_n)
    z, total, status = ratio_scan(num, den, PRODUCT)
    return z, total, status | (2 if total != 1 else 0)


def cycles(mapping):
    """the cycles of a permutation, as lists of positions"""
    seen, out = set(), []
    for p in range(len(mapping)):
        if p in seen:
            continue
        cyc = []
        while p not in seen:
            seen.add(p)
            cyc.append(p)
            p = mapping[p]
        out.append(cyc)
    return out


def satisfying_wires(mapping, n_wires, log_n, rng):
    """wires [W][n] that are constant on every cycle of the mapping: the copy constraints hold"""
    n = 1 << log_n
    flat = [0] * (n_wires * n)
    for cyc in cycles(mapping):
        v = rng.randrange(R)
        for p in cyc:
            flat[p] = v
    return [flat[j * n:(j + 1) * n] for j in range(n_wires)]
