"""Poseidon over the BN254 scalar field in plain integers: the circomlib / circomlibjs instance (x^5, t = 2 .. 17, R_F = 8, R_P per width),
its parameters from the Poseidon paper's Grain LFSR, the permutation, the hash and the binary Merkle tree built from hash([left, right]).
The model of tests/test_poseidon_model.py and of the GPU tests; it shares nothing with the C++ generator (sylow_amd/csrc/poseidon_params.hpp).
Not a test."""
from functools import lru_cache

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
R_F = 8
R_P = {t: rp for t, rp in zip(range(2, 18), (56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68))}
T_MIN, T_MAX = 2, 17
FIELD_BITS = 254


class Grain:
    """the 80-bit register; bit 0 is the oldest"""

    def __init__(self, t):
        fields = ((2, 1), (4, 0), (12, FIELD_BITS), (12, t), (10, R_F), (10, R_P[t]), (30, (1 << 30) - 1))
        self.b = [(v >> (w - 1 - k)) & 1 for w, v in fields for k in range(w)]
        assert len(self.b) == 80
        for _ in range(160):
            self.update()

    def update(self):
        b = self.b
        new = b[62] ^ b[51] ^ b[38] ^ b[23] ^ b[13] ^ b[0]
        b.pop(0)
        b.append(new)
        return new

    def bit(self):
        while not self.update():
            self.update()
        return self.update()

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v


@lru_cache(maxsize=None)
def draws(t):
    """(round constants [(R_F + R_P) t], xs [t], ys [t]) as the generator draws them"""
    g = Grain(t)
    consts = []
    while len(consts) < (R_F + R_P[t]) * t:
        v = g.bits(FIELD_BITS)
        if v < R:
            consts.append(v)
    while True:
        c = [g.bits(FIELD_BITS) % R for _ in range(2 * t)]
        if len(set(c)) == 2 * t:
            break
    return tuple(consts), tuple(c[:t]), tuple(c[t:])


@lru_cache(maxsize=None)
def params(t):
    """(C, M): C [(R_F + R_P) t] round-major, M [t][t] with M[i][j] = (xs[i] + ys[j])^-1"""
    consts, xs, ys = draws(t)
    return consts, tuple(tuple(pow((x + y) % R, R - 2, R) for y in ys) for x in xs)


def table(t):
    """the parameter table as the device holds it: the round constants, then M row by row"""
    C, M = params(t)
    return list(C) + [v for row in M for v in row]


def permute(state):
    t = len(state)
    C, M = params(t)
    s = [v % R for v in state]
    rounds = R_F + R_P[t]
    for r in range(rounds):
        s = [(v + C[r * t + i]) % R for i, v in enumerate(s)]
        if r < R_F // 2 or r >= R_F // 2 + R_P[t]:
            s = [pow(v, 5, R) for v in s]
        else:
            s[0] = pow(s[0], 5, R)
        s = [sum(M[i][j] * s[j] for j in range(t)) % R for i in range(t)]
    return s


def hash(inputs, init=0):
    return permute([init] + list(inputs))[0]


def merkle_levels(leaves):
    """levels 1 .. depth of the tree over 2^depth leaves, the root last"""
    out, cur = [], [v % R for v in leaves]
    while len(cur) > 1:
        cur = [hash([cur[2 * i], cur[2 * i + 1]]) for i in range(len(cur) // 2)]
        out.append(cur)
    return out


def merkle_nodes(leaves):
    """the n - 1 nodes in the order of nodes_out: level 1, level 2, ..., the root"""
    return [v for level in merkle_levels(leaves) for v in level]


def level_offset(depth, k):
    """where level k (1 .. depth) starts in nodes_out"""
    return (1 << depth) - (1 << (depth - k + 1))


def merkle_open(leaves, index):
    """the siblings of leaf `index`, level 0 (a leaf) first"""
    levels = [[v % R for v in leaves]] + merkle_levels(leaves)
    return [levels[k][(index >> k) ^ 1] for k in range(len(levels) - 1)]


def merkle_root(leaf, index, siblings):
    cur = leaf % R
    for k, s in enumerate(siblings):
        cur = hash([s, cur]) if (index >> k) & 1 else hash([cur, s])
    return cur
