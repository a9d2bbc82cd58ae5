"""Host-side mirror of sylow's public items for the hot path, batch-first.

Names and argument meaning follow src/lib.rs:71-84,105-236 (`pairing`, `glued_pairing`, `sign`,
`verify`, `G1Affine`/`G1Projective`, `G2Affine`/`G2Projective`, `Gt`, `Fp`), so tests written against
the reference read the same here -- except that every object is a BATCH of n values and every call
runs on the GPU through the C ABI.  Error behaviour mirrors `GroupError` (groups/group.rs:38-47):
constructors that validate raise `GroupError` with the reference's variant names.

Fp batches are numpy uint64 [n, 4] (little-endian limbs of the canonical value, `Fp::value().to_words()`).
"""
from __future__ import annotations

import numpy as np

from .engine import Engine

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R_ORDER = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001      # fp.rs:60-65
_M64 = (1 << 64) - 1
_G2 = (0x1800DEEF121F1E76426A00665E5C4479674322D4F75EDADD46DEBD5CD992F6ED,
       0x198E9393920D483A7260BFB731FB5D25F1AA493335A9E71297E485B7AEF312C2,
       0x12C85EA5DB8C6DEB4AAB71808DCB408FE3D1E7690C43D37B4CE6CC0166FA7DAA,
       0x090689D0585FF075EC9E99AD690C3395BC4B313370B38EF355ACDADCD122975B)
DST = b"WARLOCK-CHAOS-V01-CS01-SHA-256"   # src/lib.rs:90

_engine: Engine | None = None


def engine() -> Engine:
    global _engine
    if _engine is None:
        _engine = Engine(0)
    return _engine


def set_engine(e: Engine) -> None:
    global _engine
    _engine = e


class GroupError(Exception):
    """groups/group.rs:38-47"""
    NOT_ON_CURVE, NOT_IN_SUBGROUP, CANNOT_HASH_TO_GROUP, DECODE_ERROR = "NotOnCurve", "NotInSubgroup", "CannotHashToGroup", "DecodeError"


def _ints(arr) -> list:
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(arr[i, k]) << (64 * k) for k in range(4)) for i in range(arr.shape[0])]


def fp(values) -> np.ndarray:
    """Fp::new on a list of Python ints (any 256-bit value; reduced on the device like the reference)."""
    vals = [int(v) for v in np.atleast_1d(np.asarray(values, dtype=object))]
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            out[i, k] = (v >> (64 * k)) & _M64
    return out


def _row(vals):
    return np.array([[(v >> (64 * k)) & _M64 for v in vals for k in range(4)]], dtype=np.uint64)


def _raise_status(st):
    """per-element status bytes (include/sylow_hip.h) -> the reference's error for the first failing element"""
    names = {1: GroupError.NOT_ON_CURVE, 2: GroupError.NOT_IN_SUBGROUP, 3: GroupError.CANNOT_HASH_TO_GROUP, 4: GroupError.DECODE_ERROR}
    bad = np.nonzero(np.asarray(st))[0]
    if len(bad):
        raise GroupError(names[int(st[bad[0]])])


def fp_from_be_bytes(blobs):
    """Fp::from_be_bytes (fp.rs:686-719): (values [n, 4], is_some [n]) -- both halves of the CtOption (value = v mod p)."""
    v, st = engine().fp_from_be_bytes(list(blobs))
    return v, st == 0


def fp_to_be_bytes(values):                         # fp.rs:727-737
    return engine().fp_to_be_bytes(values)


class _Points:
    WIDTH = 0

    def __init__(self, xy: np.ndarray, infinity: np.ndarray | None = None):
        self.xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, self.WIDTH)
        n = self.xy.shape[0]
        self.infinity = np.zeros(n, dtype=np.uint8) if infinity is None else np.ascontiguousarray(infinity, dtype=np.uint8).reshape(n)

    def __len__(self):
        return self.xy.shape[0]

    def __eq__(self, other):                       # GroupAffine ct_eq (group.rs:226-235), elementwise
        both_inf = (self.infinity & other.infinity).astype(bool)
        same = (~self.infinity.astype(bool)) & (~other.infinity.astype(bool)) & (self.xy == other.xy).all(axis=1)
        return both_inf | same

    def is_zero(self):
        return self.infinity.astype(bool)



def _random_scalars(n, seed):
    """n scalars in [0, r) as [n, 4] limbs.  seed None: the operating system's generator (what the reference's `rand(&mut OsRng)` call
    sites use); an int: the reproducible xoshiro test stream -- NOT for secrets or nonces."""
    if seed is None:
        import secrets
        return fp([secrets.randbelow(R_ORDER) for _ in range(n)])
    return engine().fr_add(engine().xoshiro_fp_soa(seed, n).T.copy(), np.zeros((n, 4), dtype=np.uint64))

class G1Affine(_Points):
    """Batch of G1 points in affine form (g1.rs:30); identity = (0, 1, infinity)."""
    WIDTH = 8

    @classmethod
    def generator(cls, n=1):                       # g1.rs:54-60
        return cls(np.repeat(_row([1, 2]), n, 0))

    @classmethod
    def zero(cls, n=1):
        return cls(np.repeat(_row([0, 1]), n, 0), np.ones(n, dtype=np.uint8))

    @classmethod
    def hash_to_curve(cls, msgs, dst: bytes = DST, expander=None):     # g1.rs:307-331; expander None: XMDExpander<Keccak256>(dst, 128)
        if expander is not None:
            xy, inf = engine().hash_to_g1(list(msgs), expander.dst, expander=expander.id, k=expander.k)
        else:
            xy, inf = engine().hash_to_g1(list(msgs), dst)
        return cls(xy, inf)

    def __mul__(self, k):                          # Mul<&Fp> (group.rs:639-667)
        xy, inf = engine().g1_scalar_mul(self.xy, k, self.infinity)
        return G1Affine(xy, inf)

    def __add__(self, other):                      # Add (group.rs:528-599)
        xy, inf = engine().g1_add(self.xy, other.xy, self.infinity, other.infinity)
        return G1Affine(xy, inf)

    def __sub__(self, other):                      # Sub (group.rs:614-624): self + (-other)
        xy, inf = engine().g1_sub(self.xy, other.xy, self.infinity, other.infinity)
        return G1Affine(xy, inf)

    def __neg__(self):
        y = engine().fp_neg(self.xy[:, 4:])
        return G1Affine(np.concatenate([self.xy[:, :4], y], axis=1), self.infinity)

    def double(self):                              # GroupProjective::double (group.rs:339-386)
        xy, inf = engine().g1_double(self.xy, self.infinity)
        return G1Affine(xy, inf)

    @classmethod
    def rand(cls, n=1, seed=None):                 # GroupTrait::rand (g1.rs:293-305): generator * random scalar; an int seed is test-only
        xy, inf = engine().g1_generator_mul(_random_scalars(n, seed))
        return cls(xy, inf)

    def to_be_bytes(self):                         # g1.rs:151-180
        return engine().g1_to_be_bytes(self.xy, self.infinity)

    @classmethod
    def from_be_bytes(cls, blobs):                 # g1.rs:224-280: CtOption none -> GroupError(DecodeError / NotOnCurve)
        xy, inf, st = engine().g1_from_be_bytes(list(blobs))
        _raise_status(st)
        return cls(xy, inf)


G1Projective = G1Affine   # results are compared after normalisation: one batch type serves both names


class G2Affine(_Points):
    WIDTH = 16
    in_subgroup = False                            # set on values whose r-torsion membership is established

    def _checked(self, flag=True):
        self.in_subgroup = bool(flag)
        return self

    @classmethod
    def generator(cls, n=1):                       # g2.rs:47-77
        return cls(np.repeat(_row(_G2), n, 0))._checked()

    @classmethod
    def zero(cls, n=1):
        return cls(np.repeat(_row([0, 0, 1, 0]), n, 0), np.ones(n, dtype=np.uint8))._checked()

    @classmethod
    def new(cls, xy):                              # G2Projective::new (g2.rs:460-525): on-curve + subgroup
        pts = cls(xy)
        st = engine().g2_subgroup_check(pts.xy, pts.infinity)
        if (st == 1).any():
            raise GroupError(GroupError.NOT_ON_CURVE)
        if (st == 2).any():
            raise GroupError(GroupError.NOT_IN_SUBGROUP)
        return pts._checked()

    def __mul__(self, k):
        # values built the way the reference allows (generator, new, from_be_bytes, and what the group law makes of them) are in
        # the r-torsion and take the endomorphism-split product; a raw G2Affine(xy) is treated as an arbitrary twist point
        xy, inf = engine().g2_scalar_mul(self.xy, k, self.infinity, subgroup=self.in_subgroup)
        return G2Affine(xy, inf)._checked(self.in_subgroup)

    def __neg__(self):
        y = np.concatenate([engine().fp_neg(self.xy[:, 8:12]), engine().fp_neg(self.xy[:, 12:16])], axis=1)
        return G2Affine(np.concatenate([self.xy[:, :8], y], axis=1), self.infinity)._checked(self.in_subgroup)

    def __add__(self, other):
        xy, inf = engine().g2_add(self.xy, other.xy, self.infinity, other.infinity)
        return G2Affine(xy, inf)._checked(self.in_subgroup and other.in_subgroup)

    def __sub__(self, other):                      # Sub (group.rs:614-624)
        xy, inf = engine().g2_sub(self.xy, other.xy, self.infinity, other.infinity)
        return G2Affine(xy, inf)._checked(self.in_subgroup and other.in_subgroup)

    def double(self):
        xy, inf = engine().g2_double(self.xy, self.infinity)
        return G2Affine(xy, inf)._checked(self.in_subgroup)

    def precompute(self) -> "G2PreComputed":        # pairing.rs:676
        return G2PreComputed(self)

    def endomorphism(self) -> "G2Affine":           # GroupTrait::endomorphism = psi (g2.rs:140-152); panics upstream if the image is off-curve
        xy, inf, st = engine().g2_psi(self.xy, self.infinity)
        _raise_status(st)
        return G2Affine(xy, inf)._checked(self.in_subgroup)

    @classmethod
    def rand(cls, n=1, seed=None):                 # GroupTrait::rand (g2.rs:204-240): a random r-torsion point; an int seed is test-only
        xy, inf = engine().g2_generator_mul(_random_scalars(n, seed))
        return cls(xy, inf)._checked()

    def to_be_bytes(self):                         # g2.rs:319-359
        return engine().g2_to_be_bytes(self.xy, self.infinity)

    @classmethod
    def from_be_bytes(cls, blobs):                 # g2.rs:361-433 (decode + on-curve + subgroup)
        xy, inf, st = engine().g2_from_be_bytes(list(blobs))
        _raise_status(st)
        return cls(xy, inf)._checked()


G2Projective = G2Affine



class _Ext:
    """Batch of extension-field elements, canonical limbs [n, 4 * degree] in the reference's nesting order; the operators of
    FieldExtension<D, N, F> (extensions.rs:41-238) run on the GPU."""
    DEGREE = 0

    def __init__(self, v):
        self.v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4 * self.DEGREE)

    def __len__(self): return self.v.shape[0]
    def __eq__(self, o): return (self.v == o.v).all(axis=1)
    def __add__(self, o): return type(self)(engine().fext_op("add", self.v, o.v))
    def __sub__(self, o): return type(self)(engine().fext_op("sub", self.v, o.v))
    def __neg__(self): return type(self)(engine().fext_op("neg", self.v))
    def scale(self, k): return type(self)(engine().fext_op("scale", self.v, np.ascontiguousarray(k, dtype=np.uint64).reshape(-1, 4)))


class Fp2(_Ext):
    DEGREE = 2
    def __mul__(self, o): return Fp2(engine().fp2_mul(self.v, o.v))
    def square(self): return Fp2(engine().fp2_sqr(self.v))
    def inv(self): return Fp2(engine().fp2_inv(self.v))
    def residue_mul(self): return Fp2(engine().fp2_residue_mul(self.v))          # x (9 + u), fp2.rs:99-107
    def frobenius(self, exponent: int): return Fp2(engine().fp2_frobenius(self.v, exponent))   # fp2.rs:119-133


class Fp6(_Ext):
    DEGREE = 6
    def __mul__(self, o): return Fp6(engine().fp6_mul(self.v, o.v))
    def square(self): return Fp6(engine().fp6_sqr(self.v))                       # fp6.rs:213-236
    def inv(self): return Fp6(engine().fp6_inv(self.v))
    def residue_mul(self): return Fp6(engine().fp6_residue_mul(self.v))          # x v, fp6.rs:189-192
    def frobenius(self, exponent: int): return Fp6(engine().fp6_frobenius(self.v, exponent))   # fp6.rs:205-211


class Fp12(_Ext):
    DEGREE = 12
    def __mul__(self, o): return Fp12(engine().fp12_mul(self.v, o.v))
    def square(self): return Fp12(engine().fp12_sqr(self.v))
    def inv(self): return Fp12(engine().fp12_inv(self.v))
    def frobenius(self, exponent: int): return Fp12(engine().fp12_frobenius(self.v, exponent))  # exponent in {1, 2, 3}
    def sparse_mul(self, ell): return Fp12(engine().fp12_sparse_mul(self.v, ell))               # fp12.rs:426-503, ell = [n, 24]


class Gt:
    """Batch of target-group elements (groups/gt.rs): 12 Fp each; `+` is the group law (Fp12 product)."""

    def __init__(self, v: np.ndarray):
        self.v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 48)

    @classmethod
    def identity(cls, n=1):                        # gt.rs:263-265
        v = np.zeros((n, 48), dtype=np.uint64)
        v[:, 0] = 1
        return cls(v)

    def __len__(self):
        return self.v.shape[0]

    def __eq__(self, other):                       # gt.rs:139-159
        return (self.v == other.v).all(axis=1)

    def __add__(self, other):                      # gt.rs: Add = Fp12 multiplication
        return Gt(engine().fp12_mul(self.v, other.v))

    def __neg__(self):                             # gt.rs:107-114: unitary inverse (conjugate)
        v = self.v.copy()
        v[:, 24:] = np.concatenate([engine().fp_neg(self.v[:, 24 + 4 * j:28 + 4 * j]) for j in range(6)], axis=1)
        return Gt(v)

    def __mul__(self, k):                          # Mul<&Fr> (gt.rs:161-187); k: Fr values [n, 4]
        return Gt(engine().gt_pow(self.v, k))


class MillerLoopResult:
    """Batch of raw Miller values (pairing.rs:72): public but NOT unique -- the engine replays the reference's
    line formulas and digit schedule, so these match `G2PreComputed::miller_loop` bit for bit."""

    def __init__(self, v: np.ndarray):
        self.v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 48)

    def __eq__(self, other):
        return (self.v == other.v).all(axis=1)

    def __mul__(self, other):                      # Mul<&MillerLoopResult> (pairing.rs:98-128): Fp12 product
        return MillerLoopResult(engine().fp12_mul(self.v, other.v))

    def final_exponentiation(self) -> "Gt":        # pairing.rs:245-492
        return Gt(engine().final_exp(self.v))


class Fr:
    """Batch of scalar-field elements (fp.rs:556-565), canonical limbs [n, 4]; arithmetic runs on the GPU."""

    def __init__(self, v):
        self.v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)

    @classmethod
    def from_ints(cls, values):
        return cls(fp(values))

    def __len__(self): return self.v.shape[0]
    def __add__(self, o): return Fr(engine().fr_add(self.v, o.v))
    def __sub__(self, o): return Fr(engine().fr_sub(self.v, o.v))
    def __mul__(self, o): return Fr(engine().fr_mul(self.v, o.v))
    def __neg__(self): return Fr(engine().fr_neg(self.v))
    def inv(self): return Fr(engine().fr_inv(self.v))
    def batch_inv(self): return Fr(engine().fr_batch_inv(self.v))   # the words of inv() (inv(0) = 0), one shared inversion per 2048 elements
    def __eq__(self, o): return (self.v == o.v).all(axis=1)
    # running sums / products of the batch taken as ONE row (sylow_hip_fr_scan_batch); exclusive: element k holds the elements before k
    def cumsum(self, exclusive=False): return Fr(engine().fr_scan(self.v, 0, exclusive)[0]) if len(self) else Fr(self.v)
    def cumprod(self, exclusive=False): return Fr(engine().fr_scan(self.v, 1, exclusive)[0]) if len(self) else Fr(self.v)

    @classmethod
    def from_be_bytes(cls, blobs):                 # Fr::from_be_bytes (fp.rs:746-778): none for v >= r
        v, st = engine().fr_from_be_bytes(list(blobs))
        _raise_status(st)
        return cls(v)

    def to_be_bytes(self):
        return engine().fr_to_be_bytes(self.v)

    @classmethod
    def rand(cls, n=1, seed=None):                 # FieldExtensionTrait::rand; seed None = OS generator, an int = reproducible test stream
        return cls(_random_scalars(n, seed))


def aggregate(points, weights: "Fr", n_jobs: int, n_terms: int):
    """sum_i weights[j,i] * points[j,i] per job (examples/threshold_signing.rs:124-143); rows are term-major
    (row i*n_jobs + j is term i of job j).  G1Affine in, G1Affine out; G2Affine in (public keys: a threshold group key
    sum_i lambda_i pk_i), G2Affine out."""
    if isinstance(points, G2Affine):
        xy, inf = engine().g2_lincomb(points.xy, weights.v, n_jobs, n_terms, points.infinity)
        return G2Affine(xy, inf)
    xy, inf = engine().g1_lincomb(points.xy, weights.v, n_jobs, n_terms, points.infinity)
    return G1Affine(xy, inf)


def msm(points, scalars):
    """sum_i scalars[i] * points[i] as one point (bucket method on the GPU): KZG-style commitments, random linear combinations,
    weighted aggregation over a whole batch.  scalars: Fr, or [n, 4] Fp words (values >= p are reduced like Fp::new).  Same
    point as aggregate(points, scalars, 1, n).  G1Affine in, G1Affine out; G2Affine in (a rogue-key-safe aggregate key
    sum_i t_i pk_i, the G2 half of a KZG verifier), G2Affine out."""
    v = scalars.v if isinstance(scalars, Fr) else np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    if len(points) != v.shape[0]:
        raise ValueError(f"msm: {len(points)} points but {v.shape[0]} scalars")
    if isinstance(points, G2Affine):
        xy, inf = engine().g2_msm(points.xy, v, points.infinity)
        return G2Affine(xy, inf)
    xy, inf = engine().g1_msm(points.xy, v, points.infinity)
    return G1Affine(xy, inf)


def point_sum(points):
    """sum_i points[i] as one point of the same type (the `+` fold of examples/dkg.rs:309-314 over keys, of
    examples/verify_multiple_messages_same_signer.rs:41-60 over signatures)."""
    if isinstance(points, G2Affine):
        xy, inf = engine().g2_sum(points.xy, points.infinity)
        return G2Affine(xy, inf)
    xy, inf = engine().g1_sum(points.xy, points.infinity)
    return G1Affine(xy, inf)


class G2PreComputed:
    """G2Affine::precompute() (pairing.rs:556,676-708): q plus the 87 line-coefficient triples, [n, 87*24] words."""

    def __init__(self, q: "G2Affine"):
        self.q = q
        self.coeffs = engine().g2_precompute(q.xy)

    def miller_loop(self, g1: G1Affine, table_idx=None) -> MillerLoopResult:     # pairing.rs:590-619
        """Consumes the cached tables (no G2 arithmetic): element i pairs g1[i] with table table_idx[i] (default: table i), so
        ONE precomputed key serves any number of G1 points."""
        if table_idx is None and len(g1) != len(self.q):
            raise ValueError(f"{len(g1)} G1 points against {len(self.q)} precomputed tables: pass table_idx (one table index per point)")
        return MillerLoopResult(engine().miller_loop_precomputed(self.coeffs, g1.xy, table_idx))


def glued_miller_loop(g2s, g1s: G1Affine, offsets=None) -> MillerLoopResult:
    """glued_miller_loop(&[G2PreComputed], &[G1Affine]) -> MillerLoopResult (pairing.rs:970-1022).  `g2s` is a G2PreComputed or
    G2Affine batch; without `offsets` the whole batch is one job."""
    q = g2s.q if isinstance(g2s, G2PreComputed) else g2s
    if offsets is None:
        offsets = [0, min(len(g1s), len(q))]               # zip truncates (pairing.rs:975)
    if isinstance(g2s, G2PreComputed) and len(g1s) == len(q):          # the cached tables are consumed as they are
        return MillerLoopResult(engine().glued_miller_loop_precomputed(g2s.coeffs, g1s.xy, offsets))
    return MillerLoopResult(engine().glued_miller_loop(g1s.xy, q.xy, offsets))


def pairing(p: G1Affine, q: G2Affine) -> Gt:
    """pairing(&G1Projective, &G2Projective) -> Gt (pairing.rs:870-893), n independent values."""
    return Gt(engine().pairing(p.xy, q.xy, p.infinity, q.infinity))


def glued_pairing(g1s: G1Affine, g2s: G2Affine, offsets=None, evm_infinity: bool = False) -> Gt:
    """glued_pairing(&[G1Projective], &[G2Projective]) -> Gt (pairing.rs:1029-1037).  Without `offsets` the
    whole batch is ONE product (the reference's shape); with offsets, job j multiplies pairs
    [offsets[j], offsets[j+1])."""
    if offsets is None:            # one product over the whole batch: spread over the GPU, one final exponentiation
        gt, _ = engine().pairing_product(g1s.xy, g2s.xy, g1s.infinity, g2s.infinity, skip_infinity=evm_infinity)
        return Gt(gt)
    gt, _ = engine().multi_pairing(g1s.xy, g2s.xy, offsets, g1s.infinity, g2s.infinity, skip_infinity=evm_infinity)
    return Gt(gt)


def verify_same_signer(pubkey: G2Affine, msgs, sig: G1Affine) -> np.ndarray:
    """examples/verify_multiple_messages_same_signer.rs:41-60: one key, many (message, signature) pairs."""
    assert len(pubkey) == 1
    return engine().bls_verify_same_signer(pubkey.xy, list(msgs), sig.xy, pubkey.infinity, sig.infinity).astype(bool)


def aggregate_verify(pubkey: G2Affine, msgs, sig: G1Affine) -> bool:
    """The batch check of examples/verify_multiple_messages_same_signer.rs:41-60 / threshold_signing.rs:92-121: the product of the
    2n pairs (sig_i, G2gen), (-H(msg_i), pk_i) == Gt::identity(), as one boolean; `pubkey` holds one key per message or ONE key.
    Two more shapes of `pubkey`, rows term-major like aggregate(): c * n keys are n COMMITTEES of c keys (key j belongs to message
    j mod n, sig_i is committee i's aggregate signature; the keys are summed, so they must come with proofs of possession), and n / c
    keys (at least two) are keys REUSED with that period (signature i is under key i mod len(pubkey))."""
    msgs = list(msgs)
    if not engine().aggregate_shape_ok(len(msgs), len(pubkey)) or len(sig) != len(msgs):
        raise ValueError(f"aggregate_verify: {len(pubkey)} keys and {len(sig)} signatures for {len(msgs)} messages")
    _, ok = engine().bls_aggregate_verify(pubkey.xy, msgs, sig.xy, pubkey.infinity, sig.infinity)
    return bool(ok)


def fast_aggregate_verify(pubkeys: G2Affine, msg: bytes, sig: G1Affine) -> bool:
    """Many signers, ONE message (examples/threshold_signing.rs:92-121, dkg.rs:146-175; every committee / validator-set check):
    e(sig, G2gen) e(-H(msg), sum_j pk_j) == Gt::identity() -- one hash, one G2 sum and two Miller loops whatever the number of keys.
    `sig` is the aggregate signature, or the signers' individual signatures (summed first).  Summing keys presumes proofs of
    possession: without them a signer can choose a key that cancels the others' (rogue-key attack)."""
    if len(pubkeys) == 0:
        raise ValueError("fast_aggregate_verify: no public keys")
    sig_xy, sig_inf = sig.xy, sig.infinity
    if len(sig) != 1:
        sig_xy, sig_inf = engine().g1_sum(sig_xy, sig_inf)
    _, ok = engine().bls_aggregate_verify(pubkeys.xy, [bytes(msg)], sig_xy, pubkeys.infinity, sig_inf)
    return bool(ok)


class KeyTable:
    """One signer's `G2PreComputed` kept ON THE DEVICE across calls (examples/verify_multiple_messages_same_signer.rs:41-60):
    built once, then every `verify` is two table-driven Miller loops with no G2 arithmetic."""

    def __init__(self, pubkey: G2Affine):
        assert len(pubkey) == 1
        self.infinity = pubkey.infinity
        self.table = engine().g2_line_table(pubkey.xy)

    def verify(self, msgs, sig: G1Affine) -> np.ndarray:
        return engine().bls_verify_line_table(self.table, list(msgs), sig.xy, self.infinity, sig.infinity).astype(bool)


def batch_verify(pubkey: G2Affine, msgs, sig: G1Affine, weight_bits: int = 128, seed=None) -> bool:
    """Sound one-boolean batch verification (the small-exponent test): prod_i [e(sig_i, G2gen) e(-H(m_i), pk_i)]^(w_i) == identity
    with fresh non-zero `weight_bits`-bit weights from the operating system's generator (an int `seed` draws reproducible weights:
    tests only).  True when every signature is valid; a batch with an invalid one passes with probability <= 2^-weight_bits PROVIDED
    the keys lie in G2 proper: keys whose r-torsion membership is not established (a G2Affine built from raw coordinates) go through
    the subgroup check first and a failing one raises, exactly where G2Projective::new (g2.rs:460-525) would have refused the key."""
    if not 1 <= int(weight_bits) <= 128:
        raise ValueError("weight_bits must be in 1..128")
    if not pubkey.in_subgroup:
        st = engine().g2_subgroup_check(pubkey.xy, pubkey.infinity)
        if np.any(st != 0):
            raise ValueError(f"batch_verify: public key {int(np.flatnonzero(st != 0)[0])} is not a point of G2 (status {int(st[st != 0][0])})")
    n = len(sig)
    mask = (1 << weight_bits) - 1
    if seed is None:
        import secrets
        w = []
        while len(w) < n:                                  # uniform over [1, 2^weight_bits): zero is redrawn, no bit is forced
            v = secrets.randbits(weight_bits)
            if v:
                w.append(v)
        w = fp(w)
    else:
        w = fp([(int(v) & mask) or 1 for v in _ints(engine().xoshiro_fp_soa(seed, n).T)])
    _, ok = engine().bls_batch_verify_weighted(pubkey.xy, list(msgs), sig.xy, w, pubkey.infinity, sig.infinity)
    return ok


class Groth16VerifyingKey:
    """A Groth16 verifying key on BN254: alpha (one G1 point), beta / gamma / delta (one G2 point each) and ic (the l + 1 G1 points
    IC_0 .. IC_l).  A plain holder: nothing is cached on the device between calls."""

    def __init__(self, alpha: G1Affine, beta: G2Affine, gamma: G2Affine, delta: G2Affine, ic: G1Affine):
        if not (len(alpha) == len(beta) == len(gamma) == len(delta) == 1 and len(ic) >= 1):
            raise ValueError("Groth16VerifyingKey: alpha, beta, gamma, delta are single points and ic holds at least IC_0")
        if alpha.infinity.any() or beta.infinity.any() or gamma.infinity.any() or delta.infinity.any() or ic.infinity.any():
            raise ValueError("Groth16VerifyingKey: the key's points cannot be the identity")
        self.alpha, self.beta, self.gamma, self.delta, self.ic = alpha, beta, gamma, delta, ic

    @property
    def n_inputs(self) -> int:
        return len(self.ic) - 1

    def arrays(self):
        return self.alpha.xy, self.beta.xy, self.gamma.xy, self.delta.xy, self.ic.xy


def groth16_verify(vk: Groth16VerifyingKey, a: G1Affine, b: G2Affine, c: G1Affine, inputs) -> np.ndarray:
    """ok[i] = [ e(-A_i, B_i) e(alpha, beta) e(IC_0 + sum_j x_ij IC_j, gamma) e(C_i, delta) == 1 ] for n proofs under one key; inputs
    [n, l, 4] words (or [n, l] Python ints), taken mod r.  Points are taken as given: B must lie in G2 proper (G2Affine.from_be_bytes and
    the subgroup check establish that), and a host that wants the Solidity rule rejects inputs >= r beforehand."""
    x = np.asarray(inputs)
    if x.dtype == object or x.ndim == 2:
        x = fp([int(v) for v in np.asarray(inputs, dtype=object).reshape(-1)]).reshape(len(a), vk.n_inputs, 4)
    return engine().groth16_verify(vk.arrays(), a.xy, b.xy, c.xy, x, a.infinity, b.infinity, c.infinity).astype(bool)


class Groth16ProvingKey:
    """A Groth16 proving key on BN254 under arkworks' names: the single points alpha_g1, beta_g1, delta_g1 (G1) and beta_g2, delta_g2 (G2), and
    the queries a_query, b_g1_query [n_vars] (G1), b_g2_query [n_vars] (G2), h_query [n - 1] (G1) and l_query [n_vars - l - 1] (G1).  A query
    entry may be the identity (a variable absent from A or B).  A plain holder: nothing is cached on the device between calls."""

    def __init__(self, alpha_g1: G1Affine, beta_g1: G1Affine, delta_g1: G1Affine, beta_g2: G2Affine, delta_g2: G2Affine, a_query: G1Affine,
                 b_g1_query: G1Affine, b_g2_query: G2Affine, h_query: G1Affine, l_query: G1Affine):
        singles = (alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2)
        if any(len(p) != 1 or p.infinity.any() for p in singles):
            raise ValueError("Groth16ProvingKey: alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2 are single points, not the identity")
        if not len(a_query) == len(b_g1_query) == len(b_g2_query):
            raise ValueError("Groth16ProvingKey: a_query, b_g1_query and b_g2_query hold one point per variable")
        self.alpha_g1, self.beta_g1, self.delta_g1, self.beta_g2, self.delta_g2 = singles
        self.a_query, self.b_g1_query, self.b_g2_query, self.h_query, self.l_query = a_query, b_g1_query, b_g2_query, h_query, l_query

    def arrays(self):
        out = {k: getattr(self, k).xy for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")}
        out.update({k: (getattr(self, k).xy, getattr(self, k).infinity) for k in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")})
        return out


class Groth16Circuit:
    """An R1CS over Fr for the prover: the matrices a, b, c in CSR -- each (row_ptr [n_cons + 1], col [nnz], val [nnz, 4] words or Python ints)
    -- over n_vars variables, of which variable 0 is the constant 1 and variables 1 .. n_inputs are public, on the domain of 2^log_n >=
    n_cons points."""

    def __init__(self, a, b, c, n_vars: int, n_inputs: int, log_n: int):
        self.mats = tuple(self._csr(m) for m in (a, b, c))
        self.n_vars, self.n_inputs, self.log_n = int(n_vars), int(n_inputs), int(log_n)
        self.n_cons = len(self.mats[0][0]) - 1
        if any(len(m[0]) - 1 != self.n_cons for m in self.mats):
            raise ValueError("Groth16Circuit: a, b and c have one row per constraint")
        if not (0 <= self.log_n <= 28 and self.n_cons <= 1 << self.log_n and 0 <= self.n_inputs < self.n_vars):
            raise ValueError("Groth16Circuit: n_cons <= 2^log_n <= 2^28 and n_inputs < n_vars")

    @staticmethod
    def _csr(m):
        row_ptr, col, val = m
        v = np.asarray(val)
        if v.dtype != np.uint64:
            v = fp([int(x) for x in np.asarray(val, dtype=object).reshape(-1)])
        return (np.asarray([int(x) for x in row_ptr], dtype=np.uint64), np.asarray([int(x) for x in col], dtype=np.uint64), v.reshape(-1, 4))


def groth16_prove(pk: Groth16ProvingKey, circuit: Groth16Circuit, witnesses, r, s):
    """(A: G1Affine, B: G2Affine, C: G1Affine), one proof per witness, for witnesses [m, n_vars, 4] words (or m lists of Python ints) and the
    caller's randomness r, s ([m, 4] words or Python ints) -- any 256-bit values, taken mod r (sylow_hip_groth16_prove_batch).  The three
    points are what groth16_verify takes, with inputs = witnesses[:, 1 : n_inputs + 1].  Neither z_0 = 1 nor the constraints are checked: an
    unsatisfied witness yields a proof the verifier rejects."""
    z = _fr_arrays(witnesses)
    if z.ndim != 3 or z.shape[1] != circuit.n_vars:
        raise ValueError("groth16_prove: witnesses hold one value per variable")
    if len(pk.a_query) != circuit.n_vars or len(pk.h_query) != (1 << circuit.log_n) - 1 or len(pk.l_query) != circuit.n_vars - circuit.n_inputs - 1:
        raise ValueError("groth16_prove: the proving key does not fit the circuit")
    (a, ai), (b, bi), (c, ci) = engine().groth16_prove(circuit.mats, circuit.n_vars, circuit.n_inputs, circuit.log_n, pk.arrays(), z,
                                                       KzgVerifier._words(r), KzgVerifier._words(s))
    return G1Affine(a, ai), G2Affine(b, bi), G1Affine(c, ci)


class KzgVerifier:
    """The verifier's half of a BN254 KZG SRS: tau_g2 = tau G2gen (one point of G2 proper, not the identity) and its line table, built on
    first use and kept on the device.  An opening is (C, z, y, pi) and claims f(z) = y for the polynomial committed in C; `openings` below is
    the tuple (c: G1Affine, z, y, pi: G1Affine) with z, y as [n, 4] words or Python ints -- any 256-bit values, taken mod r."""

    def __init__(self, tau_g2: G2Affine):
        if len(tau_g2) != 1 or tau_g2.infinity.any():
            raise ValueError("KzgVerifier: tau_g2 is a single point of G2, not the identity")
        self.tau_g2, self._table = tau_g2, None

    @staticmethod
    def _words(v):
        a = np.asarray(v)
        return fp([int(x) for x in np.asarray(v, dtype=object).reshape(-1)]) if a.dtype == object or a.ndim == 1 else a

    def verify(self, openings) -> np.ndarray:
        """ok[i] = [ e(C_i - y_i G1gen + z_i pi_i, G2gen) e(-pi_i, tau_g2) == 1 ]; identities follow EIP-197 (a flagged pi proves a constant
        polynomial: the row is valid iff C = y G1gen).  Points are taken as given."""
        c, z, y, pi = openings
        if self._table is None:
            self._table = engine().g2_line_table(self.tau_g2.xy)
        return engine().kzg_verify_line_table(self._table, c.xy, self._words(z), self._words(y), pi.xy, c.infinity, pi.infinity).astype(bool)

    def verify_weighted(self, openings, weights) -> bool:
        """"are ALL of them valid?" as ONE boolean, the sound small-exponent test (sylow_hip_kzg_batch_verify_weighted): one weight per opening,
        drawn AFTER the openings are fixed; a batch with an invalid opening passes with probability at most 2^-(bits of the weights)."""
        c, z, y, pi = openings
        return engine().kzg_batch_verify_weighted(self.tau_g2.xy, c.xy, self._words(z), self._words(y), pi.xy, self._words(weights), c.infinity, pi.infinity)[1]


    def combine(self, c: G1Affine, y, groups, gamma):
        """The folded rows of openings that share a point: with the m commitments `c` and claimed values `y` in G groups of consecutive
        polynomials (`groups`: the group SIZES, see group_offsets) and one challenge gamma_g per group, (C_F: G1Affine of G points, y_F [G, 4])
        with C_F,g = sum_j gamma_g^i C_j and y_F,g = sum_j gamma_g^i y_j, i the index inside the group
        (sylow_hip_kzg_combine_openings_batch).  (C_F, z, y_F, pi) is then the tuple verify / verify_weighted take.  gamma must have been
        drawn AFTER c and y were fixed; the library draws no challenge."""
        cf_xy, cf_inf, yf = engine().kzg_combine_openings(c.xy, self._words(y), group_offsets(groups, len(c)), self._words(gamma), c.infinity)
        return G1Affine(cf_xy, cf_inf), yf

    def verify_multi(self, c: G1Affine, y, groups, z, gamma, pi: G1Affine) -> np.ndarray:
        """ok[g] for every group: the folded row (C_F,g, z_g, y_F,g, pi_g) checked under tau_g2 (sylow_hip_kzg_verify_multi_batch); `groups`
        are the group SIZES, z and gamma hold one value per group, pi one proof per group (KzgProver.open_multi)."""
        return engine().kzg_verify_multi(self.tau_g2.xy, c.xy, self._words(y), group_offsets(groups, len(c)), self._words(z), self._words(gamma),
                                         pi.xy, c.infinity, pi.infinity).astype(bool)

    def verify_multi_weighted(self, c: G1Affine, y, groups, z, gamma, pi: G1Affine, weights) -> bool:
        """"are ALL the folded rows valid?" as ONE boolean: combine, then verify_weighted over the G rows.  One weight per group, drawn AFTER
        the proofs pi are fixed (and gamma after c and y)."""
        cf, yf = self.combine(c, y, groups, gamma)
        return self.verify_weighted((cf, self._words(z), yf, pi), weights)


class KzgPointsVerifier:
    """The verifier's key for openings of one polynomial at k points under one proof: srs_g1 = (tau^i G1gen) for i < k and srs_g2 =
    (tau^i G2gen) for i <= k, in G2 proper; longer arrays are cut to what a call's k needs.  The library draws no challenge and takes the SRS
    as given: the key is trusted input, and the points z are the caller's."""

    def __init__(self, srs_g1: G1Affine, srs_g2: G2Affine):
        if len(srs_g1) < 1 or len(srs_g2) != len(srs_g1) + 1 or srs_g1.infinity.any() or srs_g2.infinity.any():
            raise ValueError("KzgPointsVerifier: k >= 1 powers in G1, k + 1 powers in G2, no identity among them")
        self.srs_g1, self.srs_g2 = srs_g1, srs_g2

    @staticmethod
    def _rows(v):
        a = np.asarray(v)
        if a.dtype == object or a.ndim == 2:
            rows = [list(r) for r in v]
            a = fp([int(x) for r in rows for x in r]).reshape(len(rows), -1, 4) if rows else np.zeros((0, 1, 4), dtype=np.uint64)
        if a.ndim != 3 or a.shape[2] != 4 or a.shape[1] < 1:
            raise ValueError("z, y: [n, k, 4] words or n rows of k integers, k >= 1")
        return a

    def verify(self, c: G1Affine, z, y, pi: G1Affine) -> np.ndarray:
        """ok[j] = [ e(C_j - R_j(tau) G1gen, G2gen) e(-pi_j, Z_j(tau) G2gen) == 1 ] and the k points of row j are distinct mod r, with
        Z_j = prod_i (X - z[j, i]) and R_j the interpolant of the y[j, i] (sylow_hip_kzg_verify_points_batch).  A flagged pi (a zero
        quotient) is legal: the row is then valid iff C_j = R_j(tau) G1gen.  Points are taken as given."""
        z, y = self._rows(z), self._rows(y)
        k = z.shape[1]
        if k > len(self.srs_g1):
            raise ValueError(f"KzgPointsVerifier: the key holds {len(self.srs_g1)} powers, the rows have {k} points")
        return engine().kzg_verify_points(self.srs_g1.xy[:k], self.srs_g2.xy[:k + 1], c.xy, z, y, pi.xy, c.infinity, pi.infinity).astype(bool)


class KzgCosetVerifier:
    """The verifier's key for openings of one polynomial on a coset of l = 2^log_l points of its domain of n = 2^(log_c + log_l) under one
    proof (KzgProver.open_cosets): srs_g1_prefix = (tau^k G1gen) for k < l (a longer array is cut) and tau_l_g2 = tau^l G2gen, one point of
    G2 proper.  A row is (C, idx, cell, pi): the cell holds the l values of the polynomial committed in C on coset idx < c, in the order
    w_n^(idx + c t).  Each row reduces to a single-point opening (C - R(tau) G1gen, v^idx, 0, pi) under tau_l_g2, R the interpolant of the
    cell, so ONE G2 point and one line table serve the whole batch.  The key is trusted input; the library makes no G2 powers."""

    def __init__(self, srs_g1_prefix: G1Affine, tau_l_g2: G2Affine, log_c: int, log_l: int):
        log_c, log_l = int(log_c), int(log_l)
        if log_c < 0 or log_l < 0 or log_c + log_l > 27:
            raise ValueError("KzgCosetVerifier: log_c >= 0, log_l >= 0, log_c + log_l <= 27")
        if len(srs_g1_prefix) < 1 << log_l or srs_g1_prefix.infinity[:1 << log_l].any():
            raise ValueError("KzgCosetVerifier: 2^log_l powers in G1, no identity among them")
        self.srs_g1 = G1Affine(srs_g1_prefix.xy[:1 << log_l], srs_g1_prefix.infinity[:1 << log_l])
        self._single = KzgVerifier(tau_l_g2)          # the single-point verifier under tau^l G2gen, with its cached line table
        self.log_c, self.log_l = log_c, log_l

    def _cells(self, idx, cells):
        idx = np.ascontiguousarray([int(i) for i in np.asarray(idx, dtype=object).reshape(-1)], dtype=np.uint64)
        a = np.asarray(cells)
        if a.dtype == object or a.ndim == 2:
            rows = [list(r) for r in cells]
            a = fp([int(x) for r in rows for x in r]).reshape(len(rows), -1, 4) if rows else np.zeros((0, 1 << self.log_l, 4), dtype=np.uint64)
        if a.ndim != 3 or a.shape != (idx.shape[0], 1 << self.log_l, 4):
            raise ValueError("cells: [rows, 2^log_l, 4] words or rows of 2^log_l integers, one row per index")
        return idx, a

    def reduce(self, c: G1Affine, idx, cells):
        """(C - R(tau) G1gen: G1Affine, z [rows, 4] = v^idx, in_range [rows] bool): the rows KzgVerifier(tau_l_g2) takes with y = 0
        (sylow_hip_kzg_cosets_reduce_batch); words as for idx mod c where idx >= c, and in_range False there."""
        idx, a = self._cells(idx, cells)
        xy, inf, z, ok = engine().kzg_cosets_reduce(self.srs_g1.xy, c.xy, idx, a, self.log_c, self.log_l, c.infinity)
        return G1Affine(xy, inf), z, ok.astype(bool)

    def verify(self, c: G1Affine, idx, cells, pi: G1Affine) -> np.ndarray:
        """ok[j] = [ e(C_j - R_j(tau) G1gen, G2gen) e(-pi_j, tau^l G2gen - v^idx_j G2gen) == 1 ] and idx_j < c
        (sylow_hip_kzg_verify_cosets_batch).  A flagged pi (a zero quotient) is legal: the row is then valid iff C_j = R_j(tau) G1gen."""
        idx, a = self._cells(idx, cells)
        return engine().kzg_verify_cosets(self.srs_g1.xy, self._single.tau_g2.xy, c.xy, idx, a, pi.xy, self.log_c, self.log_l, c.infinity, pi.infinity).astype(bool)

    def verify_line_table(self, c: G1Affine, idx, cells, pi: G1Affine) -> np.ndarray:
        """The same flags over the cached line table of tau^l G2gen: reduce, then sylow_hip_kzg_verify_line_table_batch."""
        cred, z, ok = self.reduce(c, idx, cells)
        return self._single.verify((cred, z, np.zeros_like(z), pi)) & ok

    def verify_weighted(self, c: G1Affine, idx, cells, pi: G1Affine, weights) -> bool:
        """"are ALL the rows valid?" as ONE boolean: reduce, then the small-exponent test of KzgVerifier.verify_weighted on the reduced
        rows; one weight per row, drawn AFTER the rows are fixed.  False when a row with a non-zero weight (mod r) names no coset."""
        cred, z, ok = self.reduce(c, idx, cells)
        w = KzgVerifier._words(weights)
        live = np.array([x % R_ORDER != 0 for x in _ints(w)], dtype=bool)
        if (live & ~ok).any():
            return False
        return self._single.verify_weighted((cred, z, np.zeros_like(z), pi), w)


class KzgCellBatchVerifier:
    """The sampling node's question -- "are these N cells of B blobs, B << N, all valid?" -- answered ONCE over shared commitments
    (include/sylow_hip_kzg_cells.h).  The key is KzgCosetVerifier's: srs_g1_prefix = (tau^k G1gen) for k < l and tau_l_g2 = tau^l G2gen.
    Row k is (com_idx[k] < len(commitments), idx[k] < c, cells[k], pi[k], weights[k]); the weighted sums are taken in Fr before anything
    touches the curve: one commitment of l terms for the whole batch where KzgCosetVerifier.verify_weighted commits l terms per row.
    Weights are drawn by the caller AFTER the rows are fixed; the library draws none.  A weight of 0 removes a row, so a bad cell is
    localised by masking weights.  A row that names no cell or no commitment adds nothing and fails the check unless its weight is 0."""

    def __init__(self, srs_g1_prefix: G1Affine, tau_l_g2: G2Affine, log_c: int, log_l: int):
        self._coset = KzgCosetVerifier(srs_g1_prefix, tau_l_g2, log_c, log_l)      # the same key, checked the same way
        self.srs_g1, self._single, self.log_c, self.log_l = self._coset.srs_g1, self._coset._single, self._coset.log_c, self._coset.log_l

    def _rows(self, com_idx, idx, cells, weights):
        idx, a = self._coset._cells(idx, cells)
        com_idx = np.ascontiguousarray([int(i) for i in np.asarray(com_idx, dtype=object).reshape(-1)], dtype=np.uint64)
        w = KzgVerifier._words(weights) if len(idx) else np.zeros((0, 4), dtype=np.uint64)
        if com_idx.shape[0] != idx.shape[0] or w.shape != (idx.shape[0], 4):
            raise ValueError("KzgCellBatchVerifier: one commitment index and one weight per row")
        return com_idx, idx, a, w

    def fold(self, n_com: int, com_idx, idx, cells, weights):
        """(W [n_com, 4], A [l, 4], r [rows, 4], rz [rows, 4], in_range: bool): the Fr half (sylow_hip_kzg_cells_fold_batch)."""
        com_idx, idx, a, w = self._rows(com_idx, idx, cells, weights)
        return engine().kzg_cells_fold(idx, com_idx, a, w, self.log_c, self.log_l, n_com)

    def reduce(self, commitments: G1Affine, com_idx, idx, cells, pi: G1Affine, weights):
        """(F: G1Affine, P: G1Affine, in_range: bool): the batch as the one row (F, 0, 0, P) of KzgVerifier(tau_l_g2)
        (sylow_hip_kzg_cells_reduce_batch)."""
        com_idx, idx, a, w = self._rows(com_idx, idx, cells, weights)
        f, fi, p, pi_f, ok = engine().kzg_cells_reduce(self.srs_g1.xy, commitments.xy, idx, com_idx, a, pi.xy, w, self.log_c, self.log_l, commitments.infinity, pi.infinity)
        return G1Affine(f, fi), G1Affine(p, pi_f), ok

    def verify(self, commitments: G1Affine, com_idx, idx, cells, pi: G1Affine, weights) -> bool:
        """ONE boolean for the whole batch (sylow_hip_kzg_cells_verify_weighted): two Miller loops and one final exponentiation."""
        com_idx, idx, a, w = self._rows(com_idx, idx, cells, weights)
        return engine().kzg_cells_verify_weighted(self.srs_g1.xy, self._single.tau_g2.xy, commitments.xy, idx, com_idx, a, pi.xy, w, self.log_c, self.log_l,
                                                  commitments.infinity, pi.infinity)[1]

    def verify_line_table(self, commitments: G1Affine, com_idx, idx, cells, pi: G1Affine, weights) -> bool:
        """The same boolean over the cached line table of tau^l G2gen: reduce, then the one row through KzgVerifier.verify."""
        f, p, ok = self.reduce(commitments, com_idx, idx, cells, pi, weights)
        zero = np.zeros((1, 4), dtype=np.uint64)
        return bool(self._single.verify((f, zero, zero, p))[0]) and ok


class KzgCellRecovery:
    """A blob -- a polynomial of degree below n / 2 on a domain of n = 2^(log_c + log_l) points cut into c = 2^log_c cells of l = 2^log_l
    values, the cells of KzgProver.open_cosets -- from ANY c / 2 of its cells (sylow_hip_kzg_recover_batch).  It needs no SRS.  The
    extension is fixed at 2x, and the cost of the vanishing values is quadratic in c: log_c <= 12."""

    def __init__(self, log_c: int, log_l: int):
        log_c, log_l = int(log_c), int(log_l)
        if log_c < 0 or log_l < 0 or log_c > 12 or not 1 <= log_c + log_l <= 27:
            raise ValueError("KzgCellRecovery: 0 <= log_c <= 12, log_l >= 0, 1 <= log_c + log_l <= 27")
        self.log_c, self.log_l = log_c, log_l

    def _rows(self, idx, cells):
        """-> (y [m, n, 4], present [m, c]) from the indices of ONE blob or a list of index lists, and the matching rows of l values"""
        c, l = 1 << self.log_c, 1 << self.log_l
        idx = list(idx)
        if not idx or not isinstance(idx[0], (list, tuple, np.ndarray)):
            idx, cells = [idx], [cells]
        if len(cells) != len(idx):
            raise ValueError("KzgCellRecovery: one set of cells per set of indices")
        y, present = np.zeros((len(idx), l, c, 4), dtype=np.uint64), np.zeros((len(idx), c), dtype=np.uint8)
        form = KzgCosetVerifier._cells
        for j, (ix, rows) in enumerate(zip(idx, cells)):
            ix, a = form(self, ix, rows)
            if (ix >= c).any() or len(set(ix.tolist())) != len(ix):
                raise ValueError("KzgCellRecovery: cell indices below c = 2^log_c, each at most once per blob")
            present[j, ix.astype(np.int64)] = 1
            y[j, :, ix.astype(np.int64)] = a                                   # value t of cell i at y[i + c t]
        return y.reshape(len(idx), l * c, 4), present

    def recover(self, idx, cells):
        """(polys [m, n, 4] words, status [m]): idx is the list of the cell indices held of ONE blob, or a list of such lists for m blobs;
        `cells` the matching rows of l values ([rows, l, 4] words or rows of l integers).  status 0: polys[j] is the blob (upper half
        zero); 1: fewer than c / 2 cells (zero row); 2: the cells are not the values of a polynomial of degree below n / 2."""
        y, present = self._rows(idx, cells)
        coeffs, _, status = engine().kzg_recover(y, present, self.log_c, self.log_l, want_y=False)
        return coeffs, status


def group_offsets(groups, m: int) -> np.ndarray:
    """`groups` in this module is the list of group SIZES (e.g. [12, 2]: twelve polynomials opened at the first point, two at the second; a
    size of 0 is legal); the C ABI and the Engine take the G + 1 OFFSETS, which this returns.  ValueError unless the sizes add up to m."""
    sizes = [int(x) for x in groups]
    if any(x < 0 for x in sizes) or sum(sizes) != m:
        raise ValueError(f"groups: non-negative group sizes that add up to the {m} polynomials")
    return np.cumsum([0] + sizes).astype(np.uint64)


class KzgProver:
    """The prover's half of a BN254 KZG SRS: srs_g1 = (tau^k G1gen) for k = 0 .. len - 1.  `polys` below is [m, len, 4] words or m lists of
    Python ints (lowest degree first, padded with zeros to the length of the SRS by the caller if shorter) -- any 256-bit values, taken mod
    r; z as for KzgVerifier.  (commit(polys), z, *open(polys, z)) is the tuple KzgVerifier.verify takes."""

    def __init__(self, srs_g1: G1Affine):
        if len(srs_g1) < 1 or srs_g1.infinity.any():
            raise ValueError("KzgProver: srs_g1 holds at least G1gen and no identity")
        self.srs_g1 = srs_g1
        self._open_all_table = None      # open_all: built on first use
        self._open_cosets_tables = {}    # open_cosets: one table per log_l, built on first use

    def _polys(self, polys):
        a = np.asarray(polys)
        if a.dtype == object or a.ndim == 2:
            rows = [list(f) for f in polys]
            a = fp([int(v) for f in rows for v in f]).reshape(len(rows), -1, 4) if rows else np.zeros((0, len(self.srs_g1), 4), dtype=np.uint64)
        if a.ndim != 3 or a.shape[1] != len(self.srs_g1):
            raise ValueError("KzgProver: every polynomial has one coefficient per SRS point (pad with zeros)")
        return a

    def commit(self, polys) -> G1Affine:
        """C_j = sum_k f_jk srs_k (sylow_hip_kzg_commit_batch); the zero polynomial commits to the identity."""
        return G1Affine(*engine().kzg_commit(self.srs_g1.xy, self._polys(polys)))

    def open(self, polys, z):
        """(y [m, 4] words, pi: G1Affine) with y_j = f_j(z_j) and pi_j the commitment to (f_j - y_j) / (X - z_j) (sylow_hip_kzg_open_batch); a
        constant polynomial opens with the identity."""
        y, pi_xy, pi_inf = engine().kzg_open(self.srs_g1.xy, self._polys(polys), KzgVerifier._words(z))
        return y, G1Affine(pi_xy, pi_inf)

    def open_multi(self, polys, groups, z, gamma):
        """(y [m, 4] words, pi: G1Affine of G points): the polynomials in G groups of consecutive ones (`groups`: the group SIZES, see
        group_offsets), group g opened at z_g under ONE proof folded with gamma_g -- y_j = f_j(z_g) and pi_g the proof of
        F_g = sum_j gamma_g^i f_j at z_g, word for word open(F_g, z_g) (sylow_hip_kzg_open_multi_batch).  gamma must be drawn AFTER the
        commitments and the y_j are fixed.  (commit(polys), y, groups, z, gamma, pi) is what KzgVerifier.verify_multi takes."""
        a = self._polys(polys)
        y, pi_xy, pi_inf = engine().kzg_open_multi(self.srs_g1.xy, a, group_offsets(groups, a.shape[0]), KzgVerifier._words(z), KzgVerifier._words(gamma))
        return y, G1Affine(pi_xy, pi_inf)

    def open_points(self, polys, z):
        """(y [m, k, 4] words, pi: G1Affine of m points): every f_j opened at ITS k points z[j] under ONE proof -- y[j, i] = f_j(z[j, i]) and
        pi_j the commitment to f_j div prod_i (X - z[j, i]) (sylow_hip_kzg_open_points_batch); z is [m, k, 4] words or m lists of k Python
        ints, 1 <= k <= 64, the points of a row distinct mod r.  pi_j is the identity when the quotient is zero (len <= k).  The library draws
        no challenge and takes the SRS as given.  (commit(polys), z, y, pi) is what KzgPointsVerifier.verify takes."""
        y, pi_xy, pi_inf = engine().kzg_open_points(self.srs_g1.xy, self._polys(polys), KzgPointsVerifier._rows(z))
        return y, G1Affine(pi_xy, pi_inf)

    def open_all(self, polys):
        """The openings of every f_j at ALL n = len(srs_g1) = 2^log_n points of its domain at once, in n log n (sylow_hip_kzg_open_all_batch,
        the Feist-Khovratovich construction): (y [m, n, 4] words, [G1Affine] * m) with y[j, i] = f_j(w_n^i) (= ntt(polys)) and pi_j[i] word
        for word what open(f_j, w_n^i) yields.  The table that depends on the SRS alone is built on first use and kept on the device.
        ValueError unless the SRS holds a power of two of points, at most 2^27."""
        n = len(self.srs_g1)
        if n & (n - 1) or n > 1 << 27:
            raise ValueError("KzgProver.open_all: the SRS holds a power of two of points, at most 2^27")
        a = self._polys(polys)
        if self._open_all_table is None:
            self._open_all_table = engine().kzg_open_all_prepare(self.srs_g1.xy)
        y, pi_xy, pi_inf = engine().kzg_open_all(self._open_all_table, a)
        return y, [G1Affine(pi_xy[j], pi_inf[j]) for j in range(a.shape[0])]

    def open_cosets(self, polys, log_l: int):
        """Every f_j opened on ALL c cosets of its domain of n = len(srs_g1) = c l points, l = 2^log_l, ONE proof per coset, in n log n
        (sylow_hip_kzg_open_cosets_batch, the multi-proof form of Feist-Khovratovich): (cells [m, c, l, 4] words, [G1Affine of c points] * m).
        Coset i is { w_n^(i + c t) : t < l }, cells[j, i, t] = f_j(w_n^(i + c t)) (= ntt(polys)[j, i + c t]) and pi_j[i] the commitment to
        f_j div (X^l - w_n^(l i)).  The table that depends on the SRS and log_l alone is built on first use and kept on the device.
        (commit(polys)[j], i, cells[j, i], pi_j[i]) is a row KzgCosetVerifier takes.  ValueError unless n = 2^log_n <= 2^27 and l divides n."""
        n, log_l = len(self.srs_g1), int(log_l)
        if n & (n - 1) or n > 1 << 27 or log_l < 0 or (1 << log_l) > n:
            raise ValueError("KzgProver.open_cosets: the SRS holds a power of two of points, at most 2^27, and 2^log_l of them make a coset")
        a = self._polys(polys)
        if log_l not in self._open_cosets_tables:
            self._open_cosets_tables[log_l] = engine().kzg_open_cosets_prepare(self.srs_g1.xy, log_l)
        y, pi_xy, pi_inf = engine().kzg_open_cosets(self._open_cosets_tables[log_l], a, log_l)
        l, m = 1 << log_l, a.shape[0]
        cells = np.ascontiguousarray(y.reshape(m, l, n >> log_l, 4).transpose(0, 2, 1, 3))
        return cells, [G1Affine(pi_xy[j], pi_inf[j]) for j in range(m)]

    def recover_cells_and_proofs(self, idx, cells, log_l: int):
        """Every cell and every cell proof of blobs of which at least half the cells are held: KzgCellRecovery.recover, then open_cosets on
        the rows it recovered.  idx, cells as KzgCellRecovery.recover takes them.  (status [m], cells [m, c, l, 4] words, proofs: a list of
        m G1Affine of c points); a row whose status is not 0 has zero cells and None for its proofs."""
        n, log_l = len(self.srs_g1), int(log_l)
        if n & (n - 1) or n > 1 << 27 or log_l < 0 or (1 << log_l) > n:
            raise ValueError("KzgProver.recover_cells_and_proofs: the SRS holds a power of two of points, at most 2^27, and 2^log_l of them make a cell")
        polys, status = KzgCellRecovery(n.bit_length() - 1 - log_l, log_l).recover(idx, cells)
        good = np.flatnonzero(status == 0)
        out = np.zeros((polys.shape[0], n >> log_l, 1 << log_l, 4), dtype=np.uint64)
        proofs = [None] * polys.shape[0]
        if good.size:
            out[good], pis = self.open_cosets(polys[good], log_l)
            for j, pi in zip(good, pis):
                proofs[j] = pi
        return status, out, proofs

    def commit_evals(self, evals) -> G1Affine:
        """The same commitments from the VALUES of the polynomials on the domain of len(srs_g1) = 2^log_n points, evals[j][i] = f_j(w_n^i)
        (sylow_hip_kzg_commit_evals_batch): word for word commit(intt(evals))."""
        n = len(self.srs_g1)
        if n & (n - 1):
            raise ValueError("KzgProver.commit_evals: the SRS holds a power of two of points")
        return G1Affine(*engine().kzg_commit_evals(self.srs_g1.xy, self._polys(evals)))

    def lagrange_srs(self) -> G1Affine:
        """The Lagrange-basis SRS L_i(tau) G1gen of the domain of len(srs_g1) = 2^log_n points: the inverse G1 transform of the monomial SRS
        (sylow_hip_kzg_srs_lagrange).  ValueError when tau lies in the domain (some L_i(tau) = 0: an identity comes back)."""
        n = len(self.srs_g1)
        if n & (n - 1) or n > 1 << 28:
            raise ValueError("KzgProver.lagrange_srs: the SRS holds a power of two of points, at most 2^28")
        xy, inf = engine().kzg_srs_lagrange(self.srs_g1.xy)
        if inf.any():
            raise ValueError("KzgProver.lagrange_srs: tau lies in the domain, the Lagrange-basis SRS holds an identity and is unusable")
        return G1Affine(xy, inf)

    def eval_prover(self) -> "KzgEvalProver":
        """The prover for polynomials held in evaluation form under the same tau."""
        return KzgEvalProver(self.lagrange_srs())


class KzgEvalProver:
    """The prover's half of a BN254 KZG SRS for polynomials held in EVALUATION form: srs_lagrange = (L_i(tau) G1gen) for i = 0 .. n - 1, with L_i
    the Lagrange basis of the domain <w_n> of n = 2^log_n points (the domain of ntt).  `evals` below is [m, n, 4] words or m lists of n Python
    ints, evals[j][i] = f_j(w_n^i) -- any 256-bit values, taken mod r; z as for KzgVerifier, inside the domain or not.
    (commit(evals), z, *open(evals, z)) is the tuple KzgVerifier.verify takes, word for word what KzgProver yields for the interpolated
    coefficients under the monomial SRS of the same tau."""

    def __init__(self, srs_lagrange: G1Affine):
        n = len(srs_lagrange)
        if n < 1 or n & (n - 1) or n > 1 << 28 or srs_lagrange.infinity.any():
            raise ValueError("KzgEvalProver: srs_lagrange holds a power of two of points, at most 2^28, and no identity")
        self.srs_lagrange = srs_lagrange

    def _evals(self, evals):
        a = np.asarray(evals)
        n = len(self.srs_lagrange)
        if a.dtype == object or a.ndim == 2:
            rows = [list(f) for f in evals]
            a = fp([int(v) for f in rows for v in f]).reshape(len(rows), -1, 4) if rows else np.zeros((0, n, 4), dtype=np.uint64)
        if a.ndim != 3 or a.shape[1] != n:
            raise ValueError("KzgEvalProver: every polynomial has one value per SRS point")
        return a

    def commit(self, evals) -> G1Affine:
        """C_j = sum_i f_j(w^i) srs_lagrange_i = f_j(tau) G1gen: sylow_hip_kzg_commit_batch over the values as they lie."""
        return G1Affine(*engine().kzg_commit(self.srs_lagrange.xy, self._evals(evals)))

    def evaluate(self, evals, z) -> np.ndarray:
        """y [m, 4] words, y_j = f_j(z_j), by the barycentric formula (sylow_hip_kzg_quotient_evals_batch without a quotient buffer)."""
        return engine().kzg_quotient_evals(self._evals(evals), KzgVerifier._words(z), want_q=False)[1]

    def quotient(self, evals, z):
        """(q [m, n, 4], y [m, 4]): the values on the domain of (f_j - y_j) / (X - z_j), and y_j (sylow_hip_kzg_quotient_evals_batch)."""
        return engine().kzg_quotient_evals(self._evals(evals), KzgVerifier._words(z))

    def open(self, evals, z):
        """(y [m, 4] words, pi: G1Affine) with pi_j the commitment to the quotient's values (sylow_hip_kzg_open_evals_batch); a constant
        polynomial opens with the identity."""
        y, pi_xy, pi_inf = engine().kzg_open_evals(self.srs_lagrange.xy, self._evals(evals), KzgVerifier._words(z))
        return y, G1Affine(pi_xy, pi_inf)

    def open_multi(self, evals, groups, z, gamma):
        """KzgProver.open_multi from evaluation form (sylow_hip_kzg_open_multi_evals_batch): the same words as for the interpolated
        coefficients under the monomial SRS of the same tau; z_g inside the domain or not.  `groups`: the group SIZES."""
        a = self._evals(evals)
        y, pi_xy, pi_inf = engine().kzg_open_multi_evals(self.srs_lagrange.xy, a, group_offsets(groups, a.shape[0]), KzgVerifier._words(z),
                                                         KzgVerifier._words(gamma))
        return y, G1Affine(pi_xy, pi_inf)


class PlonkPermutation:
    """The copy-constraint argument of a PLONK-style prover over the domain <w_n> of n = 2^log_n points (the domain of ntt): W wire columns, the
    identity columns shifts[j] w_n^i and the permutation columns sigma [W, n, 4], which hold the identity values permuted along the copy cycles.
    `shifts`: W coset representatives as [W, 4] words or Python ints (k_j with the cosets k_j <w_n> disjoint, e.g. 1, 5, 7, ...).
    THE LIBRARY DRAWS NO CHALLENGE: beta and gamma are the caller's, drawn AFTER the wire commitments are fixed."""

    def __init__(self, log_n: int, shifts, sigma):
        self.log_n, self.shifts = int(log_n), _words(shifts)
        self.sigma = np.ascontiguousarray(sigma, dtype=np.uint64)
        W = self.shifts.shape[0]
        if not 0 <= self.log_n <= 28 or not 1 <= W <= 32 or self.sigma.shape != (W, 1 << self.log_n, 4):
            raise ValueError("PlonkPermutation: log_n in 0 .. 28, 1 .. 32 columns, sigma [W, n, 4]")

    @classmethod
    def from_mapping(cls, log_n: int, shifts, mapping):
        """sigma from a permutation of the W n positions, position j n + i being row i of column j: sigma at position p is the identity value
        of position mapping[p].  The identity columns come from the device (sylow_hip_plonk_identity_batch); the gather runs on the host."""
        sh = _words(shifts)
        n, W = 1 << int(log_n), sh.shape[0]
        mp = np.ascontiguousarray(mapping, dtype=np.int64).reshape(-1)
        if mp.shape[0] != W * n or not np.array_equal(np.sort(mp), np.arange(W * n)):
            raise ValueError("PlonkPermutation.from_mapping: mapping is a permutation of the W n positions")
        ident = engine().plonk_identity(sh, int(log_n)).reshape(W * n, 4)
        return cls(log_n, sh, ident[mp].reshape(W, n, 4))

    def grand_product(self, wires, beta, gamma):
        """(z [m, n, 4] canonical words, status [m]) for wires [m, W, n, 4] (or [W, n, 4]: one instance) and one (beta, gamma) per instance
        (sylow_hip_plonk_permutation_batch): z[j, 0] = 1 and z[j, i + 1] = z[j, i] num_i / den_i; status 0 = the copy constraints hold, bit 0 =
        a zero denominator, bit 1 = z does not close to 1.  z is the argument KzgProver.commit_evals takes."""
        w = np.ascontiguousarray(wires, dtype=np.uint64)
        w = w[None] if w.ndim == 3 else w
        z, _, status = engine().plonk_permutation(w, self.sigma, self.shifts, _words(beta), _words(gamma))
        return z, status


class PlonkQuotient:
    """The quotient polynomial of a PLONK-style prover for ONE circuit over the domain <w_n>, n = 2^log_n, formed on the coset 5 <w_N> of
    N = 2^log_e n points: t = [gate + alpha perm + alpha^2 L_1 (z - 1)] / (X^n - 1) with gate = q_M w_0 w_1 + sum_j q_j w_j + q_C + PI and perm
    the two products of the copy-constraint argument (include/sylow_plonk.h).  `shifts` and `sigma` are PlonkPermutation's; `selectors` holds
    the values on <w_n> of q_0 .. q_(W-1), q_M, q_C as [W + 2, n, 4] words or W + 2 lists of Python ints.  The circuit's table is built once,
    here, and stays on the device.  THE LIBRARY DRAWS NO CHALLENGE: beta and gamma are drawn AFTER the wire commitments are fixed, alpha AFTER
    the commitment to z is fixed."""

    def __init__(self, log_n: int, shifts, sigma, selectors, log_e: int = 2):
        perm = PlonkPermutation(log_n, shifts, sigma)                  # its validation of log_n, the shifts and sigma
        self.log_n, self.log_e, self.shifts, self.sigma = perm.log_n, int(log_e), perm.shifts, perm.sigma
        self.W = self.shifts.shape[0]
        sel = _fr_nd(selectors, 2)
        if self.W < 2 or self.log_e < 0 or self.log_n + self.log_e > 28 or sel.shape != (self.W + 2, 1 << self.log_n, 4):
            raise ValueError("PlonkQuotient: 2 .. 32 columns, log_n + log_e <= 28, selectors [W + 2, n, 4]")
        self.table = engine().plonk_quotient_prepare(sel, self.sigma, self.log_e)

    def quotient(self, wires, z, beta, gamma, alpha, pi=None):
        """(t [m, N, 4] canonical words, status [m]) for the COEFFICIENTS of the wires [m, W, len_w, 4] (or [W, len_w, 4]: one instance), of
        z [m, len_z, 4] and of the public-input polynomial pi [m, n, 4] (or None), as words or as nested lists of Python ints, and one
        (beta, gamma, alpha) per instance (sylow_plonk_quotient_batch).  len_w and len_z are free in 1 .. N: blinded polynomials are longer
        than n.  status 0 = no coefficient of t above its degree bound; bit 0 = X^n - 1 does not divide, the constraints do not hold."""
        w = _fr_nd(wires, 3, 2)
        w = w[None] if w.ndim == 3 else w
        zc = _fr_nd(z, 2, 1)
        zc = zc[None] if zc.ndim == 2 else zc
        pc = None
        if pi is not None:
            pc = _fr_nd(pi, 2, 1)
            pc = pc[None] if pc.ndim == 2 else pc
        return engine().plonk_quotient(self.table, w, zc, pc, self.shifts, _words(beta), _words(gamma), _words(alpha), self.log_n, self.log_e)


class PlonkOpening:
    """The closing rounds of a PLONK-style prover for ONE circuit (include/sylow_popen.h): the evaluations at zeta, the linearisation
    polynomial r, the fold F = r + sum_j v^(1+j) w_j + sum_j v^(W+1+j) sigma_j and the proofs W_zeta (F at zeta) and W_omega (z at
    zeta w_n).  The arguments are PlonkQuotient's; log_e names the N = 2^log_e n coefficients of t as PlonkQuotient.quotient returns it.
    The circuit's coefficient table is built once, here, and stays on the device; every instance reads it in place.  THE LIBRARY DRAWS NO
    CHALLENGE: zeta is drawn AFTER the commitments to the chunks of t are fixed, v AFTER the evaluations are fixed."""

    def __init__(self, log_n: int, shifts, sigma, selectors, log_e: int = 2):
        perm = PlonkPermutation(log_n, shifts, sigma)                  # its validation of log_n, the shifts and sigma
        self.log_n, self.log_e, self.shifts, self.sigma = perm.log_n, int(log_e), perm.shifts, perm.sigma
        self.W = self.shifts.shape[0]
        sel = _fr_nd(selectors, 2)
        if self.W < 2 or self.log_e < 0 or self.log_n + self.log_e > 28 or sel.shape != (self.W + 2, 1 << self.log_n, 4):
            raise ValueError("PlonkOpening: 2 .. 32 columns, log_n + log_e <= 28, selectors [W + 2, n, 4]")
        self.ctable = engine().plonk_open_prepare(sel, self.sigma)

    @staticmethod
    def _batch(values, ndim):
        if values is None:
            return None
        a = _fr_nd(values, ndim - 1, ndim - 2)                        # ndim: the dimensions of the batch as words, [m, .., 4]
        return a[None] if a.ndim == ndim - 1 else a

    def evaluate(self, wires, z, zeta, pi=None):
        """evals [m, 2 W + 1, 4] canonical words for the COEFFICIENTS of the wires [m, W, len_w, 4] (or [W, len_w, 4]: one instance), of z
        and of the public-input polynomial pi (or None), as words or nested lists of Python ints, and one zeta per instance
        (sylow_popen_evaluate_batch): w_j(zeta), sigma_j(zeta) for j < W - 1, z(zeta w_n), PI(zeta)."""
        return engine().plonk_open_evaluate(self.ctable, self._batch(wires, 4), self._batch(z, 3), self._batch(pi, 3), _words(zeta))

    def linearise(self, wires, z, t, evals, beta, gamma, alpha, zeta, v=None):
        """(r, F or None, status [m]) as [m, max(n, len_z[, len_w]), 4] canonical words (sylow_popen_linearise_batch): t [m, N, 4] as
        PlonkQuotient.quotient returns it, evals as evaluate returns them.  v None: r alone.  status 0 = r(zeta) = 0 and zeta outside the
        domain; bit 0 = r(zeta) != 0, bit 1 = zeta^n = 1."""
        want_f = v is not None
        return engine().plonk_open_linearise(self.ctable, self._batch(wires, 4) if want_f else None, self._batch(z, 3), self._batch(t, 3), self._batch(evals, 3),
                                             self.shifts, _words(beta), _words(gamma), _words(alpha), _words(zeta), _words(v) if want_f else None, self.log_e,
                                             want_f=want_f)

    def open(self, prover: "KzgProver", wires, z, t, beta, gamma, alpha, zeta, v, pi=None):
        """(evals [m, 2 W + 1, 4], w_zeta: G1Affine, w_omega: G1Affine, status [m]) under the prover's SRS, which holds at least
        max(n, len_z, len_w) powers (sylow_popen_open_batch).  (commit(F), zeta, F(zeta), w_zeta) and (commit(z), zeta w_n, evals[:, 2 W - 1],
        w_omega) are rows KzgVerifier.verify accepts.  v IS TAKEN BESIDE zeta: a caller whose v depends on the evaluations calls evaluate,
        linearise and KzgProver.open instead."""
        ev, (p1, f1), (p2, f2), status = engine().plonk_open(prover.srs_g1.xy, self.ctable, self._batch(wires, 4), self._batch(z, 3), self._batch(pi, 3),
                                                             self._batch(t, 3), self.shifts, _words(beta), _words(gamma), _words(alpha), _words(zeta), _words(v),
                                                             self.log_e)
        return ev, G1Affine(p1, f1), G1Affine(p2, f2), status


class PlonkVerifier:
    """The verifier of many proofs of ONE circuit (include/sylow_pverify.h): `vk` is a G1Affine of the 2 W + 2 commitments [q_0] .. [q_(W-1)],
    [q_M], [q_C], [sigma_0] .. [sigma_(W-1)] (key_from derives them), `tau_g2` a G2Affine of one point in G2 proper, log_e names the
    E = 2^log_e chunks of t a proof commits to.  The key and tau_g2 stay on the device.  A batch of m proofs is `proofs`, a G1Affine of
    m (W + E + 3) points, proof-major: [w_0] .. [w_(W-1)], [z], [t_0] .. [t_(E-1)], W_zeta, W_omega of proof 0, then of proof 1;
    `evals` [m, 2 W + 1, 4] as PlonkOpening.open returns them (slot 2 W is not read); `pub` [m, l, 4] words or m lists of l Python ints, the
    values of PI on rows 0 .. l - 1 (None: no public inputs).  THE LIBRARY DRAWS NO CHALLENGE: beta, gamma, alpha, zeta and v are those of
    the transcript, u is drawn AFTER W_zeta and W_omega are fixed, the weights AFTER all proofs are fixed."""

    def __init__(self, log_n: int, shifts, vk: "G1Affine", tau_g2: "G2Affine", log_e: int = 2):
        self.log_n, self.log_e, self.shifts = int(log_n), int(log_e), _words(shifts)
        self.W = self.shifts.shape[0]
        if not 2 <= self.W <= 32 or self.log_n < 0 or self.log_e < 0 or self.log_n + self.log_e > 28 or len(vk) != 2 * self.W + 2 or len(tau_g2) != 1:
            raise ValueError("PlonkVerifier: 2 .. 32 columns, log_n + log_e <= 28, a key of 2 W + 2 points, one tau_g2")
        self.vk = engine().plonk_verify_key_up(vk.xy, vk.infinity)
        self.tau_g2 = engine().to_device_soa(tau_g2.xy, 16)

    @classmethod
    def key_from(cls, prover: "KzgProver", ctable) -> "G1Affine":
        """The verifying key of a circuit: the commitments to the rows of a PlonkOpening's coefficient table (a DeviceArray [2 W + 2, 4, n], or
        rows [2 W + 2, n, 4] as words) under the prover's SRS, by KzgProver.commit.  A row that is the zero polynomial gives the identity."""
        rows = ctable if isinstance(ctable, np.ndarray) else engine().plonk_open_ctable_down(ctable)
        n, have = rows.shape[1], len(prover.srs_g1)
        if have < n:
            raise ValueError("PlonkVerifier.key_from: the SRS holds fewer powers than a row has coefficients")
        return prover.commit(np.concatenate([rows, np.zeros((rows.shape[0], have - n, 4), dtype=np.uint64)], axis=1))

    def _args(self, proofs, evals, pub, challenges):
        ev = _fr_nd(evals, 2)
        m, slots = ev.shape[0], self.W + (1 << self.log_e) + 3
        if ev.shape[1] != 2 * self.W + 1 or len(proofs) != m * slots:
            raise ValueError("PlonkVerifier: evals [m, 2 W + 1, 4] and m (W + E + 3) proof points, proof-major")
        pb = None if pub is None else _fr_nd(pub, 2)
        return (self.vk, proofs.xy.reshape(m, slots, 8), ev, pb, self.shifts) + tuple(_words(c) for c in challenges), proofs.infinity.reshape(m, slots)

    def verify(self, proofs: "G1Affine", evals, pub, beta, gamma, alpha, zeta, v, u):
        """(ok [m] bool, status [m]): ok_i = proof i verifies (sylow_pverify_verify_batch); status bit 1 = zeta_i^n = 1, and ok_i is False."""
        args, inf = self._args(proofs, evals, pub, (beta, gamma, alpha, zeta, v, u))
        ok, status = engine().plonk_verify(self.tau_g2, *args, self.log_n, self.log_e, proof_inf=inf)
        return ok.astype(bool), status

    def verify_weighted(self, proofs: "G1Affine", evals, pub, beta, gamma, alpha, zeta, v, u, weights) -> bool:
        """all m proofs as one boolean (sylow_pverify_batch_verify_weighted): a weight of 0 mod r removes a proof; a proof whose zeta lies in
        the domain makes it False unless its weight is 0."""
        args, inf = self._args(proofs, evals, pub, (beta, gamma, alpha, zeta, v, u))
        return engine().plonk_batch_verify_weighted(self.tau_g2, *args, _words(weights), self.log_n, self.log_e, proof_inf=inf)[1]


class Poseidon:
    """Poseidon over Fr of width t = 2 .. 17 as circomlib deploys it (include/sylow_poseidon.h): x^5, 8 full rounds, R_P by width, the
    parameters from the paper's Grain generator.  The parameter table stays on the device (`table`).  Values are [.., 4] words or Python
    ints, any 256-bit value taken mod r; results are canonical words."""

    def __init__(self, t: int):
        if not 2 <= int(t) <= 17:
            raise ValueError("Poseidon: t = 2 .. 17")
        self.t = int(t)
        self.table = engine().poseidon_table(self.t)

    def hash(self, inputs, init=None) -> np.ndarray:
        """hash of every row of t - 1 inputs, [n, t - 1, 4] words or n lists of ints: [n, 4].  init [n, 4]: circomlibjs's initState."""
        a = _fr_nd(inputs, 2)
        if a.shape[1] != self.t - 1:
            raise ValueError(f"Poseidon({self.t}).hash: rows of {self.t - 1} inputs")
        return engine().poseidon_hash(self.table, a, None if init is None else _words(init))

    def permute(self, states) -> np.ndarray:
        """the permutation of every state, [n, t, 4] words or n lists of t ints: [n, t, 4]"""
        a = _fr_nd(states, 2)
        if a.shape[1] != self.t:
            raise ValueError(f"Poseidon({self.t}).permute: states of {self.t} elements")
        return engine().poseidon_permute(self.table, a)


class PoseidonMerkleTree:
    """m binary Merkle trees of 2^depth leaves each, node = Poseidon hash([left, right]) (include/sylow_poseidon.h).  build keeps leaves
    and nodes on the device; open gathers paths from them; root_of and verify walk paths and need no tree."""

    def __init__(self, depth: int, hasher: "Poseidon | None" = None):
        if not 1 <= int(depth) <= 28:
            raise ValueError("PoseidonMerkleTree: depth 1 .. 28")
        self.depth = int(depth)
        self.hasher = hasher if hasher is not None else Poseidon(3)
        if self.hasher.t != 3:
            raise ValueError("PoseidonMerkleTree: the hasher of a binary tree is Poseidon(3)")
        self.m, self._leaves, self._nodes, self.roots = 0, None, None, None

    def build(self, leaves) -> np.ndarray:
        """leaves [m, 2^depth, 4] words or m lists of ints (one tree: [2^depth, 4] or one list): the roots [m, 4]"""
        a = _fr_arrays(leaves)
        a = np.ascontiguousarray(a[None] if a.ndim == 2 else a)
        if a.shape[1] != 1 << self.depth:
            raise ValueError("PoseidonMerkleTree.build: 2^depth leaves per tree")
        e = engine()
        self.m = a.shape[0]
        self._leaves = e.to_device(np.ascontiguousarray(a.transpose(0, 2, 1))) if self.m else None
        self._nodes, droot = e.poseidon_merkle_build_device(self.hasher.table, self._leaves, self.depth, self.m)
        self.roots = e.from_device_soa(droot)[:self.m]
        return self.roots

    def open(self, index, tree=None):
        """(siblings [q, depth, 4], status [q]) of the leaves `index` of the trees `tree` (None: tree 0); status bit 0 = out of range"""
        index = np.asarray(index, dtype=np.uint64).reshape(-1)
        tree = np.zeros_like(index) if tree is None else np.asarray(tree, dtype=np.uint64).reshape(-1)
        return engine().poseidon_merkle_open(self._leaves, self._nodes, self.depth, self.m, tree, index)

    def root_of(self, leaf, index, siblings):
        """(roots [q, 4], status [q]) of q paths: leaf [q, 4], index [q], siblings [q, depth, 4]"""
        return engine().poseidon_merkle_root(self.hasher.table, _words(leaf), index, siblings)

    def verify(self, leaf, index, siblings, roots=None) -> np.ndarray:
        """ok [q] bool: path i leads to roots (one root [4] / [1, 4] for all, or [q, 4]; None: the root of tree 0 of the last build)"""
        roots = self.roots[:1] if roots is None else _words(roots)
        ok, _ = engine().poseidon_merkle_verify(self.hasher.table, _words(leaf), index, siblings, roots)
        return ok.astype(bool)


def _fr_nd(values, *ndims):
    """words [..., 4] from a uint64 array of words or from nested lists of Python ints with one of the given numbers of dimensions"""
    if isinstance(values, np.ndarray) and values.dtype == np.uint64:
        if values.ndim - 1 not in ndims or values.shape[-1] != 4:
            raise ValueError(f"words as a uint64 array [..., 4] over {' or '.join(map(str, ndims))} dimensions, not {values.shape}")
        return np.ascontiguousarray(values)
    a = np.asarray(values, dtype=object)
    if a.ndim not in ndims:
        raise ValueError(f"Python ints nested {' or '.join(map(str, ndims))} deep, not {a.ndim}")
    return fp(list(a.reshape(-1))).reshape(a.shape + (4,))


def _words(v):
    """[k, 4] words from words or from Python ints"""
    a = np.asarray(v)
    if a.dtype == np.uint64 and a.ndim >= 1 and a.shape[-1] == 4:
        return np.ascontiguousarray(a).reshape(-1, 4)
    return fp([int(x) for x in np.asarray(v, dtype=object).reshape(-1)])


def _fr_arrays(values):
    """a numpy uint64 array is words ([m, n, 4] or [n, 4]); anything else is Python ints, [m][n] or [n]"""
    if isinstance(values, np.ndarray) and values.dtype == np.uint64:
        return values
    a = np.asarray(values, dtype=object)
    if a.ndim not in (1, 2):
        raise ValueError("ntt: ints as [n] or [m][n], words as a uint64 array [n, 4] or [m, n, 4]")
    words = fp(list(a.reshape(-1)))
    return words.reshape(a.shape + (4,))


def fr_lincomb(arrays, weights, groups) -> np.ndarray:
    """out_g = sum_{j in group g} weights_j a_j over Fr: `arrays` [m, len, 4] words or m lists of Python ints, one weight per array, `groups`
    the group SIZES (see group_offsets); [G, len, 4] canonical words, zeros for an empty group (sylow_hip_fr_lincomb_batch).  The fold of a
    KZG multi-opening with weights = the powers of gamma, a linearisation polynomial with arbitrary weights."""
    a = _fr_arrays(arrays)
    if a.ndim != 3:
        raise ValueError("fr_lincomb: m arrays of one length")
    return engine().fr_lincomb(a, KzgVerifier._words(weights), group_offsets(groups, a.shape[0]))


def ntt(values, shift=None, inverse: bool = False, stages: int = -1) -> np.ndarray:
    """The values on the domain <w_n> (on the coset g <w_n> with shift = g) of the polynomials whose coefficients are `values`: [m, n, 4] or
    [n, 4] words, or (lists of) Python ints, n = 2^log_n <= 2^28, natural order in and out: out_i = sum_k a_k (g w_n^i)^k with
    w_n = W^(2^(28 - log_n)), W = 5^((r - 1) / 2^28) (sylow_hip_fr_ntt_batch).  Canonical words in the shape of the input."""
    sh = None if shift is None else (fp([int(shift)])[0] if isinstance(shift, int) else np.asarray(shift, dtype=np.uint64).reshape(4))
    return engine().fr_ntt(_fr_arrays(values), inverse=inverse, shift=sh, stages=stages)


def intt(values, shift=None, stages: int = -1) -> np.ndarray:
    """The inverse of ntt: out_k = n^-1 g^-k sum_i a_i w_n^(-ik).  shift = 0 mod r uses inv(0) = 0."""
    return ntt(values, shift=shift, inverse=True, stages=stages)


def g1_ntt(points, inverse: bool = False):
    """The transform of ntt with G1 points as elements: `points` is a G1Affine of n = 2^log_n <= 2^28 points or a list of m of them (equal
    lengths), natural order in and out: out_i = sum_k w_n^(ik) P_k (sylow_hip_g1_ntt_batch).  For P_k = s_k G that is ntt(s)_i G.  A G1Affine
    (or a list of them) in canonical words, identities as (0, 1) + their flag."""
    one = isinstance(points, G1Affine)
    batch = [points] if one else list(points)
    if not batch:
        return []
    n = len(batch[0])
    if n < 1 or n & (n - 1) or n > 1 << 28 or any(len(p) != n for p in batch):
        raise ValueError("g1_ntt: every array holds the same power of two of points, at most 2^28")
    xy, inf = engine().g1_ntt(np.stack([p.xy for p in batch]), np.stack([p.infinity for p in batch]), inverse=inverse)
    out = [G1Affine(xy[j], inf[j]) for j in range(len(batch))]
    return out[0] if one else out


def g1_intt(points):
    """The inverse of g1_ntt: out_k = n^-1 sum_i w_n^(-ik) P_i."""
    return g1_ntt(points, inverse=True)


class KeyPair:
    """KeyPair (lib.rs:105-137), a batch of them: secret_key = Fp::new(Fr::rand().value()) -- a scalar below r held as an Fp --
    and public_key = G2Projective::generator() * secret_key."""

    def __init__(self, secret_key: np.ndarray, public_key: "G2Affine"):
        self.secret_key, self.public_key = secret_key, public_key

    @classmethod
    def generate(cls, n=1, seed=None):
        """`seed` None: the operating system's generator like the reference's OsRng; an int: reproducible (tests)."""
        sk = _random_scalars(n, seed)
        xy, inf = engine().g2_generator_mul(sk)          # fixed-base table of the generator
        return cls(sk, G2Affine(xy, inf)._checked())

    def __len__(self):
        return self.secret_key.shape[0]


class _Expander:
    """Expander (hasher.rs:54-129), a tag and a security level bound to one of the library's expanders (SYLOW_HIP_EXPANDER_*)."""
    id = None

    def __init__(self, dst: bytes, k: int = 128):
        self.dst, self.k = bytes(dst), int(k)

    def expand_message(self, msgs, n: int) -> np.ndarray:          # expand_message(msg, len_in_bytes): uint8 [len(msgs), n]
        return engine().expand_message(list(msgs), n, self.id, self.dst, self.k)

    def hash_to_field(self, msgs) -> np.ndarray:                   # hash_to_field(msg, 2, 48) (hasher.rs:84-128): [len(msgs), 8] = (u0, u1)
        return engine().hash_to_field(list(msgs), self.dst, expander=self.id, k=self.k)


class XMDExpander(_Expander):
    """XMDExpander<D>::new(dst, k) (hasher.rs:137-173) with D = Keccak256 or Sha256."""

    def __init__(self, hash: str, dst: bytes, k: int = 128):
        if hash not in ("keccak256", "sha256"):
            raise ValueError("XMDExpander: hash is 'keccak256' or 'sha256'")
        super().__init__(dst, k)
        self.id = Engine.EXPANDERS["xmd_" + hash]


class XOFExpander(_Expander):
    """XOFExpander<Shake128>::new(dst, k) (hasher.rs:259-290)."""

    def __init__(self, hash: str, dst: bytes, k: int = 128):
        if hash != "shake128":
            raise ValueError("XOFExpander: hash is 'shake128'")
        super().__init__(dst, k)
        self.id = Engine.EXPANDERS["xof_shake128"]


def sign(k, msgs, expander=None) -> G1Affine:
    """sign(&Fp, &[u8]) (lib.rs:179-187): H(msg) * k; with an expander, sign_message(&expander, msg, k) (g1.rs:355)."""
    if expander is not None:
        xy, inf = engine().bls_sign(k, list(msgs), expander=expander.id, dst=expander.dst, k=expander.k)
    else:
        xy, inf = engine().bls_sign(k, list(msgs))
    return G1Affine(xy, inf)


def verify(pubkey: G2Affine, msgs, sig: G1Affine, expander=None) -> np.ndarray:
    """verify(&G2Projective, &[u8], &G1Projective) (lib.rs:223-236): elementwise bool; with an expander, H from that suite."""
    if expander is not None:
        return engine().bls_verify(pubkey.xy, list(msgs), sig.xy, pubkey.infinity, sig.infinity, expander=expander.id, dst=expander.dst,
                                   k=expander.k).astype(bool)
    return engine().bls_verify(pubkey.xy, list(msgs), sig.xy, pubkey.infinity, sig.infinity).astype(bool)


def verify_hashed(pubkey: G2Affine, h: G1Affine, sig: G1Affine) -> np.ndarray:
    """verify on points the caller hashed (any hash-to-curve; one hash against many signatures): e(sig, G2gen) == e(h, pubkey)."""
    return engine().bls_verify_hashed(pubkey.xy, h.xy, sig.xy, pubkey.infinity, h.infinity, sig.infinity).astype(bool)
