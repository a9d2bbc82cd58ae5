"""GPU: the Fr arithmetic core -- fr_reduce_plain, fr_add / fr_neg / fr_sub, fr_reduce_wide, fr_mulmod_inline, fr_inv (bn254_fr.hpp), mul_acc
(bn254_fr_acc.hpp) and the Euclid inversion behind fr_inv_lone (bn254_fr_euclid.hpp, bn254_fr_block.hpp) -- word for word against Python
integers, and against the C oracle's schoolbook product with bit-serial division where it offers the operation.  The inputs are the ones
random values do not reach: the full square of the edge words; products a b = s mod r whose Barrett remainder needs the final subtraction of
r (s next to 0) or does not (s next to r), canonical and lifted; sums of 16, 17 and 33 products with the same property through the unreduced
accumulator of k_fr_lincomb; structured values (1, 2, r - 1, 2^k, 2^k - 1, r - 2^k) as the product of a chunk, which is all the Euclid
inversion ever sees; and the two PLONK gate accumulators with every word at an extreme.  That the directed inputs have the classes they are
named for is asserted on the CPU, by tests/test_fr_core_model.py on the limb-exact model of tests/fr_core_model.py."""
import random

import numpy as np
import pytest

import fr_core_model as F
import kzg_evals_model as E
import kzg_multi_model as KM
import kzg_prove_model as KP
import plonk_open_model as O
import plonk_quotient_model as Q
from groth16_model import ints, limbs

pytestmark = pytest.mark.gpu
R, TOP = F.R, F.TOP
K = E.plan_constants()
L, CH = K["EVALS_LANE_ELEMS"], K["EVALS_CHUNK"]
TILE, FL = KM.plan_constants()["KZGM_LINCOMB_TILE"], KM.plan_constants()["KZGM_LINCOMB_FLUSH"]
BINOPS = {"add": lambda x, y: (x + y) % R, "sub": lambda x, y: (x - y) % R, "mul": lambda x, y: x * y % R}
UNOPS = {"sqr": lambda x: x * x % R, "neg": lambda x: -x % R, "inv": lambda x: pow(x % R, R - 2, R)}


def both_parities(vals, extra):
    """the list as it is and with one element appended: one length is even (the paired route of k_fp_binop / k_fp_unop), one odd (element-wise)"""
    out = [list(vals), list(vals) + [extra]]
    assert {len(v) % 2 for v in out} == {0, 1}
    return out


def check_binop(engine, coracle, op, pairs):
    a, b = limbs([x for x, _ in pairs]), limbs([y for _, y in pairs])
    got = getattr(engine, "fr_" + op)(a, b)
    want = limbs([BINOPS[op](x, y) for x, y in pairs])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"fr_{op}, n = {len(pairs)}: {len(bad)} differ, first {[hex(v) for v in pairs[bad[0]]]} -> {hex(ints(got[bad[:1]])[0])}"
    assert np.array_equal(got, coracle.fr_op(op, a, b)), op
    return got


def check_unop(engine, coracle, op, vals):
    a = limbs(vals)
    got = getattr(engine, "fr_" + op)(a)
    want = limbs([UNOPS[op](x) for x in vals])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"fr_{op}, n = {len(vals)}: {len(bad)} differ, first {hex(vals[bad[0]])} -> {hex(ints(got[bad[:1]])[0])}"
    assert np.array_equal(got, coracle.fr_op(op, a)), op
    return got


# ---- the edge square -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["add", "sub", "mul"])
def test_the_edge_square(engine, coracle, op):
    square = [(x, y) for x in F.EDGE for y in F.EDGE]
    assert len(square) == 39 * 39
    for pairs in both_parities(square, (R - 1, TOP)):
        got = check_binop(engine, coracle, op, pairs)
        assert all(v < R for v in ints(got))


@pytest.mark.parametrize("op", ["sqr", "neg", "inv"])
def test_the_edge_words_alone(engine, coracle, op):
    for vals in both_parities(F.EDGE, TOP):
        got = check_unop(engine, coracle, op, vals)
        assert all(v < R for v in ints(got))


# ---- the forced correction -----------------------------------------------------------------------------------------------------------------
def test_products_that_need_the_final_subtraction_and_products_that_do_not(engine, coracle):
    """a b = s mod r for s in {0, 1, 2} (the remainder before correction is r + s: class 1) and s in {r - 2, r - 1} (class 0), 64 canonical
    and 64 lifted pairs each; the classes are the model's, asserted in tests/test_fr_core_model.py"""
    pairs = F.forced_pairs()
    assert len(pairs) == 5 * 2 * F.FORCED_PER_S
    for run in both_parities(pairs, pairs[F.FORCED_PER_S]):
        got = check_binop(engine, coracle, "mul", run)
        assert ints(got[:len(pairs)]) == [s for s in F.FORCED_S for _ in range(2 * F.FORCED_PER_S)]
    for run in both_parities([(b, a) for a, b in pairs], pairs[0]):                      # the operands the other way round
        check_binop(engine, coracle, "mul", run)


def test_squares_of_every_word_of_1_and_of_r_minus_1(engine, coracle):
    words = F.forced_squares()
    assert {w % R for w in words} == {1, R - 1} and len(words) == 11
    for run in both_parities(words, F.lift(R - 1)):
        got = check_unop(engine, coracle, "sqr", run)
        assert ints(got) == [1] * len(run)
        check_binop(engine, coracle, "mul", [(w, w) for w in run])


# ---- the wide reduce with a forced correction ----------------------------------------------------------------------------------------------
def test_the_unreduced_accumulator_folds_to_s(engine):
    """groups of 16, 17 and 33 products (one fold, a fold and a residue, two folds and a residue) that sum to s in {0, 1, r - 1} in every
    column, TILE + 1 columns: the last fold of a group with s in {0, 1} needs the final subtraction in EVERY column, the one with s = r - 1
    in none (tests/test_fr_core_model.py)"""
    assert FL == F.FLUSH
    n = TILE + 1
    groups = F.wide_groups(n)
    a, w = [], []
    for terms, s, wj, cols in groups:
        a += [[cols[k][j] for k in range(n)] for j in range(terms)]
        w += wj
    gs = KM.offsets([terms for terms, _, _, _ in groups])
    assert gs[-1] == 3 * (16 + 17 + 33) == len(a)
    got = engine.fr_lincomb(KP.poly_words(a), limbs(w), gs)
    assert got.shape == (len(groups), n, 4)
    for g, (terms, s, _, _) in enumerate(groups):
        bad = np.flatnonzero((got[g] != limbs([s] * n)).any(axis=1))
        assert not len(bad), f"{terms} terms, s = {hex(s)}: {len(bad)} columns differ, column {bad[0]} is {hex(ints(got[g][bad[:1]])[0])}"
    for g, row in enumerate(KM.lincomb(a, w, gs)):
        assert np.array_equal(got[g], limbs(row))
    # the same residues from other words: the loads reduce, so the accumulator sees the same canonical factors
    rng = random.Random(0xF0C2)
    lifted = engine.fr_lincomb(KP.poly_words([[F.lift(v, rng) for v in row] for row in a]), limbs([F.lift(v) for v in w]), gs)
    assert lifted.tobytes() == got.tobytes()


# ---- the Euclid inversion ------------------------------------------------------------------------------------------------------------------
def ones(n):
    a = np.zeros((n, 4), dtype=np.uint64)
    a[:, 0] = 1
    return a


@pytest.fixture(scope="module")
def structured():
    """(the structured values, their words, their inverses by pow as words), made once"""
    return F.STRUCTURED, limbs(F.STRUCTURED), limbs([pow(x, R - 2, R) for x in F.STRUCTURED])


def test_structured_values_alone_and_as_a_lane_s_only_factor(engine, structured):
    """[x] (one lane, one element) and [x, 1, ..., 1] of L elements (one lane, every slot filled): the chunk's product is x"""
    xs, xw, want = structured
    assert len(xs) == 761 and np.array_equal(engine.fr_inv(xw), want), "fr_inv, the per-element power"
    lane = ones(L)
    for i in range(len(xs)):
        got = engine.fr_batch_inv(xw[i:i + 1])
        assert np.array_equal(got, want[i:i + 1]), f"[x], x = {hex(xs[i])}: {hex(ints(got)[0])}"
        lane[0] = xw[i]
        got = engine.fr_batch_inv(lane)
        assert np.array_equal(got[0], want[i]) and np.array_equal(got[1:], lane[1:]), f"[x, 1 x {L - 1}], x = {hex(xs[i])}: {[hex(v) for v in ints(got)]}"


def test_structured_values_as_the_product_of_whole_chunks(engine, structured):
    """[x, 1, ..., 1] of CH elements for every x, one chunk after another in ONE array, and one element more (a last chunk of [1]): every lane
    takes part in the scans and the top lane inverts x.  Against pow, and word for word against fr_inv."""
    xs, xw, want_x = structured
    n = len(xs) * CH + 1
    a, want = ones(n), ones(n)
    a[0:n - 1:CH], want[0:n - 1:CH] = xw, want_x
    got = engine.fr_batch_inv(a)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"{len(bad)} differ, first at {bad[0]} (chunk {bad[0] // CH}, x = {hex(xs[min(bad[0] // CH, len(xs) - 1)])})"
    assert np.array_equal(got, engine.fr_inv(a))
    # [x, 1, ..., 1] at CH + 1 as a call of its own, for the named values
    for i in range(7):
        short, want_short = ones(CH + 1), ones(CH + 1)
        short[0], want_short[0] = xw[i], want_x[i]
        assert np.array_equal(engine.fr_batch_inv(short), want_short), hex(xs[i])


def test_structured_values_as_the_product_of_two_factors(engine, structured):
    """[y, x / y, 1, ...] with a random y, the two factors in one lane (even chunks) or in two (odd chunks): the chunk's product is x, and both
    inverses come out of it -- y^-1 = x^-1 (x / y) and (x / y)^-1 = x^-1 y"""
    xs, _, _ = structured
    rng = random.Random(0xF0C3)
    ys = [rng.randrange(1, R) for _ in xs]
    zs = [x * pow(y, R - 2, R) % R for x, y in zip(xs, ys)]
    assert all(y * z % R == x for x, y, z in zip(xs, ys, zs))
    n = len(xs) * CH
    a, want = ones(n), ones(n)
    second = np.arange(len(xs)) * CH + np.where(np.arange(len(xs)) % 2 == 0, 1, L)
    a[0:n:CH], a[second] = limbs(ys), limbs(zs)
    want[0:n:CH], want[second] = limbs([pow(y, R - 2, R) for y in ys]), limbs([pow(z, R - 2, R) for z in zs])
    got = engine.fr_batch_inv(a)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), f"{len(bad)} differ, first at {bad[0]} (chunk {bad[0] // CH}, x = {hex(xs[bad[0] // CH])})"
    assert np.array_equal(got, engine.fr_inv(a))
    for i in (0, 1, 3, 4):                                       # [y, x / y] as a call of its own: 1, 2, r - 1, r - 2
        pair = limbs([ys[i], zs[i]])
        assert np.array_equal(engine.fr_batch_inv(pair), limbs([pow(ys[i], R - 2, R), pow(zs[i], R - 2, R)])), hex(xs[i])


# ---- the PLONK accumulators at the extremes ------------------------------------------------------------------------------------------------
POOL = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2]
FILLS = ["r - 1", "zero as r or 2r", "pool"]


def filler(kind, seed):
    """a source of input words: every word r - 1; every word a zero written as r or 2r by turns; every word drawn from POOL and lifted"""
    rng, turn = random.Random(seed), [0]

    def word():
        if kind == "r - 1":
            return R - 1
        if kind == "zero as r or 2r":
            turn[0] ^= 1
            return R if turn[0] else 2 * R
        return F.lift(rng.choice(POOL), rng if rng.random() < 0.5 else None)

    def tree(*shape):
        return [word() for _ in range(shape[0])] if len(shape) == 1 else [tree(*shape[1:]) for _ in range(shape[0])]
    return tree


def words(rows):
    """nested lists of ints [..][n] -> [.., n, 4] words"""
    a = np.asarray(rows, dtype=object)
    return limbs(list(a.reshape(-1))).reshape(a.shape + (4,))


@pytest.mark.parametrize("kind", FILLS)
@pytest.mark.parametrize("W", [3, 13, 17])
def test_the_fused_quotient_kernel_at_the_extremes(engine, W, kind):
    """gate_add of plonk_quotient.hip: W + 3 products a point (6, exactly the 16 of one flush, and 20: a fold in the middle), every factor an
    extreme, against the integer model"""
    log_n, log_e, m = 3, 2, 2
    big, tree = 1 << (log_n + log_e), filler(kind, 0xF100 + W)
    c = {"rows": tree(2 * W + 3, big), "zinv": tree(1 << log_e), "wires": tree(m, W, big), "z": tree(m, big), "pi": tree(m, big), "shifts": tree(W),
         "beta": tree(m), "gamma": tree(m), "alpha": tree(m)}
    want = [Q.quotient_evals(c["rows"], c["zinv"], c["wires"][s], c["z"][s], c["pi"][s], c["shifts"], c["beta"][s], c["gamma"][s], c["alpha"][s], log_n, log_e)
            for s in range(m)]
    table = engine.plonk_quotient_table_up(words(c["rows"]), limbs(c["zinv"]))
    got = engine.plonk_quotient_evals(table, words(c["wires"]), words(c["z"]), words(c["pi"]), limbs(c["shifts"]), limbs(c["beta"]), limbs(c["gamma"]),
                                      limbs(c["alpha"]), log_n, log_e)
    assert got.shape == (m, big, 4) and np.array_equal(got, words(want)), (W, kind)


@pytest.mark.parametrize("kind", FILLS)
@pytest.mark.parametrize("W,log_e", [(3, 2), (4, 3), (17, 5)])
def test_r_and_f_at_the_extremes(engine, W, log_e, kind):
    """gate_add of plonk_open.hip: (W, E) = (3, 4) has exactly 16 products a column with F, (4, 8) exactly 16 for r, (17, 32) several
    flushes; every factor an extreme, against the integer model"""
    log_n, m = 3, 2
    n, E_ = 1 << log_n, 1 << log_e
    assert (W + 4 + E_, 3 * W + 3 + E_) in ((11, 16), (16, 23), (53, 86))
    tree = filler(kind, 0xF200 + W)
    c = {"ct": tree(2 * W + 2, n), "wires": tree(m, W, n + 2), "z": tree(m, n + 3), "t": tree(m, n << log_e), "evals": tree(m, 2 * W + 1), "shifts": tree(W)}
    for k in ("beta", "gamma", "alpha", "zeta", "v"):
        c[k] = tree(m)
    want = [O.linearise(c["ct"], c["wires"][s], c["z"][s], c["t"][s], c["evals"][s], c["shifts"], c["beta"][s], c["gamma"][s], c["alpha"][s], c["zeta"][s],
                        c["v"][s], log_n, log_e) for s in range(m)]
    r, f, status = engine.plonk_open_linearise(engine.plonk_open_ctable_up(words(c["ct"])), words(c["wires"]), words(c["z"]), words(c["t"]), words(c["evals"]),
                                               limbs(c["shifts"]), limbs(c["beta"]), limbs(c["gamma"]), limbs(c["alpha"]), limbs(c["zeta"]), limbs(c["v"]), log_e)
    assert r.shape == (m, n + 3, 4) and f.shape == (m, n + 3, 4)
    assert np.array_equal(r, words([x[0] for x in want])), (W, kind, "r")
    assert np.array_equal(f, words([x[1] for x in want])), (W, kind, "F")
    assert list(status) == [x[2] for x in want], (W, kind)
