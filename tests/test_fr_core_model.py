"""CPU: the limb-exact model of the Fr core (tests/fr_core_model.py) against Python's % and pow, and the CONDITION that keeps
tests/test_gpu_fr_core.py honest: the directed inputs it hands the device do take the branches they are named for.  The class of an input of
the Barrett reduction is the number of times r fits into the remainder before correction; class 1 is the final conditional subtraction of r,
which about 3 in 10^4 products of canonical operands take (57 of 200,000 here) and about 1 % of products of full-range words (2126 of
200,000).  Last, the model with each fault switched on: it differs exactly where the directed inputs say it must."""
import os
import random
import re

import fr_core_model as F
import kzg_multi_model as KM

R, TOP = F.R, F.TOP
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sylow_amd", "csrc")
TILE = KM.plan_constants()["KZGM_LINCOMB_TILE"]


def hex_words(text):
    return sum(int(w, 16) << (32 * i) for i, w in enumerate(re.findall(r"0x([0-9a-fA-F]{8})u", text)))


def test_the_model_s_constants_are_the_headers():
    fr = open(os.path.join(CSRC, "bn254_fr.hpp")).read()
    assert hex_words(re.search(r"#define BN_FR_R (.*)", fr).group(1)) == R
    assert hex_words(re.search(r"#define BN_FR_2R (.*)", fr).group(1)) == 2 * R
    assert hex_words(re.search(r"#define BN_FR_MU (.*)", fr).group(1)) == F.MU == (1 << 512) // R and F.MU < 1 << 288
    eu = open(os.path.join(CSRC, "bn254_fr_euclid.hpp")).read()
    assert hex_words(re.search(r"constexpr uint32_t R\[8\] = \{(.*)\};", eu).group(1)) == R
    assert int(re.search(r"constexpr int MAX_STEPS = (\d+);", eu).group(1)) == F.MAX_STEPS
    assert KM.plan_constants()["KZGM_LINCOMB_FLUSH"] == F.FLUSH
    assert int(re.search(r"constexpr int32_t SPMV_FLUSH = (\d+);", open(os.path.join(CSRC, "groth16_prove_plan.hpp")).read()).group(1)) == F.FLUSH


def test_the_edge_and_structured_lists():
    e, s = F.EDGE, F.STRUCTURED
    assert len(e) == len(set(e)) == 39 and len(s) == len(set(s)) == 761
    for w in (0, 1, R - 1, R, R + 1, 4 * R + 1, 5 * R - 1, 5 * R, 5 * R + 1, (1 << 224) - 1, 1 << 224, TOP, F.P, 0xFFFFFFFF << 224, 0xFFFFFFFF << 96):
        assert w in e, hex(w)
    assert 6 * R - 1 > TOP and max(e) == TOP
    for x in (1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 253, (1 << 253) - 1, R - (1 << 252)):
        assert x in s, hex(x)
    assert all(0 < x < R for x in s)
    for x in (0, 1, R - 1, R - 2):
        words = F.lifts(x)
        assert len(words) == (TOP - x) // R and len(words) in (4, 5) and all(w % R == x and R <= w <= TOP for w in words) and F.lift(x) == words[-1] and words[-1] + R > TOP


def barrett_inputs():
    rng = random.Random(0xBA44E77)
    out = [rng.randrange(1 << 512) for _ in range(10 ** 4)]
    out += [x * y for x in F.EDGE for y in F.EDGE]
    out.append((1 << 512) - 1)
    q_top = ((1 << 512) - 1) // R
    for q in range(q_top, q_top - 1000, -1):
        out += [T for T in (q * R + f for f in (0, 1, R - 1)) if T < 1 << 512]
    assert len(out) == 10 ** 4 + 39 * 39 + 1 + 3000 - 1         # q_top r + r - 1 is the one past 2^512
    return out


def test_barrett_result_and_class():
    """barrett(T) is T mod r, and cls <= 1 on every input: the remainder before correction is BELOW 2r, not merely below the 4r the header's
    comment grants.  Why: MU = floor(2^512 / r) is short of 2^512 / r by its fractional part 0.0432, so q1 MU / 2^288 is short of T / r by at
    most 0.0432 T / 2^512 + 2^-29 (the 224 low bits of T that q1 drops), and the dropped columns 0 .. 6 of q1 x MU by at most
    8 (2^32)^2 2^(32 * 6) / 2^288 = 2^-29 more: the estimate is the true quotient or one less, never two.  (The model also asserts, inside
    barrett, that T - q3 r equals the 256-bit difference the device forms: nothing wraps.)  So the conditional subtraction of 2r in
    fr_reduce_wide never fires; the one of r is the only live correction."""
    seen = [0, 0]
    for T in barrett_inputs():
        got, cls = F.barrett(T)
        assert got == T % R, hex(T)
        assert cls in (0, 1), (hex(T), cls)
        seen[cls] += 1
    assert min(seen) > 0
    assert F.barrett((1 << 512) - 1)[1] == 1 and F.barrett(TOP * TOP)[1] == 0


def test_every_directed_product_has_the_class_it_is_named_for():
    """a b = s mod r: T = q r + s.  The estimate falls short of T / r by a positive error far above 2^-250, so for s next to 0 it lands
    on q - 1 (class 1) and for s next to r on q (class 0), whatever the operands.  The lone exception is T = 0 (canonical b = 0)."""
    rng = random.Random(0xD1EC7)
    for mode in ("top", "random", None):
        for s in F.FORCED_S:
            want = 1 if s <= 2 else 0
            if mode is None and s == 0:
                want = 0                                         # a x 0: T = 0
            pairs = F.product_pairs(rng, s, 400, mode)
            assert all((a >= R and b >= R) if mode else (a < R and b < R) for a, b in pairs)
            for a, b in pairs:
                got, cls = F.barrett(a * b)
                assert got == s and cls == want, (mode, s, hex(a), hex(b))


def test_every_directed_group_has_the_class_it_is_named_for():
    """16 canonical products that sum to s: class 1 for s in {0, 1}, class 0 for s = r - 1; and the LAST fold of a longer group likewise,
    since the accumulator it reduces is = s as well"""
    rng = random.Random(0xD1EC8)
    for s in (0, 1, R - 1):
        for _ in range(200):
            (T,) = F.folds(F.wide_terms(rng, s, F.FLUSH))
            assert T < R + F.FLUSH * R * R < 1 << 512
            assert F.barrett(T) == (s, 0 if s == R - 1 else 1)
    groups = F.wide_groups(TILE + 1)
    assert [(t, s) for t, s, _, _ in groups] == [(t, s) for t in (16, 17, 33) for s in (0, 1, R - 1)] and groups[0][2] == F.wide_groups(2)[0][2]
    for terms, s, w, cols in groups:
        assert len(cols) == TILE + 1 and len(w) == terms
        for a in cols:
            Ts = F.folds(list(zip(w, a)))
            assert len(Ts) == (terms + F.FLUSH - 1) // F.FLUSH
            classes = [F.barrett(T)[1] for T in Ts]
            assert F.barrett(Ts[-1])[0] == s and classes[-1] == (0 if s == R - 1 else 1), (terms, s)


def test_the_pairs_of_the_device_test_are_split_between_the_classes():
    pairs = F.forced_pairs()
    assert pairs == F.forced_pairs() and len(pairs) == 5 * 2 * F.FORCED_PER_S
    classes = [F.barrett(a * b)[1] for a, b in pairs]
    assert 3 * classes.count(1) >= len(pairs) and 3 * classes.count(0) >= len(pairs)
    assert sum(a >= R for a, _ in pairs) == len(pairs) // 2
    sq = [F.barrett(x * x) for x in F.forced_squares()]
    assert len(sq) == 11 and all(v == 1 for v, _ in sq) and {c for _, c in sq} == {0, 1}


def test_without_the_final_subtraction_every_class_1_input_comes_out_wrong():
    """the fault the directed inputs are for: fr_reduce_wide without its last conditional subtraction.  EVERY class 1 input of the device
    test's lists -- pairs, squares, and the last fold of each group -- then differs from T mod r, and no class 0 input does."""
    inputs = [a * b for a, b in F.forced_pairs()] + [x * x for x in F.forced_squares()]
    for terms, s, w, cols in F.wide_groups(3):
        inputs += [T for a in cols for T in F.folds(list(zip(w, a)))]
    hit = 0
    for T in inputs:
        good, cls = F.barrett(T)
        bad, _ = F.barrett(T, final_sub=False)
        assert good == T % R and (bad != good) == (cls == 1) and (cls == 0 or bad == good + R)
        hit += cls
    assert hit >= len(inputs) // 3


def test_euclid_is_pow_within_the_step_bound():
    """euclid(a) = a^(r-2) on the 761 structured values and 2000 random ones, in fewer than 1016 steps.  The largest counts seen: 552 on the
    structured values (asserted: the list is fixed), 568 on 20,000 random values and 560 on the 2000 drawn here."""
    rng = random.Random(0xE0C1)
    worst = 0
    for a in F.STRUCTURED:
        got, steps = F.euclid(a)
        assert got == pow(a, R - 2, R) and got * a % R == 1 and steps < F.MAX_STEPS, hex(a)
        worst = max(worst, steps)
    assert worst == 552
    for _ in range(2000):
        a = rng.randrange(1, R)
        got, steps = F.euclid(a)
        assert got == pow(a, R - 2, R) and steps < F.MAX_STEPS, hex(a)
    assert F.euclid(1) == (1, 0) and F.euclid(0) == (0, F.MAX_STEPS)


def test_a_step_bound_100_short_of_the_structured_need_is_caught():
    """the fault the structured values are for: a loop that ends too early.  With 452 steps, 100 short of what they need at most, at least
    one structured value comes out wrong (as 0), and every value that needs no more than 452 steps is still right."""
    wrong = 0
    for a in F.STRUCTURED:
        full, steps = F.euclid(a)
        cut, _ = F.euclid(a, max_steps=552 - 100)
        assert (cut == full) == (steps <= 452) and cut in (full, 0)
        wrong += cut != full
    assert wrong >= 1
