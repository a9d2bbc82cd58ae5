"""CPU: the integer model of PLONK's closing rounds (tests/plonk_open_model.py) against the protocol's own identities, on satisfied witnesses
at log_n = 0, 1, 3 and W = 2, 3, 4 (E = 4, and E = 8 for W = 4, whose blinded quotient needs it), blinded and not, with and without public
inputs: r(zeta) = 0 and status 0; F(zeta) is the fold of the evaluations under v; X - zeta divides F - F(zeta); and r agrees at three other
points with the identity's numerator minus ZH t evaluated value by value, an independent route.  Then the statuses: bit 0 after one changed
wire coefficient, one changed coefficient of t and one changed evaluation; bit 1 for zeta = 1 and zeta = w_n."""
import random

import pytest

import ntt_model as T
import plonk_open_model as O
import plonk_quotient_model as Q

R = O.R
SHAPES = [(log_n, W, 3 if W == 4 else 2) for log_n in (0, 1, 3) for W in (2, 3, 4)]


def log_e_that_holds_t(log_n, W, log_e, blinded):
    """E = 4 (8 for W = 4) holds the quotient of a blinded witness only from n = 8 on: at n = 1 and 2 the blinders dominate the degree
    (len_w = n + 2, len_z = n + 3), and t, which must be the TRUE quotient here, needs the next E that holds its D - n + 1 coefficients"""
    n, extra = 1 << log_n, (2, 3) if blinded else (0, 0)
    need = Q.degree_bound(log_n, W, n + extra[0], n + extra[1]) - n + 1
    while (n << log_e) < need:
        log_e += 1
    return log_e


def instance(log_n, W, log_e, blinded, with_pi):
    log_e = log_e_that_holds_t(log_n, W, log_e, blinded)
    rng = random.Random(0xB100 + 64 * log_n + 8 * W + 2 * blinded + with_pi)
    s = O.satisfied(rng, log_n, W, log_e, blinded, with_pi)
    s["zeta"], s["v"] = rng.randrange(2, R), rng.randrange(R)
    return s, rng


def run(s, zeta=None, wires=None, t=None, bump=None):
    zeta = s["zeta"] if zeta is None else zeta
    wires, t = s["wires"] if wires is None else wires, s["t"] if t is None else t
    ev = O.evaluate(s["ct"], wires, s["z"], s["pi"], zeta, s["log_n"])
    if bump is not None:
        ev[bump] = (ev[bump] + 1) % R
    return ev, O.linearise(s["ct"], wires, s["z"], t, ev, s["c"]["shifts"], s["beta"], s["gamma"], s["alpha"], zeta, s["v"], s["log_n"], s["log_e"])


@pytest.mark.parametrize("with_pi", [False, True])
@pytest.mark.parametrize("blinded", [False, True])
@pytest.mark.parametrize("log_n,W,log_e", SHAPES)
def test_satisfied_witnesses_linearise_to_zero_and_fold_to_the_evaluations(log_n, W, log_e, blinded, with_pi):
    s, rng = instance(log_n, W, log_e, blinded, with_pi)
    log_e = s["log_e"]
    assert log_e == (3 if W == 4 else 2) or (blinded and log_n < 3)
    n, zeta, v, sh = 1 << log_n, s["zeta"], s["v"], s["c"]["shifts"]
    ev, (r, f, status) = run(s)
    assert len(ev) == 2 * W + 1 and (ev[2 * W] != 0) == (with_pi and any(s["pi"]))
    assert len(r) == max(n, len(s["z"])) and len(f) == max(n, len(s["z"]), len(s["wires"][0]))
    assert Q.p_eval(r, zeta) == 0 and status == 0
    y = Q.p_eval(f, zeta)
    assert y == O.folded_value(ev, v, W)
    quo, rem = O.divide_by_linear(Q.p_add(f, [R - y]), zeta)
    assert rem == 0 and Q.p_add(Q.p_mul(quo, [R - zeta, 1]) if quo else [0], [y]) == f
    # without v: the same r and status, no F
    r2, f2, status2 = O.linearise(s["ct"], None, s["z"], s["t"], ev, sh, s["beta"], s["gamma"], s["alpha"], zeta, None, log_n, log_e)
    assert (r2, f2, status2) == (r, None, 0)
    # the independent route: value by value at three other points
    zh, l1, A, B = O.scalars(ev, sh, s["beta"], s["gamma"], zeta, log_n)
    a, zw, p = ev[:W], ev[2 * W - 1], ev[2 * W]
    for _ in range(3):
        x = rng.randrange(R)
        assert x != zeta
        q_at, sg_last, z_at = [Q.p_eval(row, x) for row in s["ct"][:W + 2]], Q.p_eval(s["ct"][2 * W + 1], x), Q.p_eval(s["z"], x)
        t_at = sum(pow(zeta, e * n, R) * Q.p_eval(s["t"][e * n:(e + 1) * n], x) for e in range(1 << log_e)) % R
        want = (q_at[W] * a[0] * a[1] + sum(q_at[j] * a[j] for j in range(W)) + q_at[W + 1] + p +
                s["alpha"] * (A * z_at - B * zw * (a[W - 1] + s["beta"] * sg_last + s["gamma"])) + s["alpha"] ** 2 * l1 * (z_at - 1) - zh * t_at) % R
        assert Q.p_eval(r, x) == want
    # and r(zeta) = 0 says what it should: the numerator at zeta from the values there equals t(zeta) ZH
    q_z, sg_z = [Q.p_eval(row, zeta) for row in s["ct"][:W + 2]], [Q.p_eval(row, zeta) for row in s["ct"][W + 2:]]
    assert sg_z[:W - 1] == ev[W:2 * W - 1]
    num = O.numerator_at(q_z, sg_z, a, Q.p_eval(s["z"], zeta), zw, p, sh, s["beta"], s["gamma"], s["alpha"], zeta, log_n)
    assert num == Q.p_eval(s["t"], zeta) * zh % R


@pytest.mark.parametrize("log_n,W,log_e", [(1, 2, 2), (3, 3, 2), (3, 4, 3)])
def test_statuses(log_n, W, log_e):
    s, rng = instance(log_n, W, log_e, True, True)
    wires = [list(w) for w in s["wires"]]
    wires[W - 1][1] = (wires[W - 1][1] + 1) % R
    assert run(s, wires=wires)[1][2] == O.STATUS_R_NOT_ZERO, "one changed wire coefficient"
    t = list(s["t"])
    t[(1 << log_n) + 1] = (t[(1 << log_n) + 1] + 1) % R
    assert run(s, t=t)[1][2] == O.STATUS_R_NOT_ZERO, "one changed coefficient of t"
    for slot in (0, W, 2 * W - 1, 2 * W):
        assert run(s, bump=slot)[1][2] == O.STATUS_R_NOT_ZERO, f"evaluation {slot} changed"
    for zeta in (1, T.omega(log_n), 1 + R):
        ev, (r, f, status) = run(s, zeta=zeta)
        assert status & O.STATUS_ZETA_IN_DOMAIN, zeta
    assert O.scalars(run(s, zeta=1)[0], s["c"]["shifts"], s["beta"], s["gamma"], 1, log_n)[:2] == (0, 0), "inv(0) = 0: L1 = 0 at zeta = 1"
    assert run(s)[1][2] == 0
