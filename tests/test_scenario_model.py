"""CPU: the two host statements of the scenario stage -- tests/scenario_model.py (scalar,
independent) and mpcq/scenario.py (numpy, shipped) -- against known answers, hand-computed
cases, each other, and the reference's joystick; and the coverage the GPU tests lean on."""
import functools
import os

import numpy as np
import pytest

import scenario_cases as SC
import scenario_model as SM
from conftest import GOLDEN
from monitor_model import same

KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        "d16cfe09 94fdcceb 5001e420 24126ea1"))


@pytest.fixture(scope="module")
def S():
    from mpcq import scenario
    return scenario


@functools.lru_cache(maxsize=None)
def _model(B):
    p = SM.params(**SC.SMALL)
    return p, SC.model_calls(p, B, 500 + B)


def test_philox_known_answers(S):
    for ctr, key, want in KAT:
        assert " ".join(f"{w:08x}" for w in SM.philox(ctr, key)) == want
        assert " ".join(f"{int(w):08x}" for w in S.philox(*ctr, *key)) == want
    # vectorised: the three at once
    c = np.array([k[0] for k in KAT], np.uint64).T
    k = np.array([k[1] for k in KAT], np.uint64).T
    w = np.stack(S.philox(*c, *k), axis=-1)
    assert [" ".join(f"{int(x):08x}" for x in row) for row in w] == [k[2] for k in KAT]


def test_derived_values():
    assert SM.u(0, 0) == 0.0 and SM.u(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert SM.u(1 << 31, 0) == 0.5 and SM.u(0, 1 << 6) == 2.0 ** -53
    assert SM.rng(-2.0, 6.0, 0.25) == 0.0 and SM.rng(3.0, 3.0, 0.7) == 3.0
    got = {SM.draw_int(4, 3, w) for w in (0, 1, 0x55555555, 0x55555556, 0xAAAAAAAA, 0xAAAAAAAB, 0xFFFFFFFF)}
    assert got == {4, 5, 6}
    assert SM.draw_int(4, 3, 0) == 4 and SM.draw_int(4, 3, 0xFFFFFFFF) == 6 and SM.draw_int(7, 1, 0xFFFFFFFF) == 7
    assert SM.draw_int(4, 3, 0x55555555) == 4 and SM.draw_int(4, 3, 0x55555556) == 5
    assert not SM.prob(0, 0.0) and SM.prob(0xFFFFFFFF, 1.0) and SM.prob(0x7FFFFFFF, 0.5) and not SM.prob(1 << 31, 0.5)


def test_alpha_and_exact_ends():
    p = SM.params(cmd_start=4, cmd_ramp=8, cmd_period=20, v_lo=[-1.0, -1.0, -1.0], v_hi=[1.0, 1.0, 1.0], seed=5)
    assert SM.alpha(p, 0) == (0, -4, 0.0) and SM.alpha(p, 3) == (0, -1, 0.0)
    assert SM.alpha(p, 4) == (0, 0, 0.0) and SM.alpha(p, 6) == (0, 2, 0.25)
    assert SM.alpha(p, 12) == (0, 8, 1.0) and SM.alpha(p, 19) == (0, 15, 1.0)
    # the boundary: tau = cmd_period is segment 1's tick 0 (no cmd_start there), back at alpha 0
    assert SM.alpha(p, 20) == (1, 0, 0.0) and SM.alpha(p, 21) == (1, 1, 0.125) and SM.alpha(p, 28) == (1, 8, 1.0)
    q = SM.params(cmd_start=2, cmd_ramp=0, cmd_period=0)
    assert SM.alpha(q, 1) == (0, -1, 0.0) and SM.alpha(q, 2) == (0, 0, 1.0) and SM.alpha(q, 10 ** 6) == (0, 10 ** 6 - 2, 1.0)
    t0, t1 = SM.target(p, 3, 2, 0), SM.target(p, 3, 2, 1)
    pick = lambda v: [v[0], v[1], v[5]]  # noqa: E731
    assert pick(SM.command(p, 3, 2, 0)) == [0.0, 0.0, 0.0] and pick(SM.command(p, 3, 2, 4)) == [0.0, 0.0, 0.0]
    assert pick(SM.command(p, 3, 2, 12)) == t0 and pick(SM.command(p, 3, 2, 19)) == t0
    assert pick(SM.command(p, 3, 2, 20)) == t0  # alpha 0 of segment 1: prev exactly
    assert pick(SM.command(p, 3, 2, 28)) == t1 and pick(SM.command(p, 3, 2, 39)) == t1
    mid = SM.command(p, 3, 2, 22)
    assert pick(mid) == [t0[e] + (t1[e] - t0[e]) * 0.25 for e in range(3)] and mid[2:5] == [0.0, 0.0, 0.0]
    assert all(-1.0 <= x <= 1.0 for x in t0 + t1) and t0 != t1
    assert SM.command(SM.params(commands=0), 0, 1, 100) == [0.0] * 6


def _find(pred, what):
    for b in range(4000):
        if pred(b):
            return b
    raise AssertionError(f"no robot with {what}")


def test_push_windows_jitter_prob_and_flips():
    kw = dict(pushes=1, push_first=3, push_period=10, push_jitter=4, push_ticks=2, push_flip=0b000101, seed=11,
              wrench_lo=[30.0, 1.0, 2.0, 3.0, 4.0, 5.0], wrench_hi=[60.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    p = SM.params(**kw)
    assert SM.window(p, 0, 1, 2) is None and SM.push(p, 0, 1, 2) == ([0.0] * 6, False)
    seen_jitter = {SM.window(p, b, 1, 3)["jitter"] for b in range(200)}
    assert seen_jitter == {0, 1, 2, 3, 4}
    for jit in (0, 4):  # the window's first and last active tick, at both ends of the jitter
        b = _find(lambda b: SM.window(p, b, 1, 3)["jitter"] == jit, f"jitter {jit}")
        s = 3 + jit
        assert [SM.push(p, b, 1, t)[1] for t in range(s - 1, s + 3)] == [False, True, True, False], (jit, b)
        assert SM.window(p, b, 1, s)["s"] == s and SM.window(p, b, 1, 12)["j"] == 0 and SM.window(p, b, 1, 13)["j"] == 1
        w = SM.push(p, b, 1, s)[0]
        assert w == SM.push(p, b, 1, s + 1)[0] and 30.0 <= abs(w[0]) <= 60.0 and w[1] == 1.0 and w[3:] == [3.0, 4.0, 5.0]
        bits = SM.window(p, b, 1, s)["bits"]
        assert (w[0] < 0) == bool(bits & 1) and (w[2] == -2.0) == bool(bits & 4) and abs(w[2]) == 2.0
    # all four flip combinations of the two enabled components occur, and no other component flips
    combos = set()
    for b in range(64):
        w = SM.window(p, b, 1, 3)
        x = SM.push(p, b, 1, w["s"])[0]
        combos.add((x[0] < 0, x[2] < 0))
        assert x[1] > 0 and x[3] > 0 and x[4] > 0 and x[5] > 0
    assert combos == {(False, False), (False, True), (True, False), (True, True)}
    never, always = SM.params(**dict(kw, push_prob=0.0)), SM.params(**dict(kw, push_prob=1.0))
    for b in range(20):
        assert not any(SM.push(never, b, 1, t)[1] for t in range(40))
        assert sum(SM.push(always, b, 1, t)[1] for t in range(3, 43)) == 8  # 4 windows of 2 ticks
    half = SM.params(**dict(kw, push_prob=0.5))
    n = sum(SM.window(half, b, 1, 3)["occurs"] for b in range(400))
    assert 150 < n < 250
    # a single window (push_period 0)
    one = SM.params(**dict(kw, push_period=0, push_jitter=0))
    assert [SM.push(one, 0, 1, t)[1] for t in range(2, 7)] == [False, True, True, False, False]
    assert not SM.push(one, 0, 1, 10 ** 6)[1]


def test_epoch_and_tau_on_first_ticks():
    p = SM.params(**SC.SMALL)
    base = SC.base_table(3, 0)
    st = SM.new_state(3)
    SM.step(p, st, None, False, base, init=True)  # enable: epoch 0's draw, nothing advanced
    assert st["epoch"].tolist() == [0, 0, 0] and st["tick"].tolist() == [0, 0, 0] and st["draw"][:, 2].tolist() == [0.0] * 3
    _, _, _, seen = SM.step(p, st, None, True, base)
    assert seen == [(1, 0, True)] * 3 and st["tick"].tolist() == [1, 1, 1]
    SM.step(p, st, np.zeros(3, np.int32), False, base)
    keep = st["robots"].copy()
    _, _, _, seen = SM.step(p, st, np.array([0, 1, 0], np.int32), False, base)
    assert seen == [(1, 2, False), (2, 0, True), (1, 2, False)]
    assert st["epoch"].tolist() == [1, 2, 1] and st["tick"].tolist() == [3, 1, 3]
    assert st["draw"][:, 2].tolist() == [1.0, 2.0, 1.0]
    assert same(st["robots"][[0, 2]], keep[[0, 2]]) and st["robots"][1] != keep[1]
    ms, mu = SM.constants(p, 1, 2)
    assert 0.8 <= ms <= 1.3 and 0.5 <= mu <= 1.0 and st["draw"][1, :2].tolist() == [ms, mu]
    r = st["robots"][1]
    assert r["mass"] == base["mass"][1] * ms and r["mu"] == mu and r["fz_max"] == base["fz_max"][1]
    assert same(r["gI"], (base["gI"][1].reshape(9) * ms).reshape(3, 3))
    # the bits of `robots`
    for bits in (0, 1, 2):
        q = SM.params(**dict(SC.SMALL, robots=bits))
        row = SM.robot_row(q, base[1], ms, mu)
        assert (row["mass"] == base["mass"][1]) == (not bits & 1) and (row["mu"] == base["mu"][1]) == (not bits & 2)


@pytest.mark.parametrize("B", SC.BATCHES)
def test_numpy_statement_equals_the_model(S, B):
    p, res = _model(B)
    base = SC.base_table(B, 500 + B)
    robots = np.arange(B)
    for c, r in enumerate(res):
        epochs = np.array([e for e, _, _ in r["seen"]])
        taus = np.array([t for _, t, _ in r["seen"]])
        firsts = np.array([f for _, _, f in r["seen"]])
        assert same(S.command(p, robots, epochs, taus), r["v_ref"]), (B, c)
        pu, active = S.push(p, robots, epochs, taus)
        assert same(pu, r["push"]), (B, c)
        win = SC.wrench(B, 500 + B)
        assert same(np.where(active[:, None], win + pu, win), r["wrench_out"]), (B, c)
        ms, mu = S.constants(p, robots, epochs)
        assert same(ms[firsts], r["draw"][firsts, 0]) and same(mu[firsts], r["draw"][firsts, 1]), (B, c)
        rows = S.apply_constants(p, base, ms, mu)
        for f in ("mass", "gI", "mu", "fz_max", "reserved"):
            assert same(rows[f][firsts], r["robots"][f][firsts]), (B, c, f)
    # broadcasting: a (ticks, robots) grid in one call
    grid = S.command(p, robots[None, :], 1, np.arange(13)[:, None])
    assert grid.shape == (13, B, 6) and grid[7, B - 1].tolist() == SM.command(p, B - 1, 1, 7)


@pytest.mark.parametrize("B", [b for b in SC.BATCHES if b >= 63])
def test_the_generator_covers_every_kind(B):
    p, res = _model(B)
    kinds = SC.coverage(p, res)
    assert kinds == set(SC.KINDS), sorted(set(SC.KINDS) - kinds)
    # first masks on some robots at some calls, none at others; epochs advance for those only
    masks = SC.first_masks(B, 500 + B)
    assert masks[1:].any() and not masks[1].any() and (masks.sum(axis=0) > 0).sum() > B // 2
    assert np.array_equal(res[-1]["epoch"], 1 + masks[1:].sum(axis=0))


def test_default_scenario_is_the_reference_joystick(S):
    d = np.load(os.path.join(GOLDEN, "joystick_golden.npz"))
    tau, want = d["tau"], d["v_ref"]
    assert tau.tolist() == list(range(261)) and want.shape == (261, 6)
    assert want[48, 0] == 0.0 and 0.0 < want[49, 0] < want[222, 0] < 1.0 and want[223, 0] == 1.0
    p = SM.params()
    for b, epoch in ((0, 0), (7, 1), (129, 3), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert same(S.command(p, b, epoch, tau), want), (b, epoch)
    assert same(np.array([SM.command(p, 5, 2, int(t)) for t in tau]), want)
