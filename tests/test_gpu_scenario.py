"""GPU: the scenario stage (mpcq_scenario_step_batch, mpcq_session_enable_scenario) against its
host model (tests/scenario_model.py), and what a session promises around it.

Every comparison here is bit equality (monitor_model.same: NaN equals NaN, -0.0 differs from
0.0): the generator is integer arithmetic, and kernel and model derive every double by the same
float64 operations without contraction.  The one exception is MPCQ_SV_ORDER, whose order inside
a bucket of 16 iterations is left to LDS atomics by design (tests/test_gpu_monitor.py).

The cases of the kernel tests are tests/scenario_cases.py's; tests/test_scenario_model.py
asserts on the CPU that they contain every kind of robot-tick (ramps, holds, three segments,
active / inactive / skipped windows, every jitter, flips, restarts in mid-sequence)."""
import ctypes as C

import numpy as np
import pytest

import scenario_cases as SC
import scenario_model as SM
from monitor_model import same

pytestmark = pytest.mark.gpu

N, SB, TICKS = 16, 65, 12  # the sessions: horizon, batch (two blocks, the second with one robot), ticks
SV = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_L_FEET", "SV_Q_W", "SV_COST",
      "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_ROT_FLAG", "SV_H_ROT", "SV_X_ROBOT", "SV_ORDER", "SV_FIRST")
SWING = ("SV_SWING_REF", "SV_SWING_STATE", "SV_FRAME")
PV = ("PV_STATE_END", "PV_F_EFF", "PV_WRENCH")
MV = ("MV_DONE", "MV_EP", "MV_EP_TICKS", "MV_EPISODES", "MV_LAST", "MV_TOTALS")
CV = ("CV_EPOCH", "CV_TICK", "CV_V_REF", "CV_PUSH", "CV_WRENCH", "CV_ROBOTS", "CV_DRAW")
ROBOT_FIELDS = ("mass", "gI", "mu", "fz_max", "reserved")
MON = dict(max_ticks=5, auto_reset=1)  # every robot restarts after ticks 4 and 9
PUSHED = (3, 40)  # the robots with a wrench of the user's


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.fixture(scope="module")
def eng(mpcq):
    with mpcq.Engine(N) as e:
        yield e


def _same_robots(a, b):
    return all(same(np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])) for f in ROBOT_FIELDS)


# ------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("bare", [False, True], ids=["base+wrench", "bare"])
@pytest.mark.parametrize("B", SC.BATCHES)
def test_step_batch_vs_model(mpcq, eng, B, bare):
    p = SM.params(**SC.SMALL)
    seed = 500 + B
    want = SC.model_calls(p, B, seed, with_base=not bare, with_wrench=not bare, default_row=mpcq.robots(1)[0])
    masks = SC.first_masks(B, seed)
    base = None if bare else SC.base_table(B, seed)
    win = None if bare else SC.wrench(B, seed)
    scn = mpcq.Scenario(eng, mpcq.default_scenario_params(**SC.SMALL))
    st = None
    for c, w in enumerate(want):
        v_ref, pu, wo, st = scn.step(st, first=masks[c], all_first=c == 0, base=base, wrench_in=win, batch=B)
        ctx = (B, bare, c)
        assert same(v_ref, w["v_ref"]) and same(pu, w["push"]) and same(wo, w["wrench_out"]), ctx
        assert same(st["epoch"], w["epoch"]) and same(st["tick"], w["tick"]) and same(st["draw"], w["draw"]), ctx
        assert _same_robots(st["robots"], w["robots"]), ctx
    assert st["epoch"].max() > 1 or B == 1


def test_step_batch_optional_outputs_and_device_pointers(mpcq, eng):
    import torch
    B, seed = 65, 9
    p = SM.params(**SC.SMALL)
    masks = SC.first_masks(B, seed, 4)
    masks[2, [0, 64]] = 1
    want = []
    stm = SM.new_state(B)
    base, win = SC.base_table(B, seed), SC.wrench(B, seed)
    for c in range(4):
        want.append(SM.step(p, stm, masks[c], c == 0, base, win)[:3] + (stm["epoch"].copy(), stm["tick"].copy()))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda")  # noqa: E731
    host = lambda t, dt, shape: t.cpu().numpy().view(dt).reshape(shape)  # noqa: E731
    d_epoch, d_tick = dev(np.zeros(B, np.int32)), dev(np.zeros(B, np.int32))
    d_v, d_p, d_w = (dev(np.full((B, 6), -1.0)) for _ in range(3))
    d_base, d_win, d_masks = dev(base), dev(win), [dev(m) for m in masks]
    torch.cuda.synchronize()
    scn = mpcq.Scenario(eng, mpcq.default_scenario_params(**SC.SMALL))
    for c in range(4):  # robots_out and draw absent: the other outputs are the same
        scn.step_device(B, d_epoch.data_ptr(), d_tick.data_ptr(), d_v.data_ptr(), d_p.data_ptr(), d_w.data_ptr(),
                        first_ptr=d_masks[c].data_ptr(), all_first=c == 0, base_ptr=d_base.data_ptr(),
                        wrench_in_ptr=d_win.data_ptr(), asynchronous=False)
        v, pu, wo, epoch, tick = want[c]
        assert same(host(d_v, np.float64, (B, 6)), v) and same(host(d_p, np.float64, (B, 6)), pu), c
        assert same(host(d_w, np.float64, (B, 6)), wo), c
        assert same(host(d_epoch, np.int32, (B,)), epoch) and same(host(d_tick, np.int32, (B,)), tick), c
    # host pointers with robots_out and draw absent
    st = SM.new_state(B)
    marks = (st["robots"].copy(), st["draw"].copy())
    v, pu, wo, st = scn.step(st, all_first=True, base=base, wrench_in=win, robots_out=False, draw=False)
    assert same(v, want[0][0]) and same(pu, want[0][1]) and same(wo, want[0][2])
    assert _same_robots(st["robots"], marks[0]) and same(st["draw"], marks[1])


# ------------------------------------------------------------------------------- sessions
def _gaits():
    from mpcq import synth
    return np.stack([synth.gait_table(("trot", "bound")[b % 2], N) for b in range(SB)])


def _user_wrench():
    w = np.zeros((SB, 6))
    w[PUSHED[0]] = [5.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    w[PUSHED[1]] = [0.0, -4.0, 0.0, 0.0, 0.0, 0.2]
    return w


def _plant_table(mpcq):
    rng = np.random.default_rng(77)
    return mpcq.robots(SB, mass=rng.uniform(2.2, 2.9, SB), mu=rng.uniform(0.6, 1.0, SB))


def _snap(mpcq, sess, names):
    out = {}
    for n in names:
        read = sess.read if n.startswith("SV") else sess.plant_read if n.startswith("PV") else \
            sess.monitor_read if n.startswith("MV") else sess.scenario_read
        out[n] = read(getattr(mpcq, n))
    return out


def _order_same(a, b, ctx):
    """MPCQ_SV_ORDER of two snapshots: permutations that agree in the buckets."""
    oa, ob = a["SV_ORDER"], b["SV_ORDER"]
    assert np.array_equal(np.sort(oa), np.arange(SB)) and np.array_equal(np.sort(ob), np.arange(SB)), ctx
    key = np.where(a["SV_FIRST"] != 0, 256, np.minimum(np.maximum(a["SV_ITERS"], 0) >> 4, 255))
    assert np.array_equal(key[oa], key[ob]), ctx
    assert (np.diff(key[oa]) <= 0).all(), ctx


def _all_same(a, b, names, ctx):
    for n in names:
        if n == "SV_ORDER":
            _order_same(a, b, ctx)
        elif n == "CV_ROBOTS":
            assert _same_robots(a[n], b[n]), (ctx, n)
        else:
            assert same(a[n], b[n]), (ctx, n)


def _open(mpcq, eng, scenario=None, swing=False, monitor=True):
    """The sessions of these tests: trot and bound alternating, the rigid plant with a table and a
    user wrench on two robots, the monitor (unless monitor is False) restarting every robot after
    5 ticks; scenario = the parameters to enable, or None."""
    sess = mpcq.Session(eng, SB, gait0=_gaits())
    if swing:
        sess.enable_swing()
    sess.enable_plant()
    sess.set_wrench(_user_wrench())
    sess.set_plant_robots(_plant_table(mpcq))
    if monitor:
        sess.enable_monitor(**MON)
    if scenario is not None:
        sess.enable_scenario(**scenario)
    return sess


def _model_after_enable(p, base):
    st = SM.new_state(SB)
    SM.step(p, st, None, False, base, init=True)
    return st


def _check_cv(snap, v, pu, wo, st, ctx):
    assert same(snap["CV_V_REF"], v) and same(snap["CV_PUSH"], pu) and same(snap["CV_WRENCH"], wo), ctx
    assert same(snap["CV_EPOCH"], st["epoch"]) and same(snap["CV_TICK"], st["tick"]), ctx
    assert same(snap["CV_DRAW"], st["draw"]) and _same_robots(snap["CV_ROBOTS"], st["robots"]), ctx


def test_degenerate_scenario_is_a_constant_command(mpcq, eng):
    """v_lo == v_hi, no ramp, no period: every robot-tick commands the constant, whatever the
    robot, the epoch (the restarts after ticks 4 and 9 included) and the tick."""
    v = [0.3, 0.1, 0.0, 0.0, 0.0, 0.4]
    sc = dict(v_lo=[0.3, 0.1, 0.4], v_hi=[0.3, 0.1, 0.4], cmd_start=0, cmd_ramp=0, cmd_period=0, pushes=0, robots=0,
              seed=SC.SEED)
    names = SV + SWING + PV + MV
    with _open(mpcq, eng, sc, swing=True) as a, _open(mpcq, eng, None, swing=True) as b:
        for k in range(TICKS):
            a.tick(None)
            b.tick(v)
            _all_same(_snap(mpcq, a, names), _snap(mpcq, b, names), names, k)
            assert same(a.scenario_read(mpcq.CV_V_REF), np.tile(v, (SB, 1))), k
        assert a.monitor_read(mpcq.MV_EPISODES).tolist() == [2] * SB
        assert a.scenario_read(mpcq.CV_EPOCH).tolist() == [3] * SB


@pytest.fixture(scope="module")
def wired(mpcq, eng):
    """The small scenario on a session (snapshots "a"), a twin without scenario that the host
    feeds the model's values before each tick ("b"), and a session whose scenario has no pushes
    ("c"); with the model's values and the first flags of each tick."""
    p = SM.params(**SC.SMALL)
    base = _plant_table(mpcq)
    user = _user_wrench()
    st = _model_after_enable(p, base)
    out = []
    with _open(mpcq, eng, SC.SMALL) as a, _open(mpcq, eng, None) as b, _open(mpcq, eng, dict(SC.SMALL, pushes=0)) as c:
        enabled = _snap(mpcq, a, CV)
        for k in range(TICKS):
            first = np.ones(SB, np.int32) if k == 0 else a.read(mpcq.SV_FIRST)
            v, pu, wo, seen = SM.step(p, st, first, False, base, user)
            b.set_wrench(wo)
            b.set_plant_robots(st["robots"])
            a.tick(None)
            b.tick(v)
            c.tick(None)
            out.append(dict(a=_snap(mpcq, a, SV + PV + MV + CV), b=_snap(mpcq, b, SV + PV + MV),
                            c=_snap(mpcq, c, PV + CV), first=first, model=(v, pu, wo), seen=seen,
                            st={n: x.copy() for n, x in st.items()}))
    return dict(enabled=enabled, ticks=out, p=p, base=base, user=user)


def test_session_scenario_vs_model(mpcq, wired):
    p, base = wired["p"], wired["base"]
    st0 = _model_after_enable(p, base)
    e = wired["enabled"]  # the enable's launch: epoch 0's draw, tau = 0, nothing advanced
    assert not e["CV_EPOCH"].any() and not e["CV_TICK"].any()
    assert same(e["CV_DRAW"], st0["draw"]) and _same_robots(e["CV_ROBOTS"], st0["robots"])
    assert same(e["CV_V_REF"], np.array([SM.command(p, b, 0, 0) for b in range(SB)]))
    assert same(e["CV_WRENCH"], wired["user"]) and not e["CV_PUSH"].any()
    for k, r in enumerate(wired["ticks"]):
        v, pu, wo = r["model"]
        _check_cv(r["a"], v, pu, wo, r["st"], k)
        if k in (0, 5, 10):  # the start, and after the tick limit's resets at ticks 4 and 9
            assert (r["first"] != 0).all(), k
        assert np.array_equal(r["first"] != 0, np.array([f for _, _, f in r["seen"]])), k
    last = wired["ticks"][-1]["a"]
    # an epoch per started episode: one more than the ended ones, unless tick 11 itself ended one
    assert last["CV_EPOCH"].min() >= 3 and (last["CV_EPOCH"] + (last["MV_DONE"] != 0) == 1 + last["MV_EPISODES"]).all()


def test_session_scenario_is_the_fed_twin(wired):
    """Every session, plant and monitor array of the scenario session equals the twin's that the
    host feeds -- but MPCQ_PV_WRENCH itself: the scenario leaves the user's wrench there and
    adds its push in MPCQ_CV_WRENCH, while the twin can only be fed the sum through
    set_wrench."""
    names = tuple(n for n in SV + PV + MV if n != "PV_WRENCH")
    for k, r in enumerate(wired["ticks"]):
        _all_same(r["a"], r["b"], names, k)
        assert same(r["a"]["PV_WRENCH"], wired["user"]), k
        assert same(r["b"]["PV_WRENCH"], r["a"]["CV_WRENCH"]), k


def test_the_push_is_felt(wired):
    felt = active_ticks = 0
    for k, r in enumerate(wired["ticks"]):
        active = r["a"]["CV_PUSH"].any(axis=1)
        assert not r["c"]["CV_PUSH"].any() and same(r["c"]["CV_WRENCH"], wired["user"]), k
        # the sessions share seed, commands and robots: the same draws but the pushes
        assert same(r["c"]["CV_V_REF"], r["a"]["CV_V_REF"]) and same(r["c"]["CV_DRAW"], r["a"]["CV_DRAW"]), k
        active_ticks += int(active.sum())
        ok = ~np.isnan(r["a"]["PV_STATE_END"]).any(axis=1) & ~np.isnan(r["c"]["PV_STATE_END"]).any(axis=1)
        felt += int(((r["a"]["PV_STATE_END"] != r["c"]["PV_STATE_END"]).any(axis=1) & active & ok).sum())
        if k < 2:  # before push_first nothing differs
            assert same(r["a"]["PV_STATE_END"], r["c"]["PV_STATE_END"]), k
    assert active_ticks > 0 and felt > 0, (active_ticks, felt)
    # the robots move: true robots that differ from the plant's table in mass and mu
    r = wired["ticks"][0]["a"]["CV_ROBOTS"]
    assert (r["mass"] != wired["base"]["mass"]).all() and (r["mu"] != wired["base"]["mu"]).all()
    assert same(np.ascontiguousarray(r["fz_max"]), np.ascontiguousarray(wired["base"]["fz_max"]))


def test_run_is_the_ticks(mpcq, eng):
    import torch
    T = 8
    names = SV + PV + MV + CV
    d_trace = torch.full((T, SB, 16), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with _open(mpcq, eng, SC.SMALL) as sess:
        sess.run_device(0, T, trace_ptr=d_trace.data_ptr(), asynchronous=False)
        assert sess.k == T
        ran = _snap(mpcq, sess, names)
    trace = d_trace.cpu().numpy()
    with _open(mpcq, eng, SC.SMALL) as sess:
        for t in range(T):
            sess.tick_device(0, asynchronous=False)
            assert np.array_equal(trace[t, :, 6], sess.monitor_read(mpcq.MV_DONE)), t
        ticked = _snap(mpcq, sess, names)
    with _open(mpcq, eng, SC.SMALL) as sess:
        tr = sess.run(None, T, trace=True)
        from_python = _snap(mpcq, sess, names)
    _all_same(ran, ticked, names, "run_device")
    _all_same(from_python, ticked, names, "run")
    assert same(tr, trace)
    assert int(ran["MV_TOTALS"][0]) == T * SB and ran["CV_EPOCH"].min() >= 2


def test_reproducibility_and_explicit_reset(mpcq, eng):
    def roll(seed, reset_at=None, mask=None):
        out = []
        with mpcq.Session(eng, SB) as sess:
            sess.enable_plant()
            sess.enable_scenario(**dict(SC.SMALL, seed=seed))
            for k in range(6):
                if k == reset_at:
                    sess.reset(mask)
                sess.tick(None)
                out.append(_snap(mpcq, sess, CV + ("SV_Q_W",)))
        return out
    one, two, other = roll(SC.SEED), roll(SC.SEED), roll(SC.SEED + 1)
    for k in range(6):
        _all_same(one[k], two[k], CV + ("SV_Q_W",), k)
        assert one[k]["CV_EPOCH"].tolist() == [1] * SB and one[k]["CV_TICK"].tolist() == [k + 1] * SB
    assert not same(one[3]["CV_V_REF"], other[3]["CV_V_REF"]) and not same(one[0]["CV_DRAW"], other[0]["CV_DRAW"])
    assert same(one[0]["CV_V_REF"], other[0]["CV_V_REF"])  # (tau 0 is before the ramp: zeros for every seed)
    mask = np.zeros(SB, np.int32)
    mask[[1, 64]] = 1
    cut = roll(SC.SEED, reset_at=3, mask=mask)
    rest = np.flatnonzero(mask == 0)
    for k in range(6):
        want_epoch = np.where((mask != 0) & (k >= 3), 2, 1)
        want_tick = np.where((mask != 0) & (k >= 3), k - 2, k + 1)
        assert cut[k]["CV_EPOCH"].tolist() == want_epoch.tolist() and cut[k]["CV_TICK"].tolist() == want_tick.tolist(), k
        for n in ("CV_V_REF", "CV_PUSH", "CV_WRENCH", "CV_DRAW", "SV_Q_W"):
            assert same(cut[k][n][rest], one[k][n][rest]), (k, n)
    p = SM.params(**SC.SMALL)
    for b in (1, 64):  # the new episode's draw, from (seed, robot, epoch) alone
        assert cut[5]["CV_DRAW"][b].tolist() == list(SM.constants(p, b, 2)) + [2.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        assert cut[5]["CV_V_REF"][b].tolist() == SM.command(p, b, 2, 2)


def test_enable_disable_and_errors(mpcq, eng):
    from mpcq import _lib as L
    lib = L.lib()
    v = [0.3, 0.1, 0.0, 0.0, 0.0, 0.4]
    p = SM.params(**SC.SMALL)
    ptr = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    with _open(mpcq, eng, None, monitor=False) as sess, _open(mpcq, eng, None, monitor=False) as twin:
        buf, out = np.empty((SB, 16)), C.c_void_p()
        for what in range(7):  # before the first enable
            assert lib.mpcq_session_scenario_read(sess._h, what, ptr(buf), 0) == L.E_INVALID
            assert lib.mpcq_session_scenario_device_ptr(sess._h, what, C.byref(out)) == L.E_INVALID
        for s in (sess, twin):
            s.tick(v)
            s.tick(v)
        iters = sess.read(mpcq.SV_ITERS)
        tick_null = lambda: lib.mpcq_session_tick(sess._h, 2, None, None, None, None, 0)  # noqa: E731
        assert tick_null() == L.E_INVALID  # no scenario
        with pytest.raises(mpcq.MpcqError):
            sess.enable_scenario(cmd_period=3)  # invalid: nothing is enabled
        assert tick_null() == L.E_INVALID
        sess.enable_scenario(**dict(SC.SMALL, commands=0))
        assert tick_null() == L.E_INVALID  # a scenario that does not command
        assert lib.mpcq_session_run(sess._h, 2, 2, None, 1, None, L.FLAG_DEVICE_PTRS) == L.E_INVALID
        assert same(sess.read(mpcq.SV_ITERS), iters) and sess.scenario_read(mpcq.CV_TICK).tolist() == [0] * SB
        # enabled in mid-run (k = 2, nothing pending): epoch 0, tau counting from the enable
        sess.enable_scenario(**SC.SMALL)
        with pytest.raises(mpcq.MpcqError):
            sess.enable_scenario(robots=4)  # invalid: the parameters in force stay
        assert lib.mpcq_session_scenario_read(sess._h, 7, ptr(buf), 0) == L.E_INVALID
        assert sess.scenario_device_ptr(mpcq.CV_V_REF) != 0
        base, user = _plant_table(mpcq), _user_wrench()
        st = _model_after_enable(p, base)
        assert not sess.scenario_read(mpcq.CV_EPOCH).any() and same(sess.scenario_read(mpcq.CV_DRAW), st["draw"])
        for tau in range(3):
            vm, pu, wo, _ = SM.step(p, st, np.zeros(SB, np.int32), False, base, user)
            twin.set_wrench(wo)
            twin.set_plant_robots(st["robots"])
            sess.tick(None)
            twin.tick(vm)
            snap = _snap(mpcq, sess, CV)
            _check_cv(snap, vm, pu, wo, st, tau)
            assert snap["CV_EPOCH"].tolist() == [0] * SB and snap["CV_TICK"].tolist() == [tau + 1] * SB
            assert same(vm, np.array([SM.command(p, b, 0, tau) for b in range(SB)]))
        # a caller's v_ref wins; CV_V_REF is written all the same
        vm, pu, wo, _ = SM.step(p, st, np.zeros(SB, np.int32), False, base, user)
        twin.set_wrench(wo)
        sess.tick(v)
        twin.tick(v)
        _check_cv(_snap(mpcq, sess, CV), vm, pu, wo, st, "v_ref given")
        names = tuple(n for n in SV + PV if n != "PV_WRENCH")
        _all_same(_snap(mpcq, sess, names), _snap(mpcq, twin, names), names, "v_ref given")
        # disable: the plant is back on the user's wrench and table, the arrays stay
        sess.disable_scenario()
        assert sess.scenario_params is None
        kept = _snap(mpcq, sess, CV)
        iters = sess.read(mpcq.SV_ITERS)
        assert lib.mpcq_session_tick(sess._h, 6, None, None, None, None, 0) == L.E_INVALID
        assert same(sess.read(mpcq.SV_ITERS), iters)
        twin.set_wrench(user)
        twin.set_plant_robots(base)
        sess.tick(v)
        twin.tick(v)
        _all_same(_snap(mpcq, sess, SV + PV), _snap(mpcq, twin, SV + PV), SV + PV, "disabled")
        _all_same(_snap(mpcq, sess, CV), kept, CV, "disabled")
