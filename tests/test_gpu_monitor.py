"""GPU: the episode monitor (mpcq_monitor_step_batch, mpcq_session_enable_monitor,
mpcq_session_run) against its host model (tests/monitor_model.py), and what a session promises
around it.

Every comparison here is bit equality (monitor_model.same: NaN equals NaN, -0.0 differs from
0.0): kernel and model evaluate the same float64 operations in the same order without
contraction, and the batch totals are integers.  The one exception is MPCQ_SV_ORDER, whose order
inside a bucket of 16 iterations is left to LDS atomics by design (tests/test_gpu_plant.py)."""
import ctypes as C

import numpy as np
import pytest

import monitor_cases as MC
import monitor_model as MM

pytestmark = pytest.mark.gpu

N, SB, TICKS = 16, 65, 12  # the sessions: horizon, batch (two blocks, the second with one robot), ticks
V_REF = np.array([0.3, 0.1, 0.0, 0.0, 0.0, 0.4])
MON = dict(max_tilt=0.5, min_height=0.1, max_ticks=5)
DOWN, ROLL, BAD = (3, 64), (6, 33), 10  # the pushed robots and the one with a malformed gait
REST = np.array([b for b in range(SB) if b not in DOWN + ROLL + (BAD,)])
SV = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_L_FEET", "SV_Q_W", "SV_COST",
      "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_ROT_FLAG", "SV_H_ROT", "SV_X_ROBOT", "SV_ORDER", "SV_FIRST",
      "SV_SWING_REF", "SV_SWING_STATE", "SV_FRAME")
PV = ("PV_STATE_END", "PV_F_EFF", "PV_WRENCH")
MV = ("MV_DONE", "MV_EP", "MV_EP_TICKS", "MV_EPISODES", "MV_LAST", "MV_TOTALS")


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.fixture(scope="module")
def eng(mpcq):
    with mpcq.Engine(N) as e:
        yield e


# ------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_step_batch_vs_model(mpcq, eng, B):
    calls = MC.batch_calls(B, 500 + B)
    want = MC.model_calls(calls, B)
    mon = mpcq.Monitor(eng, mpcq.default_monitor_params(**MC.PARAMS))
    acc = None
    seen = 0
    exact = list(set(MC.exact_robots(B)))
    for c, (args, (done_w, trace_w, acc_w)) in enumerate(zip(calls, want)):
        done, acc, trace = mon.step(acc=acc, **args)
        ctx = (B, c)
        assert MM.same(done, done_w), ctx
        assert MM.same(trace, trace_w), ctx
        for name in ("ep", "ep_ticks", "episodes", "last", "totals"):
            assert MM.same(acc[name], acc_w[name]), (ctx, name)
        # sitting exactly at a threshold is no violation: these end by the tick limit alone
        assert (done[exact] == (MM.TIMEOUT if c == 1 else 0)).all(), (ctx, done[exact])
        seen |= int(np.bitwise_or.reduce(done))
    assert int(acc["totals"][0]) == MC.CALLS * B
    if B >= 63:  # (a property of the generator)
        assert seen == sum(MM.BITS), seen
        assert (acc["totals"][1:7] > 0).all()


def test_step_batch_optional_outputs_and_device_pointers(mpcq, eng):
    """(The first test of a run to put a torch tensor on the device: torch's one-time start-up,
    some 10 s that whichever test comes first pays, shows in this one's duration; the test's own
    work is one launch.)"""
    import torch
    B = 65
    args = MC.batch_calls(B, 9)[0]
    done_w, trace_w, acc_w = MC.model_calls([args], B)[0]
    mon = mpcq.Monitor(eng, mpcq.default_monitor_params(**MC.PARAMS))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda")  # noqa: E731
    acc = MM.new_state(B)
    t = {k: dev(v) for k, v in args.items()}
    ep, et, done = dev(acc["ep"]), dev(acc["ep_ticks"]), dev(np.full(B, -1, np.int32))
    torch.cuda.synchronize()
    # episodes, last, totals and trace absent: the required outputs are the same
    mon.step_device(B, t["q_w"].data_ptr(), t["status"].data_ptr(), t["iters"].data_ptr(), t["f0"].data_ptr(),
                    t["cost"].data_ptr(), t["state"].data_ptr(), t["v_ref"].data_ptr(), ep.data_ptr(),
                    et.data_ptr(), done.data_ptr(), asynchronous=False)
    assert MM.same(done.cpu().numpy().view(np.int32), done_w)
    assert MM.same(ep.cpu().numpy().view(np.float64).reshape(B, 8), acc_w["ep"])
    assert MM.same(et.cpu().numpy().view(np.int32), acc_w["ep_ticks"])


def test_invalid_arguments(mpcq, eng):
    from mpcq import _lib as L
    lib = L.lib()
    B = 3
    a = MC.batch_calls(B, 1)[0]
    acc = MM.new_state(B)
    done = np.full(B, -7, np.int32)
    p = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731

    def call(mp, **absent):
        v = dict(q_w=a["q_w"], status=a["status"], iters=a["iters"], f0=a["f0"], cost=a["cost"], state=a["state"],
                 v_ref=a["v_ref"], ep=acc["ep"], ep_ticks=acc["ep_ticks"], done=done)
        v.update(absent)
        g = lambda k: None if v[k] is None else p(v[k])  # noqa: E731
        return lib.mpcq_monitor_step_batch(eng._h, C.byref(mp), B, g("q_w"), g("status"), g("iters"), g("f0"),
                                           g("cost"), g("state"), g("v_ref"), g("ep"), g("ep_ticks"), None, None,
                                           g("done"), None, None, 0)
    for bad in (dict(max_tilt=0.0), dict(max_tilt=-0.5), dict(max_tilt=np.nan), dict(min_height=np.nan),
                dict(min_height=np.inf), dict(max_ticks=-1), dict(auto_reset=2), dict(auto_reset=-1)):
        assert call(mpcq.default_monitor_params(**bad)) == L.E_INVALID, bad
    ok = mpcq.default_monitor_params()
    for k in ("q_w", "status", "iters", "f0", "cost", "state", "v_ref", "ep", "ep_ticks", "done"):
        assert call(ok, **{k: None}) == L.E_INVALID, k
    assert (done == -7).all() and acc["ep_ticks"].tolist() == [0] * B  # nothing was launched
    assert call(mpcq.default_monitor_params(max_tilt=np.inf, min_height=-np.inf)) == 0
    assert (done != -7).all() and acc["ep_ticks"].max() <= 1
    with mpcq.Session(eng, 2) as sess:
        buf = np.empty((2, 16))
        out = C.c_void_p()
        for what in range(6):  # before the first enable
            assert lib.mpcq_session_monitor_read(sess._h, what, p(buf), 0) == L.E_INVALID
            assert lib.mpcq_session_monitor_device_ptr(sess._h, what, C.byref(out)) == L.E_INVALID
        with pytest.raises(mpcq.MpcqError):
            sess.enable_monitor(max_tilt=-1.0)
        sess.enable_monitor()
        ep = sess.monitor_read(mpcq.MV_EP)
        assert ep[:, 4].tolist() == [np.inf, np.inf] and not np.delete(ep, 4, axis=1).any()
        for what in (mpcq.MV_DONE, mpcq.MV_EP_TICKS, mpcq.MV_EPISODES, mpcq.MV_LAST, mpcq.MV_TOTALS):
            assert not sess.monitor_read(what).any(), what
        assert lib.mpcq_session_monitor_read(sess._h, 6, p(buf), 0) == L.E_INVALID
        assert lib.mpcq_session_monitor_read(sess._h, 0, None, 0) == L.E_INVALID
        sess.disable_monitor()
        assert sess.monitor_read(mpcq.MV_EP_TICKS).tolist() == [0, 0]  # the arrays stay


# ------------------------------------------------------------------------------- sessions
def _gaits():
    from mpcq import synth
    g = np.stack([synth.gait_table(("trot", "bound")[b % 2], N) for b in range(SB)])
    g[BAD, :, 0] = 1.0  # no terminator: MPCQ_STATUS_BAD_GAIT on every tick
    return g


def _wrench():
    w = np.zeros((SB, 6))
    w[list(DOWN), 2] = -MC.DOWN_FORCE
    w[list(ROLL), 3] = MC.ROLL_TORQUE
    return w


def _snap(mpcq, sess, monitor):
    out = {n: sess.read(getattr(mpcq, n)) for n in SV}
    out.update({n: sess.plant_read(getattr(mpcq, n)) for n in PV})
    if monitor:
        out.update({n: sess.monitor_read(getattr(mpcq, n)) for n in MV})
    return out


def _open(mpcq, eng, monitor=None):
    """The sessions of these tests: trot and bound alternating, the rigid plant, swing, the
    pushes and the malformed gait; monitor = the overrides of MON, or None for no monitor."""
    sess = mpcq.Session(eng, SB, gait0=_gaits())
    sess.enable_swing()
    sess.enable_plant()
    sess.set_wrench(_wrench())
    if monitor is not None:
        sess.enable_monitor(**dict(MON, **monitor))
    return sess


def _run(mpcq, eng, monitor=None, after=None, ticks=TICKS):
    """Snapshots after every tick (after(sess) first, if given)."""
    out = []
    with _open(mpcq, eng, monitor) as sess:
        for _ in range(ticks):
            sess.tick(V_REF)
            if after:
                after(sess)
            out.append(_snap(mpcq, sess, monitor is not None))
    return out


@pytest.fixture(scope="module")
def plain(mpcq, eng):
    return _run(mpcq, eng)


@pytest.fixture(scope="module")
def monitored(mpcq, eng):
    return _run(mpcq, eng, monitor=dict(auto_reset=0))


@pytest.fixture(scope="module")
def auto(mpcq, eng):
    return _run(mpcq, eng, monitor=dict(auto_reset=1))


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
        else:
            assert MM.same(a[n], b[n]), (ctx, n)


def test_session_vs_model(mpcq, monitored):
    """After every tick the monitor's arrays are the model's, fed the session's own arrays, and
    each reason occurs where it was prepared.

    The pushes (monitor_cases.DOWN_FORCE = 250 N down, ROLL_TORQUE = 25 N m about x) are sized
    with tests/plant_model.py under the assumption that every foot is in stance and resists with
    its fz_max, the most the plant's clamp lets through: the base is then at z = 0.075 after 3
    ticks and -0.023 after 4 (threshold 0.10: crossed with 0.025 m to spare a tick early, 0.123 m
    at the fourth), the roll at 1.04 rad after 3 ticks and 1.83 after 4 (threshold 0.5);
    tests/test_monitor_model.py keeps that computation honest on the CPU."""
    acc = MM.new_state(SB)
    done_at = np.zeros((TICKS, SB), np.int32)
    for k, r in enumerate(monitored):
        done, _ = MM.step(r["SV_Q_W"], r["SV_STATUS"], r["SV_ITERS"], r["SV_F0"], r["SV_COST"], r["SV_STATE"], V_REF,
                          acc, **MON)
        done_at[k] = done
        assert MM.same(r["MV_DONE"], done), k
        assert MM.same(r["MV_EP"], acc["ep"]), k
        assert MM.same(r["MV_EP_TICKS"], acc["ep_ticks"]), k
        assert MM.same(r["MV_EPISODES"], acc["episodes"]), k
        assert MM.same(r["MV_LAST"], acc["last"]), k
        assert MM.same(r["MV_TOTALS"], acc["totals"]), k
    for b in DOWN:
        assert (done_at[:4, b] & MM.HEIGHT).any(), (b, done_at[:4, b])
    for b in ROLL:
        assert (done_at[:4, b] & MM.TILT).any(), (b, done_at[:4, b])
    assert (done_at[:, BAD] & MM.SOLVER).all() and (monitored[0]["SV_STATUS"][BAD] == mpcq.STATUS_BAD_GAIT)
    rest = done_at[:, REST]
    assert (rest[[4, 9]] == MM.TIMEOUT).all() and not np.delete(rest, [4, 9], axis=0).any(), rest
    assert int(monitored[-1]["MV_TOTALS"][0]) == TICKS * SB


def test_monitor_does_not_interfere(plain, monitored):
    for k in range(TICKS):
        _all_same(plain[k], monitored[k], SV + PV, k)


def test_auto_reset_is_the_callers_reset(mpcq, eng, auto):
    """auto_reset = 1 against auto_reset = 0 with reset_device(MV_DONE) after every tick."""
    def after(sess):
        sess.reset_device(sess.monitor_device_ptr(mpcq.MV_DONE))
    manual = _run(mpcq, eng, monitor=dict(auto_reset=0), after=after)
    resets = 0
    for k in range(TICKS):
        _all_same(auto[k], manual[k], SV + PV + MV, k)
        d = auto[k]["MV_DONE"] != 0
        resets += int(d.sum())
        assert np.array_equal(auto[k]["SV_FIRST"], d.astype(np.int32)), k
        stand = np.zeros(12)
        stand[2] = MC.H_REF
        assert (auto[k]["SV_STATE"][d] == stand).all(), k
        if k + 1 < TICKS:  # the tick after a reset is the robot's first tick again
            assert np.array_equal(auto[k + 1]["SV_STATUS"][d], auto[0]["SV_STATUS"][d]), k
            assert np.array_equal(auto[k + 1]["SV_ITERS"][d], auto[0]["SV_ITERS"][d]), k
    last = auto[-1]
    assert resets == int(last["MV_TOTALS"][1]) == int(last["MV_EPISODES"].sum())
    assert (last["MV_EPISODES"][REST] == 2).all() and last["MV_EPISODES"][BAD] == TICKS
    # the terminal pose survives the reset
    for b in DOWN:
        assert last["MV_LAST"][b, 12] < MON["min_height"] and int(last["MV_LAST"][b, 9]) & MM.HEIGHT
    for b in ROLL:
        assert abs(last["MV_LAST"][b, 13]) > MON["max_tilt"] and int(last["MV_LAST"][b, 9]) & MM.TILT


def test_explicit_reset_discards_the_running_episode(mpcq, eng):
    with mpcq.Session(eng, SB) as sess:
        sess.enable_monitor(max_tilt=0.5, min_height=0.1, max_ticks=2)
        for _ in range(3):
            sess.tick(V_REF)
        before = {n: sess.monitor_read(getattr(mpcq, n)) for n in MV}
        assert (before["MV_EPISODES"] == 1).all() and (before["MV_EP_TICKS"] == 1).all()
        assert (before["MV_LAST"][:, 8] == 2.0).all() and (before["MV_EP"][:, 2] > 0).all()
        mask = np.zeros(SB, np.int32)
        mask[[1, 64]] = 1
        sess.reset(mask)
        after = {n: sess.monitor_read(getattr(mpcq, n)) for n in MV}
        want = {n: v.copy() for n, v in before.items()}
        want["MV_EP"][[1, 64]] = [0.0, 0.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0]
        want["MV_EP_TICKS"][[1, 64]] = 0
        for n in MV:
            assert MM.same(after[n], want[n]), n
        sess.tick(V_REF)
        assert sess.monitor_read(mpcq.MV_EP_TICKS).tolist() == [0 if b not in (1, 64) else 1 for b in range(SB)]
        assert sess.monitor_read(mpcq.MV_EPISODES).tolist() == [2 if b not in (1, 64) else 1 for b in range(SB)]


@pytest.mark.parametrize("auto_reset", [0, 1])
def test_run_is_the_ticks(mpcq, eng, auto_reset):
    import torch
    T = 8
    rng = np.random.default_rng(4)
    sched = np.tile(V_REF, (3, SB, 1)) + rng.uniform(-0.05, 0.05, (3, SB, 6))
    d_sched = torch.from_numpy(sched).to("cuda")
    d_trace = torch.full((T, SB, 16), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    mon = dict(auto_reset=auto_reset)
    with _open(mpcq, eng, mon) as sess:
        sess.run_device(d_sched.data_ptr(), T, v_ref_ticks=3, trace_ptr=d_trace.data_ptr(), asynchronous=False)
        assert sess.k == T
        ran = _snap(mpcq, sess, True)
    trace = d_trace.cpu().numpy()
    acc = MM.new_state(SB)
    with _open(mpcq, eng, mon) as sess:
        for t in range(T):
            row = d_sched[min(t, 2)]
            sess.tick_device(row.data_ptr(), asynchronous=False)
            done = sess.monitor_read(mpcq.MV_DONE)
            assert np.array_equal(trace[t, :, 6], done), t
            if auto_reset:  # the pose the reset wiped is in the trace and in MV_LAST
                d = done != 0
                assert MM.same(trace[t, d, 0:6], sess.monitor_read(mpcq.MV_LAST)[d, 10:16]), t
                assert MM.same(trace[t, ~d, 0:6], sess.read(mpcq.SV_Q_W)[~d]), t
            else:  # the whole row, by the model from the tick's arrays
                r = {n: sess.read(getattr(mpcq, n)) for n in ("SV_Q_W", "SV_STATUS", "SV_ITERS", "SV_F0", "SV_COST",
                                                             "SV_STATE")}
                _, want = MM.step(r["SV_Q_W"], r["SV_STATUS"], r["SV_ITERS"], r["SV_F0"], r["SV_COST"], r["SV_STATE"],
                                  sched[min(t, 2)], acc, **MON)
                assert MM.same(trace[t], want), t
        ticked = _snap(mpcq, sess, True)
    _all_same(ran, ticked, SV + PV + MV, "final")
    assert int(ran["MV_TOTALS"][0]) == T * SB


def test_run_invalid_arguments(mpcq, eng):
    import torch
    from mpcq import _lib as L
    lib = L.lib()
    d_v = torch.from_numpy(np.tile(V_REF, (SB, 1))).to("cuda")
    d_trace = torch.zeros((2, SB, 16), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    host_v = np.tile(V_REF, (SB, 1))
    v, tr = C.c_void_p(d_v.data_ptr()), C.c_void_p(d_trace.data_ptr())
    DEV = L.FLAG_DEVICE_PTRS
    with mpcq.Session(eng, SB) as sess:
        names = ("SV_Q_W", "SV_STATUS", "SV_ITERS", "SV_X", "SV_GAIT")
        before = {n: sess.read(getattr(mpcq, n)) for n in names}
        run = lambda *a: lib.mpcq_session_run(sess._h, *a)  # noqa: E731
        assert run(0, 2, v, 1, tr, DEV) == L.E_INVALID  # a trace without a monitor
        sess.enable_monitor()
        sess.disable_monitor()
        assert run(0, 2, v, 1, tr, DEV) == L.E_INVALID  # ... or with a disabled one
        sess.enable_monitor()
        assert run(0, 0, v, 1, tr, DEV) == L.E_INVALID
        assert run(0, -1, v, 1, None, DEV) == L.E_INVALID
        assert run(-1, 2, v, 1, None, DEV) == L.E_INVALID
        assert run(0, 2, v, 0, None, DEV) == L.E_INVALID
        assert run(0, 2, None, 1, None, DEV) == L.E_INVALID
        assert run(0, 2, C.c_void_p(host_v.ctypes.data), 1, None, 0) == L.E_INVALID  # host pointers
        assert run(0, 2, C.c_void_p(host_v.ctypes.data), 1, None, L.FLAG_ASYNC) == L.E_INVALID
        for n in names:  # nothing was launched
            assert MM.same(sess.read(getattr(mpcq, n)), before[n]), n
        assert not sess.monitor_read(mpcq.MV_TOTALS).any() and not d_trace.cpu().numpy().any()
        assert run(0, 2, v, 1, tr, DEV) == 0
        assert sess.monitor_read(mpcq.MV_TOTALS)[0] == 2 * SB and (d_trace.cpu().numpy()[:, :, 9] == [[1.0], [2.0]]).all()
