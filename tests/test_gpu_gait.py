"""GPU: the gait stage (mpcq_gait_roll_batch, mpcq_gait.hip; Session.enable_gait) against the host
model (tests/gait_model.py) and, in closed loop, against the oracle's pieces composed with the
model's roll (tests/gait_cases.py).

Every comparison is bit equality (monitor_model.same: NaN equals NaN, -0.0 differs from 0.0) but
two: MPCQ_SV_ORDER, whose order inside a bucket of 16 iterations is left to LDS atomics by
design, and f0 / x against the oracle's closed loop, within tests/test_gpu_session.py's SOLVE_TOL."""
import struct

import numpy as np
import pytest

import gait_cases as GC
import gait_model as GM
from monitor_model import same

pytestmark = pytest.mark.gpu

SV = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_L_FEET", "SV_Q_W", "SV_COST",
      "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_ROT_FLAG", "SV_H_ROT", "SV_X_ROBOT", "SV_ORDER", "SV_FIRST")
V_REF = np.array([0.3, 0.0, 0.0, 0.0, 0.0, 0.1])


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.fixture(scope="module")
def eng(mpcq):
    with mpcq.Engine(16) as e:
        yield e


def _sv(mpcq, sess, names=SV):
    return {n: sess.read(getattr(mpcq, n)) for n in names}


def _order_same(a, b, ctx):
    """MPCQ_SV_ORDER of two sessions: permutations that agree in the buckets."""
    oa, ob = a["SV_ORDER"], b["SV_ORDER"]
    n = oa.shape[0]
    assert np.array_equal(np.sort(oa), np.arange(n)) and np.array_equal(np.sort(ob), np.arange(n)), ctx
    key = np.where(a["SV_FIRST"] != 0, 256, np.minimum(np.maximum(a["SV_ITERS"], 0) >> 4, 255))
    assert np.array_equal(key[oa], key[ob]), ctx


def _all_same(a, b, ctx, rows=None):
    for n in a:
        if n == "SV_ORDER":
            if rows is None:
                _order_same(a, b, ctx)
            continue
        x, y = (a[n], b[n]) if rows is None else (np.ascontiguousarray(a[n][rows]), np.ascontiguousarray(b[n][rows]))
        assert same(x, y), (ctx, n)


# ------------------------------------------------------------------------------- the kernel alone
def _batch_case(B, select, align, seed):
    rng = np.random.default_rng(seed)
    gait, state = GC.random_tables(rng, B)
    if select == GM.BY_SPEED:
        p = GM.params(n_gaits=4, select=select, align=align, thresholds=GC.THRESHOLDS, hysteresis=GC.HYSTERESIS)
        lib = GC.SPEED_LIB
    else:
        p = GM.params(n_gaits=4, select=select, align=align)
        lib = GC.LIB
    v = [GC.speed_vrefs(rng, B) for _ in range(3)]
    return p, lib, v, gait, state


def _gpu_params(mpcq, p):
    return mpcq.default_gait_params(n_gaits=p.n_gaits, select=p.select, align=p.align, thresholds=p.thresholds,
                                    hysteresis=p.hysteresis, yaw_weight=p.yaw_weight)


@pytest.mark.parametrize("B", [1, 2, 3, 63, 64, 65, 129])
def test_roll_batch_vs_model(mpcq, eng, B):
    """Three consecutive calls that carry table and state, host pointers and device pointers,
    both select modes and both align values.  (Run alone, its first case pays torch's one-time
    start-up on the device, some 10 s; the case's own work is two dozen launches.)"""
    import torch
    kinds = set()
    for select in (GM.MANUAL, GM.BY_SPEED):
        for align in (0, 1):
            p, lib, v, gait, state = _batch_case(B, select, align, 1000 * B + 10 * select + align)
            g = mpcq.Gait(eng, lib, _gpu_params(mpcq, p))
            wg, ws = gait.copy(), state.copy()
            hg, hs = gait.copy(), state.copy()
            dg, ds = torch.from_numpy(gait.copy()).to("cuda"), torch.from_numpy(state.copy()).to("cuda")
            for call in range(3):
                before = ws.copy()
                GM.roll(p, lib, v[call], wg, ws)
                kinds |= {"switch"} if (ws[:, 3] != before[:, 3]).any() else set()
                kinds |= {"untouched"} if (wg[:, :, 0] != 0).all(axis=1).any() else set()
                vr = v[call] if select == GM.BY_SPEED or call == 1 else None  # MANUAL: v_ref may be absent
                g.roll(hg, hs, vr)
                ctx = (B, select, align, call)
                assert same(hg, wg) and np.array_equal(hs, ws), ctx
                dv = None if vr is None else torch.from_numpy(vr).to("cuda")
                torch.cuda.synchronize()
                g.roll_device(B, dg.data_ptr(), ds.data_ptr(), 0 if dv is None else dv.data_ptr(), asynchronous=False)
                assert same(dg.cpu().numpy(), wg) and np.array_equal(ds.cpu().numpy(), ws), ctx
    if B >= 63:
        assert kinds == {"switch", "untouched"}


def test_each_robot_gets_the_bits_it_gets_alone(mpcq, eng):
    for select in (GM.MANUAL, GM.BY_SPEED):
        p, lib, v, gait, state = _batch_case(3, select, 1, 77 + select)
        g = mpcq.Gait(eng, lib, _gpu_params(mpcq, p))
        tg, ts = gait.copy(), state.copy()
        g.roll(tg, ts, v[0])
        for b in range(3):
            og, os_ = gait[b:b + 1].copy(), state[b:b + 1].copy()
            g.roll(og, os_, v[0][b:b + 1])
            assert same(og[0], tg[b]) and np.array_equal(os_[0], ts[b]), (select, b)


# ------------------------------------------------------------------------------- sessions
def _mixed(N, B):
    from mpcq import synth
    return np.stack([synth.gait_table(("trot", "bound", "pace")[b % 3], N) for b in range(B)])


def _v_ref(B, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, .6, B), rng.uniform(-.1, .1, B), np.zeros(B), np.zeros(B), np.zeros(B),
                     rng.uniform(-.3, .3, B)], axis=1)


@pytest.mark.parametrize("N", [16, 8])
def test_a_enabled_and_nobody_requesting_changes_nothing(mpcq, N):
    B = 5
    gaits, v = _mixed(N, B), _v_ref(B, 3)
    with mpcq.Engine(N) as e, mpcq.Session(e, B, gait0=gaits) as plain, mpcq.Session(e, B, gait0=gaits) as sess:
        sess.enable_gait(["trot", "bound", "stand"])
        assert np.array_equal(sess.gait_state(), GM.new_state(B))
        for k in range(12):
            plain.tick(v)
            sess.tick(v)
            _all_same(_sv(mpcq, sess), _sv(mpcq, plain), (N, k))
        assert np.array_equal(sess.gait_state(), GM.new_state(B))


@pytest.mark.parametrize("N", [16, 32])
def test_b_own_cycle_is_the_plain_session(mpcq, N):
    """Every robot requests its own table's cycle, P | N: bit-identical to the plain session."""
    B, names = 3, ("trot", "bound", "pace")
    gaits, v = _mixed(N, B), _v_ref(B, 4)
    with mpcq.Engine(N) as e, mpcq.Session(e, B, gait0=gaits) as plain, mpcq.Session(e, B, gait0=gaits) as sess:
        sess.enable_gait(list(names))
        sess.set_gait([0, 1, 2])
        for k in range(20 if N == 16 else 10):
            plain.tick(v)
            sess.tick(v)
            _all_same(_sv(mpcq, sess), _sv(mpcq, plain), (N, k))
        st = sess.gait_state()
        assert np.array_equal(st[:, :2], [[0, 0], [1, 1], [2, 2]]) and (st[:, 3] == 1).all()


def test_c_transitions_vs_model_and_oracle(mpcq, eng):
    """The trot -> bound -> stand -> trot schedule, robots requesting at different ticks, robot 4
    never: tables and rows are the model's after every tick, statuses and iteration counts the
    composed oracle loop's, f0 and x within SOLVE_TOL of it, robot 4 its row of a plain session."""
    from test_gpu_session import SOLVE_TOL
    B, never = 5, 4
    rec = GC.closed_loop(B, never)
    reqs = GC.requests(B, never)
    g0 = np.stack([GC.table("trot", 16)] * B)
    v = np.tile(GC.CLOSED_V_REF, (B, 1))
    worst = dict(f0=0.0, x=0.0)
    with mpcq.Session(eng, B, gait0=g0) as plain, mpcq.Session(eng, B, gait0=g0) as sess:
        sess.enable_gait(GC.LIB[:3])
        want = np.full(B, -1, np.int32)
        for k in range(GC.SCHEDULE_TICKS):
            if k in reqs:
                want = np.where(reqs[k] != -2, reqs[k], want).astype(np.int32)
                sess.set_gait(want)
            sess.tick(v)
            plain.tick(v)
            a = _sv(mpcq, sess)
            assert same(a["SV_GAIT"], rec["gait"][k]), k
            assert np.array_equal(sess.gait_state(), rec["state"][k]), k
            want = rec["state"][k][:, 0].copy()
            worst["f0"] = max(worst["f0"], float(np.abs(a["SV_F0"] - rec["f0"][k]).max()))
            worst["x"] = max(worst["x"], float(np.abs(a["SV_X"] - rec["x"][k]).max()))
            assert np.array_equal(a["SV_STATUS"], rec["status"][k]), (k, a["SV_STATUS"], rec["status"][k])
            assert np.array_equal(a["SV_ITERS"], rec["iters"][k]), (k, a["SV_ITERS"], rec["iters"][k])
            _all_same(a, _sv(mpcq, plain), (k, "never"), rows=[never])
    print(f"transitions: max |f0 - oracle| = {worst['f0']:.3e}, max |x - oracle| = {worst['x']:.3e} over "
          f"{GC.SCHEDULE_TICKS} ticks (SOLVE_TOL {SOLVE_TOL:g})")
    assert worst["f0"] <= SOLVE_TOL and worst["x"] <= SOLVE_TOL


def test_d_period_not_dividing_the_horizon(mpcq):
    """N = 12, T_gait 0.24, the period-8 trot cycle: the table is the model's, and differs from a
    plain session's first at tick 4."""
    B = 2
    g0 = np.stack([GC.table("trot", 12, half=6)] * B)
    lib = np.stack([GC.cycle("trot", half=4)])
    v = np.tile(V_REF, (B, 1))
    with mpcq.Engine(12) as e:
        pp = mpcq.default_planner_params(dt=e.params.dt, T_gait=0.24)
        with mpcq.Session(e, B, gait0=g0, planner_params=pp) as plain, \
                mpcq.Session(e, B, gait0=g0, planner_params=pp) as sess:
            sess.enable_gait(lib)
            sess.set_gait([0, -1])
            reqs = {0: np.array([0, -2], np.int32)}
            gs, ss = GC.model_run(g0, lib, GM.params(n_gaits=1), 12, reqs)
            eq = []
            for k in range(12):
                sess.tick(v)
                plain.tick(v)
                g = sess.read(mpcq.SV_GAIT)
                assert same(g, gs[k]) and np.array_equal(sess.gait_state(), ss[k]), k
                pg = plain.read(mpcq.SV_GAIT)
                assert same(g[1], pg[1]), k
                eq.append(bool(same(g[0], pg[0])))
            assert eq[:4] == [True] * 4 and not eq[4]


def test_e_row_overflow_ends_as_bad_gait(mpcq):
    """N = 20, [1 all][9 A][1 all][9 B], one robot requesting the period-2 cycle [1 A][1 B]: the
    table runs out of zero rows at the tick the model predicts; the neighbours are untouched."""
    B, T = 3, 24
    g0 = np.stack([GC.table("trot", 20, half=10)] * B)
    lib = np.zeros((1, 20, 5))
    lib[0, 0] = (1, *GC.MASKS["trot"][1])
    lib[0, 1] = (1, *GC.MASKS["trot"][3])
    reqs = {0: np.array([-2, 0, -2], np.int32)}
    gs, ss = GC.model_run(g0, lib, GM.params(n_gaits=1), T, reqs)
    # the planner's test after the roll: a terminator among rows 1..19
    full = [k for k in range(T) if (gs[k, 1, 1:, 0] != 0).all()]
    assert full and 0 < full[0] < T
    print(f"row overflow: the model's table has no zero row from tick {full[0]} on")
    v = np.tile(V_REF, (B, 1))
    with mpcq.Engine(20) as e:
        pp = mpcq.default_planner_params(dt=e.params.dt, T_gait=0.4)
        with mpcq.Session(e, B, gait0=g0, planner_params=pp) as plain, \
                mpcq.Session(e, B, gait0=g0, planner_params=pp) as sess:
            sess.enable_gait(lib)
            sess.set_gait([-1, 0, -1])
            for k in range(T):
                sess.tick(v)
                plain.tick(v)
                a = _sv(mpcq, sess)
                assert same(a["SV_GAIT"], gs[k]) and np.array_equal(sess.gait_state(), ss[k]), k
                assert (a["SV_STATUS"][1] == mpcq.STATUS_BAD_GAIT) == (k >= full[0]), (k, a["SV_STATUS"])
                _all_same(a, _sv(mpcq, plain), k, rows=[0, 2])


def test_f_reset_and_auto_reset(mpcq, eng):
    import torch
    B = 6
    g0, v = _mixed(16, B), np.tile(V_REF, (B, 1))
    with mpcq.Session(eng, B, gait0=g0) as sess:
        sess.enable_gait(GC.LIB[:3])
        sess.set_gait([1, 2, 0, 1, -1, 2])
        for k in range(5):
            sess.tick(v)
        before = sess.gait_state()
        assert (before[[0, 1, 3, 5], 1] >= 0).all()
        sess.set_gait([0, 0, 1, 0, 1, 0])  # mid-transition: requests not taken yet
        mask = np.array([1, 0, 0, 1, 0, 0], np.int32)
        sess.reset(mask)
        st, g = sess.gait_state(), sess.read(mpcq.SV_GAIT)
        assert np.array_equal(st[[0, 3]], GM.new_state(2)) and same(g[[0, 3]], g0[[0, 3]])
        assert np.array_equal(st[[1, 2, 4, 5], 1:], before[[1, 2, 4, 5], 1:]) and st[1, 0] == 0
    # the monitor's auto-reset against auto_reset = 0 plus reset_device(MV_DONE)
    reqs = GC.requests(B, never=5, stagger=1)
    with mpcq.Session(eng, B, gait0=g0) as auto, mpcq.Session(eng, B, gait0=g0) as manual:
        for s, ar in ((auto, 1), (manual, 0)):
            s.enable_gait(GC.LIB[:3])
            s.enable_monitor(max_ticks=5, auto_reset=ar)
        done = manual.monitor_device_ptr(mpcq.MV_DONE)
        ends = 0
        for k in range(14):
            if k in reqs:
                ids = np.where(reqs[k] != -2, reqs[k], auto.gait_state()[:, 0]).astype(np.int32)
                auto.set_gait(ids)
                manual.set_gait(ids)
            auto.tick(v)
            manual.tick(v)
            manual.reset_device(mask_ptr=done, asynchronous=False)
            torch.cuda.synchronize()
            ends += int((auto.monitor_read(mpcq.MV_DONE) != 0).sum())
            _all_same(_sv(mpcq, auto), _sv(mpcq, manual), k)
            assert np.array_equal(auto.gait_state(), manual.gait_state()), k
            if (auto.monitor_read(mpcq.MV_DONE) != 0).all():
                assert np.array_equal(auto.gait_state(), GM.new_state(B)), k
        assert ends >= 2 * B


def test_g_selection_by_speed_under_a_scenario(mpcq, eng):
    """BY_SPEED on a scenario's ramp from rest, stand / trot / bound: rows and tables are the
    model's, fed the scenario's own v_ref, at every tick; some robot visits all three gaits."""
    B, T = 5, 40
    g0 = np.stack([GC.table("stand", 16)] * B)
    lib = np.stack([GC.cycle("stand"), GC.cycle("trot"), GC.cycle("bound")])
    p = GM.params(n_gaits=3, select=GM.BY_SPEED, thresholds=(0.125, 0.5), hysteresis=0.03125)
    with mpcq.Session(eng, B, gait0=g0) as sess:
        sess.enable_scenario(seed=5, commands=1, cmd_start=2, cmd_ramp=24, cmd_period=0, v_lo=[0.7, -0.05, -0.2],
                             v_hi=[0.9, 0.05, 0.2])
        sess.enable_gait(lib, _gpu_params(mpcq, p))
        with pytest.raises(mpcq.MpcqError):  # the kernel owns want
            sess.set_gait(1)
        wg, ws = g0.copy(), GM.new_state(B)
        visited = [set() for _ in range(B)]
        for k in range(T):
            sess.tick()
            v = sess.scenario_read(mpcq.CV_V_REF)
            GM.roll(p, lib, v, wg, ws)
            assert same(sess.read(mpcq.SV_GAIT), wg) and np.array_equal(sess.gait_state(), ws), k
            for b in range(B):
                visited[b].add(int(ws[b, 1]))
        # (the model, fed the commands, says so first; the device's rows equal it)
        assert any(vis >= {0, 1, 2} for vis in visited), visited


def test_h_swing_follows_the_transition(mpcq, eng):
    B, T = 3, 14
    g0, v = np.stack([GC.table("trot", 16)] * B), np.tile(V_REF, (B, 1))
    with mpcq.Session(eng, B, gait0=g0) as sess:
        sess.enable_swing()
        sess.enable_gait(GC.LIB[:3])
        sess.set_gait([1, -1, 2])
        sw = mpcq.Swing(eng, B)
        for k in range(T):
            sess.tick(v)
            frame = sess.read(mpcq.SV_FRAME)
            want = sw.advance(sess.read(mpcq.SV_GAIT), sess.read(mpcq.SV_FSTEPS), frame, 0, 20, feet0=None)
            assert np.array_equal(sess.read(mpcq.SV_SWING_REF), want, equal_nan=True), k
            assert np.array_equal(sess.read(mpcq.SV_SWING_STATE), sw.state), k
        assert np.array_equal(sess.gait_state()[:, 1], [1, -1, 2])


# ------------------------------------------------------------------------------- snapshots
GROUPS = (("read", SV + ("SV_SWING_REF", "SV_SWING_STATE", "SV_FRAME")),
          ("plant_read", ("PV_STATE_END", "PV_F_EFF", "PV_WRENCH")),
          ("monitor_read", ("MV_DONE", "MV_EP", "MV_EP_TICKS", "MV_EPISODES", "MV_LAST", "MV_TOTALS")),
          ("scenario_read", ("CV_EPOCH", "CV_TICK", "CV_V_REF", "CV_PUSH", "CV_WRENCH", "CV_ROBOTS", "CV_DRAW")),
          ("channel_read", ("HV_CLOCK", "HV_OBS", "HV_F_CMD", "HV_DRAW", "HV_S_RING", "HV_F_RING")),
          ("estimator_read", ("EV_ROW",)))


def _everything(mpcq, eng, B):
    """A session with every group enabled: 49 per-robot arrays in a snapshot."""
    import scenario_cases as SC
    sess = mpcq.Session(eng, B, gait0=_mixed(16, B))
    sess.enable_swing()
    sess.enable_plant()
    w = np.zeros((B, 6))
    w[1] = [5.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    sess.set_wrench(w)
    rng = np.random.default_rng(77)
    sess.set_robots(mpcq.robots(B, mass=rng.uniform(2.3, 2.7, B), mu=rng.uniform(0.7, 1.0, B)))
    sess.set_plant_robots(mpcq.robots(B, mass=rng.uniform(2.2, 2.9, B), mu=rng.uniform(0.6, 1.0, B)))
    sess.enable_monitor(max_ticks=50)
    sess.enable_scenario(**SC.SMALL)
    sess.enable_channel(delay=2, latency=1, sigma=1e-3)
    sess.enable_estimator(lag=2, f_lag=1)
    sess.enable_gait(GC.LIB[:3])
    return sess


def _read_all(mpcq, sess, groups=GROUPS):
    out = {}
    for fn, names in groups:
        for n in names:
            a = getattr(sess, fn)(getattr(mpcq, n))
            out[n] = a.view(np.uint8).reshape(a.shape[0], -1) if a.dtype.names else a
    out["GV_STATE"] = sess.gait_state()
    return out


def _same_reads(a, b, ctx, rows_a=None, rows_b=None):
    for n in a:
        if n == "SV_ORDER" or (n == "MV_TOTALS" and rows_a is not None):
            continue
        x = a[n] if rows_a is None else a[n][rows_a]
        y = b[n] if rows_b is None else b[n][rows_b]
        assert same(np.ascontiguousarray(x), np.ascontiguousarray(y)), (ctx, n)


@pytest.mark.parametrize("full", [False, True], ids=["gait-only", "every-group"])
def test_i_snapshot_restore_and_fork(mpcq, eng, full):
    """Save mid-transition, run 6 ticks, restore, run the same 6: the same bits; fork copies the
    row.  With every group enabled the restore gathers 49 arrays: two launches."""
    B = 5
    v = np.tile(V_REF, (B, 1))
    groups = GROUPS if full else (("read", SV),)
    with (_everything(mpcq, eng, B) if full else mpcq.Session(eng, B, gait0=_mixed(16, B))) as sess:
        if not full:
            sess.enable_gait(GC.LIB[:3])
        sess.set_gait([1, 2, -1, 0, 1])
        for k in range(5):
            sess.tick(None if full else v)
        sess.set_gait([0, 0, 1, 1, 2])  # requests pending at the save
        with sess.snapshot() as snap:
            saved = _read_all(mpcq, sess, groups)
            blob = snap.tobytes()
            first = []
            for k in range(6):
                sess.tick(None if full else v)
                first.append(_read_all(mpcq, sess, groups))
            assert not np.array_equal(first[-1]["GV_STATE"], saved["GV_STATE"])
            sess.restore(snap)
            _same_reads(_read_all(mpcq, sess, groups), saved, "restored")
            for k in range(6):
                sess.tick(None if full else v)
                _same_reads(_read_all(mpcq, sess, groups), first[k], ("again", k))
        # the blob round trip
        version, = struct.unpack_from("<I", blob, 8)
        n_gaits, = struct.unpack_from("<i", blob, 136)
        assert version == 4 and n_gaits == 3
        with sess.snapshot_from(blob) as snap2:
            sess.restore(snap2)
            _same_reads(_read_all(mpcq, sess, groups), saved, "from the blob")
        # fork: robots 1 and 3 become copies of robot 0, the others stay
        for k in range(3):
            sess.tick(None if full else v)
        before = _read_all(mpcq, sess, groups)
        sess.fork([-1, 0, -1, 0, -1])
        after = _read_all(mpcq, sess, groups)
        _same_reads(after, before, "fork: copies", rows_a=[1, 3], rows_b=[0, 0])
        _same_reads(after, before, "fork: the others", rows_a=[0, 2, 4], rows_b=[0, 2, 4])
        assert np.array_equal(after["GV_STATE"][[1, 3]], before["GV_STATE"][[0, 0]])


def test_i_blob_without_the_group_and_the_refusals(mpcq, eng):
    B = 3
    g0 = _mixed(16, B)
    with mpcq.Session(eng, B, gait0=g0) as plain, mpcq.Session(eng, B, gait0=g0) as sess, \
            mpcq.Session(eng, B, gait0=g0) as two:
        sess.enable_gait(GC.LIB[:3])
        two.enable_gait(GC.LIB[:2])
        with plain.snapshot() as sp, sess.snapshot() as sg:
            bp, bg = sp.tobytes(), sg.tobytes()
            # a session without the group: the version-1 blob with its 128-byte header; with it,
            # the same arrays behind a 144-byte header, then the rows
            assert struct.unpack_from("<I", bp, 8)[0] == 1 and struct.unpack_from("<I", bg, 8)[0] == 4
            assert len(bg) == len(bp) + 16 + B * 16
            assert bg[144:144 + len(bp) - 128] == bp[128:]
            assert np.array_equal(np.frombuffer(bg[-B * 16:], np.int32).reshape(B, 4), GM.new_state(B))
            assert struct.unpack_from("<qq", bp, 88)[0] == len(bp) and struct.unpack_from("<q", bg, 88)[0] == len(bg)
            assert struct.unpack_from("<qii", bg, 128) == (B * 16, 3, 0)
            # the two refusals
            with pytest.raises(mpcq.MpcqError) as e:
                plain.restore(sg)
            assert "gait arrays exist on one side only" in str(e.value)
            with pytest.raises(mpcq.MpcqError) as e:
                sess.restore(sp)
            assert "gait arrays exist on one side only" in str(e.value)
            with pytest.raises(mpcq.MpcqError) as e:
                two.restore(sg)
            assert "gait library sizes differ" in str(e.value)
            sess.restore(sg)
            # a truncated version-4 blob is refused before the device is touched
            with pytest.raises(mpcq.MpcqError):
                sess.snapshot_from(bg[:136])
            with pytest.raises(mpcq.MpcqError):
                sess.snapshot_from(bg[:-4])


def test_set_gait_refusals_and_device_ids(mpcq, eng):
    import torch
    B = 4
    with mpcq.Session(eng, B) as sess:
        with pytest.raises(mpcq.MpcqError) as e:  # before enable
            sess.set_gait(0)
        assert "enable_gait" in str(e.value)
        with pytest.raises(mpcq.MpcqError):
            sess.gait_state()
        sess.enable_gait(GC.LIB[:3])
        for bad in ([0, 1, 3, 0], [0, -2, 0, 0]):
            with pytest.raises(mpcq.MpcqError) as e:
                sess.set_gait(bad)
            assert f"ids[{1 if bad[1] < 0 else 2}]" in str(e.value)
        assert np.array_equal(sess.gait_state(), GM.new_state(B))
        # a device array is not validated: the kernel's defensive read covers it
        ids = torch.tensor([1, 99, -5, 2], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sess.set_gait_device(ids.data_ptr(), asynchronous=False)
        st = sess.gait_state()
        assert st[:, 0].tolist() == [1, 99, -5, 2] and np.array_equal(st[:, 1:], GM.new_state(B)[:, 1:])
        sess.tick(np.tile(V_REF, (B, 1)))
        st = sess.gait_state()
        assert st[:, 0].tolist() == [1, -1, -1, 2] and st[:, 1].tolist() == [1, -1, -1, 2]
        # a refused re-enable leaves library and parameters in force
        with pytest.raises(mpcq.MpcqError):
            sess.enable_gait(GC.LIB[:3], align=2)
        sess.disable_gait()
        with pytest.raises(mpcq.MpcqError):
            sess.set_gait(0)
        sess.tick(np.tile(V_REF, (B, 1)))
        assert np.array_equal(sess.gait_state(), st)  # the planner's own roll again; the rows stay
