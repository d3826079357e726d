"""GPU: what mpcq_session_create leaves, against literals; and that the optional stages of a
tick (swing, plant, monitor, a robots table) do not disturb each other.

mpcq_session_create writes its state with the reset kernel, so "a reset is what create leaves"
(tests/test_gpu_session_reset.py) compares that kernel with itself: the first test states the
creation state independently, in numpy.  Every comparison here is bit equality."""
import ctypes as C

import numpy as np
import pytest

import monitor_model as MM
import plant_model as PM

pytestmark = pytest.mark.gpu

B0 = 3
SHOULDERS = np.array([[0.21, 0.18, -0.17, -0.2], [0.14, -0.16, 0.15, -0.13]])
H_REF, RHO = 0.23, 0.17
ZERO = ("SV_FIRST", "SV_STATUS", "SV_ITERS", "SV_ROT_FLAG", "SV_X", "SV_Y", "SV_F0", "SV_X_ROBOT", "SV_COST", "SV_XREF")
SV = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_L_FEET", "SV_Q_W", "SV_COST",
      "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_ROT_FLAG", "SV_H_ROT", "SV_X_ROBOT", "SV_FIRST")
SWING = ("SV_SWING_REF", "SV_SWING_STATE", "SV_FRAME")
PV = ("PV_STATE_END", "PV_F_EFF", "PV_WRENCH")
MV = ("MV_DONE", "MV_EP", "MV_EP_TICKS", "MV_EPISODES", "MV_LAST", "MV_TOTALS")


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _walking_trot(N):
    """create_walking_trot (FootstepPlanner.py:193-214) for T_gait / dt = 16."""
    g = np.zeros((20, 5))
    masks = ((1, 1, 1, 1), (1, 0, 0, 1), (1, 1, 1, 1), (0, 1, 1, 0))
    for i in range(N // 16):
        for r in range(4):
            g[4 * i + r] = ((1, 7, 1, 7)[r],) + masks[r]
    return g


@pytest.mark.parametrize("N", [16, 32])
@pytest.mark.parametrize("own_gait", [False, True])
def test_session_create_state(mpcq, N, own_gait):
    from mpcq import synth
    B = B0
    gait0 = np.stack([synth.gait_table(("bound", "pace", "trot")[b], N) for b in range(B)]) if own_gait else None
    pp = mpcq._lib.default_planner_params(h_ref=H_REF, shoulders=(C.c_double * 8)(*SHOULDERS.ravel()))
    with mpcq.Engine(N, rho=RHO) as eng, mpcq.Session(eng, B, gait0=gait0, planner_params=pp) as s:
        rd = lambda n: s.read(getattr(mpcq, n))  # noqa: E731
        assert np.array_equal(rd("SV_Q_W"), np.tile([0.0, 0.0, 0.2027682, 0.0, 0.0, 0.0], (B, 1)))
        state = np.zeros((B, 12))
        state[:, 2] = H_REF
        assert np.array_equal(rd("SV_STATE"), state)
        assert np.array_equal(rd("SV_L_FEET"), np.tile(np.vstack([SHOULDERS, np.zeros((1, 4))]), (B, 1, 1)))
        assert np.array_equal(rd("SV_H_ROT"), np.full(B, 0.20))
        assert np.array_equal(rd("SV_RHO"), np.full(B, RHO))
        fs = rd("SV_FSTEPS")
        assert fs.shape == (B, 20, 13) and np.isnan(fs).all()
        assert np.array_equal(rd("SV_ORDER"), np.arange(B, dtype=np.int32))
        for n in ZERO:
            a = rd(n)
            assert a.size > 0 and MM.same(a, np.zeros_like(a)), n
        assert np.array_equal(rd("SV_GAIT"), gait0 if own_gait else np.tile(_walking_trot(N), (B, 1, 1)))
        # the opt-in groups: zero, but for the running episode's minimum height
        s.enable_swing()
        s.enable_plant()
        s.enable_monitor()
        for n in SWING:
            assert rd(n).size > 0 and not rd(n).any(), n
        for n in PV:
            assert not s.plant_read(getattr(mpcq, n)).any(), n
        ep = s.monitor_read(mpcq.MV_EP)
        assert np.array_equal(ep[:, 4], np.full(B, np.inf)) and not np.delete(ep, 4, axis=1).any()
        for n in MV:
            if n != "MV_EP":
                assert not s.monitor_read(getattr(mpcq, n)).any(), n


def test_session_create_state_needs_a_table(mpcq):
    """No walking-trot table exists at N = 12 (T_gait / dt = 16 does not divide it): E_INVALID,
    and the engine goes on."""
    from mpcq import synth
    with mpcq.Engine(12) as eng:
        with pytest.raises(mpcq.MpcqError) as err:
            mpcq.Session(eng, 1)
        assert err.value.code == mpcq._lib.E_INVALID
        with mpcq.Session(eng, 2, gait0=synth.gait_table("trot", 12)) as s:
            s.tick(np.array([0.2, 0.0, 0.0, 0.0, 0.0, 0.0]))
            assert (s.read(mpcq.SV_STATUS) == mpcq.STATUS_SOLVED).all()


# ------------------------------------------------------------------------------- composition
N, B, T = 16, 5, 6
WRENCH = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [3.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, -2.0, 0.0, 0.0, 0.0, 0.0],
                   [0.0, 0.0, -4.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.2]])


def _inputs():
    from mpcq import synth
    gaits = np.stack([synth.gait_table(("trot", "bound", "pace")[b % 3], N) for b in range(B)])
    rng = np.random.default_rng(5)
    v_ref = np.zeros((T, B, 6))
    v_ref[:, :, 0] = rng.uniform(-0.1, 0.4, (T, B))
    v_ref[:, :, 1] = rng.uniform(-0.1, 0.1, (T, B))
    v_ref[:, :, 5] = rng.uniform(-0.3, 0.3, (T, B))
    return gaits, v_ref


def _oracle_loop(gaits, v_ref):
    """The oracle's closed loop with the plant's host model in place of the prediction: every
    tick's status and the monitor's done bits (default thresholds, no time limit)."""
    from oracle import oracle as O
    ors = [O.Session(N, gaits[b]) for b in range(B)]
    status, done = np.zeros((T, B), np.int32), np.zeros((T, B), np.int32)
    for k in range(T):
        q_prev = np.stack([o.q_w for o in ors])
        read = np.stack([o.state for o in ors])
        for b, o in enumerate(ors):
            status[k, b] = o.tick(k, v_ref[k, b])
        r = PM.session_tick(read, np.stack([o.planner.fsteps for o in ors]), np.stack([o.planner.gait for o in ors]),
                            np.stack([o.f0 for o in ors]), q_prev, WRENCH)
        for b, o in enumerate(ors):
            o.q_w, o.state, o.l_feet = r["q_w"][b], r["state"][b], r["l_feet"][b]
        done[k] = MM.done_bits(r["q_w"], status[k], np.full(B, k + 1), **MM.DEFAULTS)
    return status, done


def _run(mpcq, eng, gaits, v_ref, swing=False, monitor=False, table=False):
    out = []
    with mpcq.Session(eng, B, gait0=gaits) as s:
        if swing:
            s.enable_swing()
        s.enable_plant()
        s.set_wrench(WRENCH)
        if monitor:
            s.enable_monitor(auto_reset=0)
        if table:
            s.set_robots(mpcq.robots(B, params=eng.params))
        for k in range(T):
            s.tick(v_ref[k])
            snap = {n: s.read(getattr(mpcq, n)) for n in SV + (SWING if swing else ())}
            snap.update({n: s.plant_read(getattr(mpcq, n)) for n in PV})
            if monitor:
                snap.update({n: s.monitor_read(getattr(mpcq, n)) for n in MV})
            out.append(snap)
    return out


def test_session_options_compose(mpcq):
    """Swing, plant, monitor and a robots table together leave in each group what the sessions
    with fewer options leave: no stage of the tick disturbs another.  (The table holds the
    engine's own constants, so the sessions without one are its reference too.)  The inputs are
    such that, on the CPU, no robot fails and no episode ends in these ticks; the session must
    agree, or equal arrays would say little."""
    gaits, v_ref = _inputs()
    status, done = _oracle_loop(gaits, v_ref)
    assert (status == mpcq.STATUS_SOLVED).all() and not done.any(), (status, done)
    with mpcq.Engine(N) as eng:
        everything = _run(mpcq, eng, gaits, v_ref, swing=True, monitor=True, table=True)
        swung = _run(mpcq, eng, gaits, v_ref, swing=True)
        plant = _run(mpcq, eng, gaits, v_ref)
        monitored = _run(mpcq, eng, gaits, v_ref, monitor=True)
    for k in range(T):
        e = everything[k]
        assert (e["SV_STATUS"] == mpcq.STATUS_SOLVED).all() and not e["MV_DONE"].any() and not e["MV_EPISODES"].any(), k
        assert int(e["MV_TOTALS"][0]) == (k + 1) * B and not e["MV_TOTALS"][1:].any(), k
        for n in SWING:
            assert MM.same(e[n], swung[k][n]), (k, n)
        for n in SV + PV:
            assert MM.same(e[n], plant[k][n]), (k, n)
        for n in MV:
            assert MM.same(e[n], monitored[k][n]), (k, n)
    assert everything[-1]["SV_SWING_REF"].any() and everything[-1]["PV_F_EFF"].any()
