"""GPU: the disturb kernel (mpcq_disturb.hip) against the host model (tests/disturb_model.py), alone
and inside sessions.  The integer words, prev and the ring are bit-equal (no sin / cos enters
them); the estimate d and the raw sample agree within 5e-11: the estimator test's 1e-12 on states
divided by dt = 0.02, because a sample divides a difference of states by dt.  Each test prints the
greatest difference it met (measured on an MI355X: 5.6e-15 at most for the kernel alone, 0.0 in
the sessions).

The sessions' closed-loop conditions are test_disturb_model.py's, on the device: under a heavier
true robot the mean |height error| over the last half of the run is at most one fifth of the same
session's without the stage, under a constant world push the mean |vx error| at most one half.
"""
import ctypes as C
import struct

import numpy as np
import pytest

import disturb_model as DM
import estimator_model as EM
import plant_model as PM
from monitor_model import same

pytestmark = pytest.mark.gpu

N = 16
TOL = 5e-11
SIGMA = np.array([1e-3] * 6 + [1e-2] * 6)
GUARD = 256  # poisoned bytes behind every array the kernel writes
SV = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_L_FEET", "SV_Q_W", "SV_COST",
      "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_ROT_FLAG", "SV_H_ROT", "SV_X_ROBOT", "SV_FIRST")
MEASURED = {"alone": 0.0, "session": 0.0}


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.fixture(scope="module")
def eng(mpcq):
    with mpcq.Engine(N) as e:
        yield e


def _close(got, want, ctx, key):
    """NaN where the model has NaN, within TOL elsewhere; the greatest difference is kept."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), ctx
    ok = ~np.isnan(want)
    d = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    MEASURED[key] = max(MEASURED[key], d)
    assert d <= TOL, (ctx, d)


def _rows_match(got, want, ctx, key):
    """The stage's rows: the integer words, prev and the ring's records bit for bit, d as the model's."""
    c = slice(DM.CLOCK, DM.CLOCK + 2)
    assert np.array_equal(got[:, c].view(np.int32), want[:, c].view(np.int32)), (ctx, "clock")
    assert same(got[:, DM.PREV:DM.PREV + 12], want[:, DM.PREV:DM.PREV + 12]), (ctx, "prev")
    assert same(got[:, DM.RING:], want[:, DM.RING:]), (ctx, "ring")
    _close(got[:, DM.D:DM.D + 6], want[:, DM.D:DM.D + 6], (ctx, "d"), key)


# ------------------------------------------------------------------------------- the kernel alone
T = 24


def _case(B, f_lag, seed):
    """24 ticks of a synthetic loop under a constant wrench with swing feet, noise, first masks at
    ticks 7 and 15, failed ticks at 12, a NaN row and a repeated row, and a per-robot table."""
    rng = np.random.default_rng(seed)
    table_args = dict(mass=rng.uniform(2.2, 2.9, B), gI=PM.GI * rng.uniform(0.8, 1.3, (B, 1, 1)))
    f, feet = EM.trot(T, B=B, seed=seed)
    consts = PM.constants(B, mass=table_args["mass"], gI=table_args["gI"])
    w = np.concatenate([rng.uniform(-4, 4, (B, 3)), rng.uniform(-0.15, 0.15, (B, 3))], axis=1)
    truth = np.zeros((T + 1, B, 12))
    truth[0] = EM.start(B, seed)
    for t in range(T):
        ft = f[t - f_lag] if t - f_lag >= 0 else np.broadcast_to(EM.F_INIT, (B, 12))
        x = truth[t].copy()
        x[:, 6:9] += 0.02 * w[:, :3] / consts[0][:, None]  # (a push on top of the model's own step)
        x[:, 9:12] += 0.02 * w[:, 3:] / 0.05
        truth[t + 1] = EM.model_step(x, feet[t], ft, consts)
    meas = truth[:T] + SIGMA * rng.standard_normal((T, B, 12))
    r = min(2, B - 1)
    meas[5, r, 3:6] = np.nan
    meas[10, B - 1] = meas[9, B - 1]
    first = np.zeros((T, B), np.int32)
    first[7] = rng.random(B) < 0.4
    first[15] = rng.random(B) < 0.4
    first[7, 0] = 1
    failed = np.zeros((T, B), np.int32)
    failed[12] = rng.random(B) < 0.3
    failed[12, B - 1] = 1
    return dict(f=f, feet=feet, meas=meas, first=first, failed=failed, consts=consts, table_args=table_args)


class _Guarded:
    """row, dist and resid, each with a poisoned guard behind it: numpy for host pointers, a torch
    buffer on the device for device pointers."""

    def __init__(self, B, device):
        self.device, self.buf = device, {}
        self.shape = {"row": (B, DM.ROW), "dist": (B, 8), "resid": (B, 6)}
        for k, shp in self.shape.items():
            raw = np.full(int(np.prod(shp)) * 8 + GUARD, 0xA5, np.uint8)
            if k == "row":
                raw[:-GUARD] = 0
            self.buf[k] = self.up(raw) if device else raw

    @staticmethod
    def up(raw):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(-1).copy()).to("cuda")
        torch.cuda.synchronize()
        return t

    def raw(self, k):
        return self.buf[k].cpu().numpy() if self.device else self.buf[k]

    def ptr(self, k):
        return self.buf[k].data_ptr() if self.device else self.buf[k].ctypes.data

    def get(self, k):
        return self.raw(k)[:-GUARD].view(np.float64).reshape(self.shape[k]).copy()

    def guards_intact(self):
        return all((self.raw(k)[-GUARD:] == 0xA5).all() for k in self.shape)


def _launch(mpcq, eng, p, g, B, meas, f_prev, feet_prev, first, all_first, failed, table):
    flags = mpcq.FLAG_DEVICE_PTRS if g.device else 0
    keep = []

    def inp(a, dt=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        if g.device:
            t = _Guarded.up(a)
            keep.append(t)
            return C.c_void_p(t.data_ptr())
        keep.append(a)
        return C.c_void_p(a.ctypes.data)
    eng._call("mpcq_disturb_step_batch", eng._h, C.byref(p), B, inp(first, np.int32), int(all_first), inp(meas),
              inp(f_prev), inp(feet_prev), inp(failed, np.int32), inp(table), C.c_void_p(g.ptr("row")),
              C.c_void_p(g.ptr("dist")), C.c_void_p(g.ptr("resid")), flags)


@pytest.mark.parametrize("f_lag", [0, 1, 4])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 63, 64, 65, 130])
def test_kernel_alone_vs_model(mpcq, eng, B, f_lag):
    c = _case(B, f_lag, 100 + B)
    table = mpcq.robots(B, **c["table_args"])
    kw = dict(f_lag=f_lag, alpha=[0.2, 0.3, 0.5, 0.7, 0.9, 1.0], d_max=[3.0, 3.0, 5.0, 40.0, 40.0, 0.5])
    p, m = mpcq.default_disturb_params(**kw), DM.params(**kw)
    for device in (False, True):
        rows = DM.new_rows(B)
        g = _Guarded(B, device)
        firsts = samples = clipped = 0
        for t in range(T):
            ctx = (B, f_lag, device, t)
            fp = c["f"][t - 1] if t else np.full((B, 12), np.nan)  # (a robot that runs a first tick reads neither)
            ft = c["feet"][t - 1] if t else np.full((B, 3, 4), np.nan)
            d, res = DM.step(m, rows, c["meas"][t], fp, ft, first=c["first"][t], all_first=t == 0, failed=c["failed"][t],
                             consts=c["consts"], dt=eng.params.dt, gravity=eng.params.gravity)
            _launch(mpcq, eng, p, g, B, c["meas"][t], fp, ft, c["first"][t], t == 0, c["failed"][t], table)
            dist = g.get("dist")
            _close(dist[:, :6], d, ctx, "alone")
            assert not dist[:, 6:].any(), ctx  # reserved: zero
            _close(g.get("resid"), res, ctx, "alone")
            _rows_match(g.get("row"), rows, ctx, "alone")
            assert same(dist[:, :6], g.get("row")[:, DM.D:DM.D + 6]), ctx
            assert g.guards_intact(), ctx
            firsts += int((DM.clock(rows)[:, 1] == 1).sum())
            samples += int(np.isfinite(res).all(axis=1).sum())
            clipped += int((np.abs(d) == np.array(m.d_max)).sum())
        assert firsts >= B + 1 and samples >= 15 * B and clipped > 0  # tick 0, robot 0's first flag at tick 7
    print("kernel alone: max |device - model| =", MEASURED["alone"])


def test_a_robot_in_a_batch_gets_the_bits_it_gets_alone(mpcq, eng):
    B, f_lag = 5, 1
    c = _case(B, f_lag, 9)
    table = mpcq.robots(B, **c["table_args"])
    k = mpcq.Disturb(eng, mpcq.default_disturb_params(f_lag=f_lag, alpha=0.4))
    rows = mpcq.disturb.new_rows(B)
    alone = [mpcq.disturb.new_rows(1) for _ in range(B)]
    for t in range(T):
        fp = c["f"][t - 1] if t else np.zeros((B, 12))
        ft = c["feet"][t - 1] if t else np.zeros((B, 3, 4))
        dist, res, rows = k.step(c["meas"][t], fp, ft, rows, first=c["first"][t], all_first=t == 0,
                                 failed_prev=c["failed"][t], robots=table)
        for b in range(B):
            d1, r1, alone[b] = k.step(c["meas"][t, b:b + 1], fp[b:b + 1], ft[b:b + 1], alone[b],
                                      first=c["first"][t, b:b + 1], all_first=t == 0,
                                      failed_prev=c["failed"][t, b:b + 1], robots=table[b:b + 1])
            assert d1[0].tobytes() == dist[b].tobytes() and same(r1[0], res[b]) and same(alone[b][0], rows[b]), (t, b)


def test_disturb_class_on_device_arrays(mpcq, eng):
    import torch
    B = 6
    c = _case(B, 1, 4)
    k = mpcq.Disturb(eng, mpcq.default_disturb_params(f_lag=1))
    rows = None
    d_row = torch.zeros(B * DM.ROW, dtype=torch.float64, device="cuda")
    d_dist = torch.zeros(B * 8, dtype=torch.float64, device="cuda")
    for t in range(6):
        fp = c["f"][t - 1] if t else np.zeros((B, 12))
        ft = c["feet"][t - 1] if t else np.zeros((B, 3, 4))
        dist, _, rows = k.step(c["meas"][t], fp, ft, rows, all_first=t == 0)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (c["meas"][t], fp, ft)]
        torch.cuda.synchronize()
        k.step_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_row.data_ptr(), d_dist.data_ptr(),
                      all_first=t == 0, asynchronous=False)  # (no resid array: optional)
        assert d_dist.cpu().numpy().tobytes() == dist.tobytes() and same(d_row.cpu().numpy().reshape(B, DM.ROW), rows), t


# ------------------------------------------------------------------------------- sessions
SB, TICKS = 9, 40
V_REF = [0.2, 0.0, 0.0, 0.0, 0.0, 0.0]
MODEL_PLANT = dict(integrator=0, clamp=0)  # MPCQ_PLANT_MODEL


def _gaits(B):
    from mpcq import synth
    return np.stack([synth.gait_table("trot", N) for b in range(B)])


def _open(mpcq, eng, B, disturb=None, plant=None, heavier=None, push=None, channel=None, estimator=None, monitor=None):
    sess = mpcq.Session(eng, B, gait0=_gaits(B))
    if plant is not None:
        sess.enable_plant(mpcq.default_plant_params(dt=eng.params.dt, **plant))
    if heavier is not None:
        sess.set_plant_robots(mpcq.robots(B, mass=PM.MASS * np.asarray(heavier)))
    if push is not None:
        sess.set_wrench(push)
    if monitor:
        sess.enable_monitor(**monitor)
    if channel is not None:
        sess.enable_channel(**channel)
    if estimator is not None:
        sess.enable_estimator(**estimator)
    if disturb is not None:
        sess.enable_disturb(**disturb)
    return sess


def _feet(fsteps):
    B = fsteps.shape[0]
    return np.ascontiguousarray(fsteps[:, 0, 1:].reshape(B, 4, 3).transpose(0, 2, 1))


def _failed(mpcq, status):
    return ~np.isin(status, (mpcq.STATUS_SOLVED, mpcq.STATUS_SOLVED_INACCURATE, mpcq.STATUS_MAX_ITER_REACHED))


def _tracked(mpcq, s, ticks, model=None, eng=None):
    """ticks ticks at V_REF: the states every tick's planner read; with ``model``, MPCQ_DV_DIST and
    the rows against the host model fed the session's own arrays."""
    states = []
    for k in range(ticks):
        if model is not None:
            rows = s.disturb_read(mpcq.DV_ROW)
            f_prev, feet_prev = s.read(mpcq.SV_F0), _feet(s.read(mpcq.SV_FSTEPS))
            failed = _failed(mpcq, s.read(mpcq.SV_STATUS))
        meas = s.read(mpcq.SV_STATE)  # (no channel, no estimator: what the planner is about to read)
        s.tick(V_REF)
        assert (s.read(mpcq.SV_STATUS) == mpcq.STATUS_SOLVED).all(), (k, s.read(mpcq.SV_STATUS))
        assert same(np.ascontiguousarray(s.read(mpcq.SV_XREF)[:, :, 0]), meas), k  # the stage does not change it
        states.append(meas)
        if model is not None:
            d, res = DM.step(model, rows, meas, f_prev, feet_prev, all_first=k == 0, failed=failed,
                             dt=eng.params.dt, gravity=eng.params.gravity)
            dist = s.disturb_read(mpcq.DV_DIST)
            _close(dist["a"], d, k, "session")
            assert not dist["reserved"].any()
            _close(s.disturb_read(mpcq.DV_RESID), res, k, "session")
            _rows_match(s.disturb_read(mpcq.DV_ROW), rows, k, "session")
    return np.array(states)


def test_session_payload_and_push_vs_model_and_the_conditions(mpcq, eng):
    """N = 16, B = 9, 40 ticks, the MODEL plant without clamp.  Robots 0..4 carry 1.4 x the believed
    mass, robots 5..8 are pushed by a constant world wrench of (3, -2, 0) N."""
    heavier = np.where(np.arange(SB) < 5, 1.4, 1.0)
    push = np.where((np.arange(SB) >= 5)[:, None], np.array([3.0, -2.0, 0, 0, 0, 0]), 0.0)
    kw = dict(plant=MODEL_PLANT, heavier=heavier, push=push)
    par = dict(alpha=0.3)
    with _open(mpcq, eng, SB, **kw) as plain, _open(mpcq, eng, SB, disturb=par, **kw) as comp:
        s0 = _tracked(mpcq, plain, TICKS)
        s1 = _tracked(mpcq, comp, TICKS, model=DM.params(**par), eng=eng)
        d = comp.disturb_read(mpcq.DV_DIST)["a"]
        ck = mpcq.disturb.unpack(comp.disturb_read(mpcq.DV_ROW))
        assert (ck["valid"] == 1).all() and (ck["tau_next"] == TICKS).all()
    half = TICKS // 2
    h0 = np.abs(s0[half:, :5, 2] - 0.2027682).mean()
    h1 = np.abs(s1[half:, :5, 2] - 0.2027682).mean()
    v0 = np.abs(s0[half:, 5:, 6] - V_REF[0]).mean()
    v1 = np.abs(s1[half:, 5:, 6] - V_REF[0]).mean()
    print(f"sessions: payload mean |height error| {h0:.4f} -> {h1:.4f} (1/{h0 / h1:.1f}), push mean |vx error| "
          f"{v0:.4f} -> {v1:.4f} (1/{v0 / v1:.1f}); d of robot 0 {np.round(d[0], 3).tolist()}, of robot 5 "
          f"{np.round(d[5], 3).tolist()}; max |DV - model| {MEASURED['session']:.2e}")
    assert h1 <= h0 / 5, (h0, h1)
    assert v1 <= v0 / 2, (v0, v1)
    assert np.abs(d[5:, :3] - np.array([3.0, -2.0, 0.0]) / PM.MASS).max() < 0.05  # F / m


def test_no_compensation_leaves_every_array_as_it_was(mpcq, eng):
    """compensate = 0: the stage estimates, and every SV array is bit for bit that of a session
    that never enabled it; the solve then takes the user's table where there is one."""
    kw = dict(plant=MODEL_PLANT, heavier=np.full(SB, 1.3))
    tab = mpcq.disturbances(SB, lin=[0.0, 0.0, -2.0])
    with _open(mpcq, eng, SB, **kw) as a, _open(mpcq, eng, SB, disturb=dict(compensate=0, alpha=0.5), **kw) as b:
        for k in range(8):
            if k == 4:
                a.set_disturbance(tab)
                b.set_disturbance(tab)
            a.tick(V_REF)
            b.tick(V_REF)
            for n in SV:
                assert same(a.read(getattr(mpcq, n)), b.read(getattr(mpcq, n))), (k, n)
        assert (b.disturb_read(mpcq.DV_DIST)["a"][:, 2] < -1.0).all()  # (seen, not used)
        # with compensation the estimate takes precedence over the user's table
        b.enable_disturb(compensate=1, alpha=0.5)
        a.tick(V_REF)
        b.tick(V_REF)
        assert not same(a.read(mpcq.SV_F0), b.read(mpcq.SV_F0))
        with pytest.raises(mpcq.MpcqError, match="disturb"):
            a.disturb_read(mpcq.DV_DIST)


def test_enable_then_disable_changes_nothing(mpcq, eng):
    with _open(mpcq, eng, SB, plant={}) as a, _open(mpcq, eng, SB, plant={}, disturb={}) as b:
        b.disable_disturb()
        for k in range(6):
            a.tick(V_REF)
            b.tick(V_REF)
            for n in SV:
                assert same(a.read(getattr(mpcq, n)), b.read(getattr(mpcq, n))), (k, n)
        assert not b.disturb_read(mpcq.DV_ROW).any() and not b.disturb_read(mpcq.DV_DIST)["a"].any()  # never launched
        # enabling again zeroes the rows: the first tick after it is a first tick of the stage
        b.enable_disturb(alpha=1.0)
        b.tick(V_REF)
        b.tick(V_REF)
        b.disable_disturb()
        b.tick(V_REF)
        assert b.disturb_read(mpcq.DV_ROW).any()
        b.enable_disturb(alpha=1.0)
        assert not b.disturb_read(mpcq.DV_ROW).any() and not b.disturb_read(mpcq.DV_DIST)["a"].any()
        b.tick(V_REF)
        ck = mpcq.disturb.unpack(b.disturb_read(mpcq.DV_ROW))
        assert (ck["tau_next"] == 1).all() and not ck["d"].any()
        # enabling while enabled only replaces the parameters
        b.enable_disturb(alpha=0.5)
        assert (mpcq.disturb.unpack(b.disturb_read(mpcq.DV_ROW))["tau_next"] == 1).all()


def test_works_without_plant_channel_or_estimator(mpcq, eng):
    """The virtual robot follows the solver's own prediction, which satisfies the model's dynamics
    rows to OSQP's primal tolerance eps_abs + eps_rel max(|Ax|, |z|), with |Ax|, |z| <= 2 fz_max (a
    cone row adds two force components): every sample, and so every convex combination of
    samples, is at most that over dt -- 2.6e-4 m/s^2 with the defaults (measured: 5.4e-5)."""
    p = eng.params
    bound = (p.eps_abs + p.eps_rel * 2 * p.fz_max) / p.dt
    with _open(mpcq, eng, SB, disturb=dict(alpha=0.5)) as s:
        worst = 0.0
        for k in range(12):
            s.tick(V_REF)
            assert (s.read(mpcq.SV_STATUS) == mpcq.STATUS_SOLVED).all(), k
            res = s.disturb_read(mpcq.DV_RESID)
            assert np.isfinite(res).all() == (k > 0), k
            worst = max(worst, float(np.abs(s.disturb_read(mpcq.DV_DIST)["a"]).max()))
        print(f"no plant: max |d| {worst:.2e}, bound {bound:.2e}")
        assert worst <= bound


def test_behind_channel_and_estimator(mpcq, eng):
    """enable_channel(delay=2, latency=1) + enable_estimator(lag=2, f_lag=1), the stage with
    f_lag=1: every tick solves, the estimate is finite and bounded by d_max."""
    dp = dict(f_lag=1, alpha=0.2)
    with _open(mpcq, eng, SB, plant={}, heavier=np.full(SB, 1.2), channel=dict(delay=2, latency=1, seed=4),
               estimator=dict(lag=2, f_lag=1), disturb=dp) as s:
        d_max = np.array(mpcq.default_disturb_params().d_max[:])
        for k in range(30):
            s.tick(V_REF)
            assert (s.read(mpcq.SV_STATUS) == mpcq.STATUS_SOLVED).all(), k
            d = s.disturb_read(mpcq.DV_DIST)["a"]
            assert np.isfinite(d).all() and (np.abs(d) <= d_max).all(), k
            assert same(np.ascontiguousarray(s.read(mpcq.SV_XREF)[:, :, 0]), s.estimator_read(mpcq.EV_EST)), k
        assert (d[:, 2] < -0.5).all()  # (the payload is seen through the estimator)


def test_reset_and_auto_reset_zero_those_robots_rows_only(mpcq, eng):
    kw = dict(plant=MODEL_PLANT, heavier=np.full(SB, 1.3), disturb=dict(alpha=0.5))
    mask = (np.arange(SB) % 3 == 0).astype(np.int32)
    keep = mask == 0
    with _open(mpcq, eng, SB, **kw) as a, _open(mpcq, eng, SB, **kw) as b:
        for k in range(10):
            if k == 5:
                a.reset(mask)
            a.tick(V_REF)
            b.tick(V_REF)
            ra, rb = a.disturb_read(mpcq.DV_ROW), b.disturb_read(mpcq.DV_ROW)
            assert same(ra[keep], rb[keep]), k
            assert a.disturb_read(mpcq.DV_DIST)[keep].tobytes() == b.disturb_read(mpcq.DV_DIST)[keep].tobytes(), k
            u = mpcq.disturb.unpack(ra)
            assert u["tau_next"].tolist() == [k + 1 - 5 if (m and k >= 5) else k + 1 for m in mask], k
            if k == 5:
                assert not u["d"][~keep].any() and not a.disturb_read(mpcq.DV_DIST)["a"][~keep].any()
                assert (u["d"][keep][:, 2] < -0.5).all()  # (the others keep their estimate of the payload)
    with _open(mpcq, eng, SB, monitor=dict(max_ticks=6, auto_reset=1), **kw) as s:
        want = np.zeros(SB, np.int64)
        ended = 0
        for k in range(14):
            if k == 3:
                s.reset(mask)
            first = np.ones(SB, np.int32) if k == 0 else s.read(mpcq.SV_FIRST)
            s.tick(V_REF)
            want = np.where(first != 0, 1, want + 1)
            u = mpcq.disturb.unpack(s.disturb_read(mpcq.DV_ROW))
            assert np.array_equal(u["tau_next"], want), k
            assert not u["d"][first != 0].any(), k
            done = s.monitor_read(mpcq.MV_DONE) != 0
            ended += int(done.sum())
            assert not done.all()
        assert ended >= SB


# ------------------------------------------------------------------------------- snapshots
SNAP = dict(plant=MODEL_PLANT, heavier=np.linspace(1.1, 1.4, SB), disturb=dict(alpha=0.4))


def _ticks(mpcq, s, n):
    out = []
    for _ in range(n):
        s.tick(V_REF)
        out.append({"DV_ROW": s.disturb_read(mpcq.DV_ROW), "DV_DIST": s.disturb_read(mpcq.DV_DIST)["a"].copy(),
                    "SV_F0": s.read(mpcq.SV_F0), "SV_STATE": s.read(mpcq.SV_STATE)})
    return out


def _same_ticks(got, want, ctx):
    for k, (g, w) in enumerate(zip(got, want)):
        for n in w:
            assert same(g[n], w[n]), (ctx, k, n)


def test_snapshot_save_restore_and_blob(mpcq, eng):
    with _open(mpcq, eng, SB, **SNAP) as s:
        _ticks(mpcq, s, 6)
        snap = s.snapshot()
        row = s.disturb_read(mpcq.DV_ROW)
        want = _ticks(mpcq, s, 5)
        s.restore(snap)
        assert same(s.disturb_read(mpcq.DV_ROW), row)
        assert same(s.disturb_read(mpcq.DV_DIST)["a"], want[-1]["DV_DIST"])  # derived: the last tick's until the next
        _same_ticks(_ticks(mpcq, s, 5), want, "restored")
        blob = snap.tobytes()
        version, = struct.unpack_from("<I", blob, 8)
        flags, = struct.unpack_from("<I", blob, 28)
        part, pad = struct.unpack_from("<2q", blob, 144)
        total, = struct.unpack_from("<q", blob, 88)
        assert version == 5 and flags & 2048 and not flags & 1024 and part == SB * DM.ROW * 8 and pad == 0
        assert blob[128:144] == bytes(16) and total == len(blob)  # (no gait part: its header fields zero)
        assert np.array_equal(np.frombuffer(blob[-part:], np.float64).reshape(SB, DM.ROW).view(np.int64), row.view(np.int64))
        with _open(mpcq, eng, SB, **SNAP) as f:
            f.restore(f.snapshot_from(blob))
            _same_ticks(_ticks(mpcq, f, 5), want, "imported")
            with pytest.raises(mpcq.MpcqError):  # a truncated version-5 blob is refused
                f.snapshot_from(blob[:-8])
        # a session without the stage's arrays: refused, naming them; its own blob is the format of before
        older = dict(SNAP, disturb=None)
        with _open(mpcq, eng, SB, **older) as q:
            with pytest.raises(mpcq.MpcqError, match="disturb"):
                q.restore(snap)
            with pytest.raises(mpcq.MpcqError, match="disturb"):
                q.restore(q.snapshot_from(blob))
            for _ in range(2):
                q.tick(V_REF)
            q.set_disturbance(mpcq.disturbances(SB, lin=[0.1, 0.0, -1.0]))  # (a table is not carried)
            with q.snapshot() as snap1:
                blob1 = snap1.tobytes()
            assert struct.unpack_from("<I", blob1, 8) == (1,) and not struct.unpack_from("<I", blob1, 28)[0] >> 9
            assert len(blob1) == 128 + sum(struct.unpack_from("<7q", blob1, 32))
            # an older blob, without the part, is read as before -- and refused by a session with the arrays
            q.restore(q.snapshot_from(blob1))
            with pytest.raises(mpcq.MpcqError, match="disturb"):
                s.restore(s.snapshot_from(blob1))
        snap.close()


def test_fork_inherits_the_row(mpcq, eng):
    r = 5
    with _open(mpcq, eng, SB, **SNAP) as a:
        _ticks(mpcq, a, 6)
        row = a.disturb_read(mpcq.DV_ROW)
        a.fork(r)
        assert same(a.disturb_read(mpcq.DV_ROW), np.repeat(row[r:r + 1], SB, axis=0))
        a.tick(V_REF)
        u = mpcq.disturb.unpack(a.disturb_read(mpcq.DV_ROW))
        assert (u["valid"] == 1).all() and (u["tau_next"] == 7).all()
