"""GPU: the estimate kernel (mpcq_estimator.hip) against the host model (tests/estimator_model.py),
alone and inside sessions.  The integer words and every P entry are bit-equal (no sin / cos enters
them); means and estimates agree within 1e-12, tests/test_gpu_plant.py's bound for the same
formulas (there measured at 4.4e-15).  Measured here on an MI355X: at most 5.6e-17 for the kernel
alone, 0.0 in the exact-recovery session; each test prints the greatest difference it met."""
import struct

import numpy as np
import pytest

import estimator_model as EM
import plant_model as PM
from monitor_model import same

pytestmark = pytest.mark.gpu

N = 16
TOL = 1e-12
SIGMA = np.array([1e-3] * 6 + [1e-2] * 6)
V_REF = [0.3, 0.0, 0.0, 0.0, 0.0, 0.1]
GUARD = 256  # poisoned bytes behind every array the kernel writes
SV = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_L_FEET", "SV_Q_W", "SV_COST",
      "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_ROT_FLAG", "SV_H_ROT", "SV_X_ROBOT", "SV_FIRST")
SCEN = dict(seed=5, v_lo=[0.2, -0.1, -0.2], v_hi=[0.6, 0.1, 0.2], cmd_start=1, cmd_ramp=3, cmd_period=0, pushes=0,
            robots=3, mass_scale_lo=0.9, mass_scale_hi=1.2, mu_lo=0.6, mu_hi=1.0)
CHANNEL = dict(seed=21, delay=3, latency=2, hold_prob=0.2, sigma=list(SIGMA), f_sigma=[0.2, 0.2, 0.4], f_gain=0.1)
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
    """Filter rows: the integer words and P bit for bit, the means and the ring's records
    (copies of the inputs) as the model's."""
    c = slice(EM.CLOCK, EM.CLOCK + 2)
    assert np.array_equal(got[:, c].view(np.int32), want[:, c].view(np.int32)), (ctx, "clock")
    assert same(got[:, EM.P_OFF:EM.P_OFF + 18], want[:, EM.P_OFF:EM.P_OFF + 18]), (ctx, "P")
    assert same(got[:, EM.PREV:EM.PREV + 12], want[:, EM.PREV:EM.PREV + 12]), (ctx, "prev_obs")
    assert same(got[:, EM.RING:], want[:, EM.RING:]), (ctx, "ring")
    _close(got[:, EM.POST:EM.POST + 12], want[:, EM.POST:EM.POST + 12], (ctx, "post"), key)


# ------------------------------------------------------------------------------- the kernel alone
T = 24


def _case(B, lag, f_lag, seed):
    """24 ticks of a synthetic loop with swing feet, noise, first masks at ticks 7 and 15, failed
    ticks at 12, a NaN row and a repeated row, and a per-robot table."""
    rng = np.random.default_rng(seed)
    table_args = dict(mass=rng.uniform(2.2, 2.9, B), gI=PM.GI * rng.uniform(0.8, 1.3, (B, 1, 1)))
    f, feet = EM.trot(T, B=B, seed=seed)
    consts = PM.constants(B, mass=table_args["mass"], gI=table_args["gI"])
    truth = EM.rollout(EM.start(B, seed), f, feet, f_lag=f_lag, consts=consts)
    obs = EM.delayed(truth, lag) + SIGMA * rng.standard_normal((T, B, 12))
    r = min(2, B - 1)
    obs[5, r, 3:6] = np.nan
    obs[10, B - 1] = obs[9, B - 1]
    first = np.zeros((T, B), np.int32)
    first[7] = rng.random(B) < 0.4
    first[15] = rng.random(B) < 0.4
    first[7, 0] = 1
    failed = np.zeros((T, B), np.int32)
    failed[12] = rng.random(B) < 0.3
    failed[12, B - 1] = 1
    return dict(f=f, feet=feet, obs=obs, first=first, failed=failed, consts=consts, table_args=table_args)


class _Guarded:
    """row and est, each with a poisoned guard behind it: numpy for host pointers, a torch buffer
    on the device for device pointers."""

    def __init__(self, B, device):
        self.device, self.buf = device, {}
        self.shape = {"row": (B, EM.ROW), "est": (B, 12)}
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


def _launch(mpcq, eng, p, g, B, obs, f_prev, feet_prev, first, all_first, failed, table):
    import ctypes as C
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
    eng._call("mpcq_estimator_step_batch", eng._h, C.byref(p), B, inp(first, np.int32), int(all_first), inp(obs),
              inp(f_prev), inp(feet_prev), inp(failed, np.int32), inp(table), C.c_void_p(g.ptr("row")),
              C.c_void_p(g.ptr("est")), flags)


@pytest.mark.parametrize("lags", [(0, 0), (1, 0), (3, 1), (8, 4)], ids=lambda d: f"lag{d[0]}f{d[1]}")
@pytest.mark.parametrize("B", [1, 3, 4, 5, 63, 64, 65, 130])
def test_kernel_alone_vs_model(mpcq, eng, B, lags):
    lag, f_lag = lags
    c = _case(B, lag, f_lag, 100 + B)
    table = mpcq.robots(B, **c["table_args"])
    kw = dict(lag=lag, f_lag=f_lag, r=list(SIGMA ** 2))
    p, m = mpcq.default_estimator_params(**kw), EM.params(**kw)
    for device in (False, True):
        rows = EM.new_rows(B)
        g = _Guarded(B, device)
        inits = 0
        for t in range(T):
            ctx = (B, lags, device, t)
            fp = c["f"][t - 1] if t else np.full((B, 12), np.nan)  # (a robot that initialises reads neither)
            ft = c["feet"][t - 1] if t else np.full((B, 3, 4), np.nan)
            want = EM.step(m, rows, c["obs"][t], fp, ft, first=c["first"][t], all_first=t == 0, failed=c["failed"][t],
                           consts=c["consts"], dt=eng.params.dt, gravity=eng.params.gravity)
            _launch(mpcq, eng, p, g, B, c["obs"][t], fp, ft, c["first"][t], t == 0, c["failed"][t], table)
            _close(g.get("est"), want, ctx, "alone")
            _rows_match(g.get("row"), rows, ctx, "alone")
            assert g.guards_intact(), ctx
            inits += int((EM.clock(rows)[:, 2] == 1).sum())
        assert inits >= B + 2  # tick 0, robot 0's first flag at tick 7, the last robot's failed tick 12
    print("kernel alone: max |device - model| =", MEASURED["alone"])


def test_a_robot_in_a_batch_gets_the_bits_it_gets_alone(mpcq, eng):
    B, lag, f_lag = 5, 3, 1
    c = _case(B, lag, f_lag, 9)
    table = mpcq.robots(B, **c["table_args"])
    est_k = mpcq.Estimator(eng, mpcq.default_estimator_params(lag=lag, f_lag=f_lag, r=list(SIGMA ** 2)))
    rows = mpcq.estimator.new_rows(B)
    alone = [mpcq.estimator.new_rows(1) for _ in range(B)]
    for t in range(T):
        fp = c["f"][t - 1] if t else np.zeros((B, 12))
        ft = c["feet"][t - 1] if t else np.zeros((B, 3, 4))
        est, rows = est_k.step(c["obs"][t], fp, ft, rows, first=c["first"][t], all_first=t == 0,
                               failed_prev=c["failed"][t], robots=table)
        for b in range(B):
            e1, alone[b] = est_k.step(c["obs"][t, b:b + 1], fp[b:b + 1], ft[b:b + 1], alone[b],
                                      first=c["first"][t, b:b + 1], all_first=t == 0,
                                      failed_prev=c["failed"][t, b:b + 1], robots=table[b:b + 1])
            assert same(e1[0], est[b]) and same(alone[b][0], rows[b]), (t, b)


def test_estimator_class_on_device_arrays(mpcq, eng):
    import torch
    B = 6
    c = _case(B, 2, 1, 4)
    est_k = mpcq.Estimator(eng, mpcq.default_estimator_params(lag=2, f_lag=1))
    rows = None
    d_row = torch.zeros(B * EM.ROW, dtype=torch.float64, device="cuda")
    d_est = torch.zeros(B * 12, dtype=torch.float64, device="cuda")
    for t in range(6):
        fp = c["f"][t - 1] if t else np.zeros((B, 12))
        ft = c["feet"][t - 1] if t else np.zeros((B, 3, 4))
        est, rows = est_k.step(c["obs"][t], fp, ft, rows, all_first=t == 0)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (c["obs"][t], fp, ft)]
        torch.cuda.synchronize()
        est_k.step_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_row.data_ptr(), d_est.data_ptr(),
                          all_first=t == 0, asynchronous=False)
        assert same(d_est.cpu().numpy().reshape(B, 12), est) and same(d_row.cpu().numpy().reshape(B, EM.ROW), rows), t


# ------------------------------------------------------------------------------- sessions
SB, TICKS = 9, 30


def _gaits(B):
    from mpcq import synth
    return np.stack([synth.gait_table(("trot", "bound")[b % 2], N) for b in range(B)])


def _open(mpcq, eng, B, estimator=None, channel=None, plant=None, monitor=None, scenario=None, swing=False,
          tables=False):
    sess = mpcq.Session(eng, B, gait0=_gaits(B))
    if swing:
        sess.enable_swing()
    if plant is not None:
        sess.enable_plant(mpcq.default_plant_params(dt=eng.params.dt, **plant))
    if tables:  # both tables in force: with everything else, every array a snapshot can hold
        rng = np.random.default_rng(8)
        sess.set_robots(mpcq.robots(B, mass=rng.uniform(2.4, 2.6, B)))
        sess.set_plant_robots(mpcq.robots(B, mass=rng.uniform(2.2, 2.9, B), mu=rng.uniform(0.6, 1.0, B)))
    if monitor:
        sess.enable_monitor(**monitor)
    if scenario:
        sess.enable_scenario(**scenario)
    if channel is not None:
        sess.enable_channel(**channel)
    if estimator is not None:
        sess.enable_estimator(**estimator)
    return sess


def _feet(fsteps):
    B = fsteps.shape[0]
    return np.ascontiguousarray(fsteps[:, 0, 1:].reshape(B, 4, 3).transpose(0, 2, 1))


def _failed(mpcq, status):
    return ~np.isin(status, (mpcq.STATUS_SOLVED, mpcq.STATUS_SOLVED_INACCURATE, mpcq.STATUS_MAX_ITER_REACHED))


def test_session_recovers_the_truth_exactly(mpcq, eng):
    """The plant is the model, the channel delays the state by 3 ticks and the forces by 1 and adds
    nothing: the estimate is the truth the plant holds, while the raw observation is not."""
    with _open(mpcq, eng, SB, estimator=dict(lag=3, f_lag=1), channel=dict(delay=3, latency=1),
               plant=dict(integrator=mpcq.PLANT_MODEL, clamp=0)) as s:
        worst_obs = np.inf
        for k in range(TICKS):
            truth = s.read(mpcq.SV_STATE)
            s.tick(V_REF)
            est, obs = s.estimator_read(mpcq.EV_EST), s.channel_read(mpcq.HV_OBS)
            assert (s.read(mpcq.SV_STATUS) == mpcq.STATUS_SOLVED).all(), k
            _close(est, truth, k, "session")
            assert same(np.ascontiguousarray(s.read(mpcq.SV_XREF)[:, :, 0]), est), k
            if k >= 4:
                off = np.abs(obs - truth).max(axis=1)
                worst_obs = min(worst_obs, off.min())
                assert (off > 1e-6).all(), (k, off)
        print("exact session: max |EV_EST - truth| =", MEASURED["session"], " least |HV_OBS - truth| =", worst_obs)
        ck = mpcq.estimator.unpack(s.estimator_read(mpcq.EV_ROW))
        assert (ck["valid"] == 1).all() and (ck["tau_next"] == TICKS).all() and (ck["s"] == TICKS - 1 - 3).all()


def test_noisy_session_vs_model(mpcq, eng):
    ch = dict(seed=3, delay=3, latency=1, sigma=list(SIGMA), hold_prob=0.15)
    kw = dict(lag=3, f_lag=1, r=list(SIGMA ** 2))
    m = EM.params(**kw)
    table = mpcq.robots(SB, mass=np.linspace(2.3, 2.7, SB))
    consts = PM.from_table(table)
    with _open(mpcq, eng, SB, estimator=kw, channel=ch, plant={}) as s:
        s.set_robots(table)
        missing = 0
        for k in range(TICKS):
            rows = s.estimator_read(mpcq.EV_ROW)
            f_prev, feet_prev = s.read(mpcq.SV_F0), _feet(s.read(mpcq.SV_FSTEPS))
            failed = _failed(mpcq, s.read(mpcq.SV_STATUS))
            truth = s.read(mpcq.SV_STATE)
            s.tick(V_REF)
            assert (s.read(mpcq.SV_STATUS) == mpcq.STATUS_SOLVED).all(), k
            obs = s.channel_read(mpcq.HV_OBS)
            missing += int((obs == rows[:, EM.PREV:EM.PREV + 12]).all(axis=1).sum())
            want = EM.step(m, rows, obs, f_prev, feet_prev, all_first=k == 0, failed=failed, consts=consts,
                           dt=eng.params.dt, gravity=eng.params.gravity)
            est = s.estimator_read(mpcq.EV_EST)
            _close(est, want, k, "session")
            _rows_match(s.estimator_read(mpcq.EV_ROW), rows, k, "session")
            assert same(np.ascontiguousarray(s.read(mpcq.SV_XREF)[:, :, 0]), est), k
            assert not same(est, obs) or k == 0
            assert not same(truth, obs) or k == 0
        assert missing > 0  # held frames were met


def test_enable_then_disable_changes_nothing(mpcq, eng):
    with _open(mpcq, eng, SB, plant={}) as a, _open(mpcq, eng, SB, plant={}, estimator={}) as b:
        b.disable_estimator()
        for k in range(6):
            a.tick(V_REF)
            b.tick(V_REF)
            for n in SV:
                assert same(a.read(getattr(mpcq, n)), b.read(getattr(mpcq, n))), (k, n)
        assert not b.estimator_read(mpcq.EV_ROW).any()  # never launched
        with pytest.raises(mpcq.MpcqError, match="estimator"):
            a.estimator_read(mpcq.EV_EST)


def test_estimator_without_channel_or_plant_leaves_a_solvable_loop(mpcq, eng):
    with _open(mpcq, eng, SB, estimator=dict(lag=0, f_lag=0)) as s:
        for k in range(TICKS):
            s.tick(V_REF)
            assert (s.read(mpcq.SV_STATUS) == mpcq.STATUS_SOLVED).all(), k
            est = s.estimator_read(mpcq.EV_EST)
            assert same(np.ascontiguousarray(s.read(mpcq.SV_XREF)[:, :, 0]), est), k
            assert np.isfinite(est).all(), k
        assert (mpcq.estimator.unpack(s.estimator_read(mpcq.EV_ROW))["tau_next"] == TICKS).all()


def test_reset_and_auto_reset_reinitialise_those_robots_only(mpcq, eng):
    kw = dict(estimator=dict(lag=2, f_lag=1), channel=dict(delay=2, latency=1, sigma=list(SIGMA), seed=4), plant={})
    mask = (np.arange(SB) % 3 == 0).astype(np.int32)
    keep = mask == 0
    with _open(mpcq, eng, SB, **kw) as a, _open(mpcq, eng, SB, **kw) as b:
        for k in range(10):
            if k == 5:
                a.reset(mask)
            a.tick(V_REF)
            b.tick(V_REF)
            ra, rb = a.estimator_read(mpcq.EV_ROW), b.estimator_read(mpcq.EV_ROW)
            assert same(ra[keep], rb[keep]), k
            assert same(a.estimator_read(mpcq.EV_EST)[keep], b.estimator_read(mpcq.EV_EST)[keep]), k
            tau = mpcq.estimator.unpack(ra)["tau_next"]
            assert tau.tolist() == [k + 1 - 5 if (m and k >= 5) else k + 1 for m in mask], k
            if k == 5:  # re-initialised: the estimate is the observation
                assert same(a.estimator_read(mpcq.EV_EST)[~keep], a.channel_read(mpcq.HV_OBS)[~keep])
    # auto-reset: episodes of 6 ticks, a third of the robots restarted by hand at tick 3, so the
    # two groups' episodes end at different ticks; a pending reset initialises the filter
    with _open(mpcq, eng, SB, monitor=dict(max_ticks=6, auto_reset=1), **kw) as s:
        want = np.zeros(SB, np.int64)
        ended = 0
        for k in range(14):
            if k == 3:
                s.reset(mask)
            first = np.ones(SB, np.int32) if k == 0 else s.read(mpcq.SV_FIRST)
            s.tick(V_REF)
            want = np.where(first != 0, 1, want + 1)
            tau = mpcq.estimator.unpack(s.estimator_read(mpcq.EV_ROW))["tau_next"]
            assert np.array_equal(tau, want), k
            done = s.monitor_read(mpcq.MV_DONE) != 0
            ended += int(done.sum())
            assert not done.all()
        assert ended >= SB


# ------------------------------------------------------------------------------- snapshots
SNAP_B = 17
EVERYTHING = dict(plant={}, monitor=dict(max_ticks=5, auto_reset=1), scenario=SCEN, swing=True, tables=True,
                  channel=CHANNEL)
EST = dict(lag=3, f_lag=2, r=list(SIGMA ** 2))


def _ticks(mpcq, s, n):
    out = []
    for _ in range(n):
        s.tick(None)
        out.append({"EV_ROW": s.estimator_read(mpcq.EV_ROW), "EV_EST": s.estimator_read(mpcq.EV_EST),
                    "SV_F0": s.read(mpcq.SV_F0), "SV_STATE": s.read(mpcq.SV_STATE)})
    return out


def _same_ticks(got, want, ctx):
    for k, (g, w) in enumerate(zip(got, want)):
        for n in w:
            assert same(g[n], w[n]), (ctx, k, n)


def test_snapshot_save_restore_and_blob(mpcq, eng):
    """With every group enabled the snapshot lists 49 arrays and gathers 48."""
    with _open(mpcq, eng, SNAP_B, estimator=EST, **EVERYTHING) as s:
        _ticks(mpcq, s, 6)
        snap = s.snapshot()
        row = s.estimator_read(mpcq.EV_ROW)
        want = _ticks(mpcq, s, 5)
        s.restore(snap)
        assert same(s.estimator_read(mpcq.EV_ROW), row)
        assert same(s.estimator_read(mpcq.EV_EST), want[-1]["EV_EST"])  # derived: the last tick's until the next
        _same_ticks(_ticks(mpcq, s, 5), want, "restored")
        blob = snap.tobytes()
        version, = struct.unpack_from("<I", blob, 8)
        flags, = struct.unpack_from("<I", blob, 28)
        part, = struct.unpack_from("<q", blob, 120)
        assert version == 3 and flags & 512 and flags & 256 and part == SNAP_B * EM.ROW * 8
        assert np.array_equal(np.frombuffer(blob[-part:], np.float64).reshape(SNAP_B, EM.ROW).view(np.int64), row.view(np.int64))
        with _open(mpcq, eng, SNAP_B, estimator=EST, **EVERYTHING) as f:
            f.restore(f.snapshot_from(blob))
            _same_ticks(_ticks(mpcq, f, 5), want, "imported")
        # a session without the estimator's arrays: refused, naming them
        with _open(mpcq, eng, SNAP_B, **EVERYTHING) as q:
            with pytest.raises(mpcq.MpcqError, match="estimator"):
                q.restore(snap)
            with pytest.raises(mpcq.MpcqError, match="estimator"):
                q.restore(q.snapshot_from(blob))
            # and its own blob is the format of before: version 2, nothing at the new offset or bit
            for _ in range(2):
                q.tick(None)
            with q.snapshot() as snap2:
                blob2 = snap2.tobytes()
            assert struct.unpack_from("<I", blob2, 8) == (2,) and not struct.unpack_from("<I", blob2, 28)[0] >> 9
            assert blob2[120:128] == bytes(8)
            parts = struct.unpack_from("<7q", blob2, 32) + struct.unpack_from("<q", blob2, 104)
            assert len(blob2) == 128 + sum(parts) == struct.unpack_from("<q", blob2, 88)[0]
        snap.close()
    with _open(mpcq, eng, SNAP_B, plant={}) as p:  # no channel either: version 1
        p.tick(V_REF)
        with p.snapshot() as snap1:
            blob1 = snap1.tobytes()
        assert struct.unpack_from("<I", blob1, 8) == (1,) and blob1[104:128] == bytes(24)


def test_restore_under_another_lag_reinitialises(mpcq, eng):
    kw = dict(channel=dict(delay=3, latency=1, sigma=list(SIGMA), seed=6), plant={})
    with _open(mpcq, eng, SB, estimator=dict(lag=3, f_lag=1), **kw) as a, \
            _open(mpcq, eng, SB, estimator=dict(lag=5, f_lag=1), **kw) as o:
        for _ in range(8):
            a.tick(V_REF)
        o.tick(V_REF)
        with a.snapshot() as snap:
            row = a.estimator_read(mpcq.EV_ROW)
            o.restore(snap)  # legal: the row is self-describing
            assert same(o.estimator_read(mpcq.EV_ROW), row)
            o.tick(V_REF, k=8)
            a.tick(V_REF)
        ck = mpcq.estimator.unpack(o.estimator_read(mpcq.EV_ROW))
        assert (ck["tau_next"] == 1).all() and (ck["s"] == 0).all() and (ck["valid"] == 1).all()
        assert same(o.estimator_read(mpcq.EV_EST), o.channel_read(mpcq.HV_OBS))
        assert (mpcq.estimator.unpack(a.estimator_read(mpcq.EV_ROW))["tau_next"] == 9).all()


def test_fork_inherits_the_row(mpcq, eng):
    r = 5
    with _open(mpcq, eng, SNAP_B, estimator=EST, **EVERYTHING) as a:
        _ticks(mpcq, a, 6)
        row = a.estimator_read(mpcq.EV_ROW)
        a.fork(r)
        assert same(a.estimator_read(mpcq.EV_ROW), np.repeat(row[r:r + 1], SNAP_B, axis=0))
        a.tick(None)
        ck = mpcq.estimator.unpack(a.estimator_read(mpcq.EV_ROW))
        assert (ck["valid"] == 1).all() and (ck["tau_next"] == ck["tau_next"][0]).all()
