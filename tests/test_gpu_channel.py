"""GPU: the channel kernels (mpcq_channel.hip) against the host model (tests/channel_model.py),
alone and inside sessions, bit for bit throughout: what the planner sees is the observation, what
the plant integrates is the truth under the delayed command; a zero channel changes nothing;
resets, enables in mid-run and snapshots carry the channel's state."""
import struct

import numpy as np
import pytest

import channel_model as CM
from monitor_model import same

pytestmark = pytest.mark.gpu

N = 16
MIXED = dict(sigma=[0.0, 0.01, 0.02] * 4, bias=[0.05, 0.0, 0.1] * 4, f_sigma=[0.5, 0.0, 1.0], f_gain=0.2)
ALL_ON = dict(seed=21, delay=3, latency=2, hold_prob=0.2, sigma=[0.002, 0.002, 0.001, 0.003, 0.003, 0.003] * 2,
              bias=[0.004, 0.004, 0.002, 0.005, 0.005, 0.005] * 2, f_sigma=[0.2, 0.2, 0.4], f_gain=0.1)
HV = ("HV_CLOCK", "HV_OBS", "HV_F_CMD", "HV_DRAW", "HV_S_RING", "HV_F_RING")
KEYS = ("clock", "obs", "f_cmd", "draw", "s_ring", "f_ring")  # new_state's names, in the ids' order
SV = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_L_FEET", "SV_Q_W", "SV_COST",
      "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_ROT_FLAG", "SV_H_ROT", "SV_X_ROBOT", "SV_FIRST")
PV = ("PV_STATE_END", "PV_F_EFF", "PV_WRENCH")
MV = ("MV_DONE", "MV_EP", "MV_EP_TICKS", "MV_EPISODES", "MV_LAST", "MV_TOTALS")
SCEN = dict(seed=5, v_lo=[0.2, -0.1, -0.2], v_hi=[0.6, 0.1, 0.2], cmd_start=1, cmd_ramp=3, cmd_period=0, pushes=0,
            robots=3, mass_scale_lo=0.9, mass_scale_hi=1.2, mu_lo=0.6, mu_hi=1.0)
V_REF = [0.3, 0.0, 0.0, 0.0, 0.0, 0.1]
GUARD = 256  # poisoned bytes behind every array the kernels write


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.fixture(scope="module")
def eng(mpcq):
    with mpcq.Engine(N) as e:
        yield e


def _hv(mpcq, sess):
    return {k: sess.channel_read(getattr(mpcq, n)) for k, n in zip(KEYS, HV)}


def _hv_same(got, st, ctx, keys=KEYS):
    for k in keys:
        assert same(got[k], st[k]), (ctx, k)


# ------------------------------------------------------------------------------- the kernels alone
def _inputs(B, seed):
    """12 ticks of truths and forces with -0.0 entries and NaN in one robot, the first masks of
    ticks 4 and 9, the robots armed before tick 6."""
    rng = np.random.default_rng(seed)
    tr, f0 = rng.standard_normal((12, B, 12)), rng.standard_normal((12, B, 12)) * 10.0
    tr[rng.random(tr.shape) < 0.05] = -0.0
    f0[rng.random(f0.shape) < 0.05] = -0.0
    r = min(2, B - 1)
    tr[3:8, r, 1:7] = np.nan
    f0[5:7, r, 4:9] = np.nan
    first = {4: (rng.random(B) < 0.4).astype(np.int32), 9: (rng.random(B) < 0.4).astype(np.int32)}
    first[4][0] = 1
    armed = (rng.random(B) < 0.5).astype(np.int32)
    armed[B - 1] = 1
    return tr, f0, first, armed


class _Guarded:
    """The six arrays, each with a poisoned guard behind it: numpy for host pointers, a torch
    buffer on the device for device pointers."""

    def __init__(self, st, device):
        self.device, self.shape, self.buf = device, {}, {}
        for k in KEYS:
            a = st[k]
            raw = np.full(a.nbytes + GUARD, 0xA5, np.uint8)
            raw[:a.nbytes] = a.view(np.uint8).reshape(-1)
            self.shape[k] = (a.shape, a.dtype, a.nbytes)
            self.buf[k] = self._up(raw) if device else raw

    @staticmethod
    def _up(raw):
        import torch
        t = torch.from_numpy(raw).to("cuda")
        torch.cuda.synchronize()
        return t

    def raw(self, k):
        return self.buf[k].cpu().numpy() if self.device else self.buf[k]

    def ptr(self, k):
        return self.buf[k].data_ptr() if self.device else self.buf[k].ctypes.data

    def get(self, k):
        shape, dt, nb = self.shape[k]
        return self.raw(k)[:nb].view(dt).reshape(shape).copy()

    def put(self, k, a):
        raw = self.raw(k).copy()
        raw[:a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        if self.device:
            self.buf[k] = self._up(raw)
        else:
            self.buf[k][:] = raw

    def guards_intact(self):
        return all((self.raw(k)[self.shape[k][2]:] == 0xA5).all() for k in KEYS)


def _launch(mpcq, eng, p, g, B, truth=None, f0=None, first=None, all_first=False):
    """One stage on the guarded arrays through the C entry point, host or device pointers."""
    import ctypes as C
    flags = mpcq.FLAG_DEVICE_PTRS if g.device else 0
    keep = []

    def inp(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if g.device:
            t = _Guarded._up(a.view(np.uint8).reshape(-1).copy())
            keep.append(t)
            return C.c_void_p(t.data_ptr())
        keep.append(a)
        return C.c_void_p(a.ctypes.data)
    v = lambda k: C.c_void_p(g.ptr(k))  # noqa: E731
    if truth is not None:
        eng._call("mpcq_channel_observe_batch", eng._h, C.byref(p), B, inp(first), int(all_first), inp(truth),
                  v("clock"), v("obs"), v("draw"), v("s_ring"), v("f_ring"), flags)
    else:
        eng._call("mpcq_channel_actuate_batch", eng._h, C.byref(p), B, inp(f0), v("clock"), v("draw"), v("f_ring"),
                  v("f_cmd"), flags)


@pytest.mark.parametrize("depths", [(0, 0), (1, 1), (3, 2), (8, 4)], ids=lambda d: f"d{d[0]}l{d[1]}")
@pytest.mark.parametrize("B", [1, 3, 4, 5, 63, 64, 65, 130])
def test_kernels_alone_vs_model(mpcq, eng, B, depths):
    tr, f0, first, armed = _inputs(B, 100 + B)
    for hold in (0.0, 0.3):
        for device in (False, True):
            kw = dict(MIXED, seed=77 + B, delay=depths[0], latency=depths[1], hold_prob=hold)
            p, m = mpcq.default_channel_params(**kw), CM.params(**kw)
            st = CM.new_state(B)
            g = _Guarded(st, device)
            for t in range(12):
                ctx = (B, depths, hold, device, t)
                if t == 6:  # what a re-enable with other depths does to these robots
                    CM.arm(st, armed)
                    g.put("clock", st["clock"])
                CM.observe(m, st, tr[t], first=first.get(t), all_first=t == 0)
                _launch(mpcq, eng, p, g, B, truth=tr[t], first=first.get(t), all_first=t == 0)
                _hv_same({k: g.get(k) for k in KEYS}, st, ctx + ("observe",))
                CM.actuate(m, st, f0[t])
                _launch(mpcq, eng, p, g, B, f0=f0[t])
                _hv_same({k: g.get(k) for k in KEYS}, st, ctx + ("actuate",))
                assert g.guards_intact(), ctx
            assert st["clock"][:, 0].max() >= 2 and (st["draw"][:, 12] > 0).all()


def test_package_classes_run_the_kernels(mpcq, eng):
    """mpcq.Channel's observe / actuate on host arrays and its *_device forms."""
    import torch
    B = 9
    tr, f0, _, _ = _inputs(B, 3)
    kw = dict(MIXED, seed=4, delay=2, latency=1, hold_prob=0.3)
    ch, m = mpcq.Channel(eng, mpcq.default_channel_params(**kw)), CM.params(**kw)
    st, mst = None, CM.new_state(B)
    dev = {k: torch.from_numpy(v.copy()).to("cuda") for k, v in CM.new_state(B).items()}
    for t in range(5):
        obs, st = ch.observe(tr[t], st, all_first=t == 0)
        cmd, st = ch.actuate(f0[t], st)
        d_tr, d_f0 = torch.from_numpy(tr[t].copy()).to("cuda"), torch.from_numpy(f0[t].copy()).to("cuda")
        torch.cuda.synchronize()
        ch.observe_device(B, d_tr.data_ptr(), dev["clock"].data_ptr(), dev["obs"].data_ptr(), dev["draw"].data_ptr(),
                          dev["s_ring"].data_ptr(), dev["f_ring"].data_ptr(), all_first=t == 0)
        ch.actuate_device(B, d_f0.data_ptr(), dev["clock"].data_ptr(), dev["draw"].data_ptr(), dev["f_ring"].data_ptr(),
                          dev["f_cmd"].data_ptr(), asynchronous=False)
        assert same(obs, CM.observe(m, mst, tr[t], all_first=t == 0)) and same(cmd, CM.actuate(m, mst, f0[t])), t
        _hv_same(st, mst, t)
        _hv_same({k: v.cpu().numpy() for k, v in dev.items()}, mst, (t, "device"))


# ------------------------------------------------------------------------------- sessions
def _gaits(B):
    from mpcq import synth
    return np.stack([synth.gait_table(("trot", "bound")[b % 2], N) for b in range(B)])


def _open(mpcq, eng, B, channel=None, plant=True, monitor=None, scenario=None, swing=False, tables=False):
    sess = mpcq.Session(eng, B, gait0=_gaits(B))
    if swing:
        sess.enable_swing()
    if plant:
        sess.enable_plant()
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
    return sess


def _read(mpcq, sess, names):
    out = {}
    for n in names:
        read = sess.read if n.startswith("SV") else sess.plant_read if n.startswith("PV") else \
            sess.monitor_read if n.startswith("MV") else sess.scenario_read if n.startswith("CV") else sess.channel_read
        out[n] = read(getattr(mpcq, n))
    return out


def _all_same(a, b, names, ctx):
    for n in names:
        assert same(a[n], b[n]), (ctx, n)


def test_session_with_everything_vs_model(mpcq, eng):
    """Plant + monitor (auto-reset) + scenario + channel: the planner saw the observation, the
    plant integrated the truth under the delayed, scaled, noisy command."""
    B = 65
    m = CM.params(**ALL_ON)
    st = CM.new_state(B)
    plant = mpcq.Plant(eng)
    with _open(mpcq, eng, B, ALL_ON, monitor=dict(max_ticks=4, auto_reset=1), scenario=SCEN) as s:
        _hv_same(_hv(mpcq, s), st, "enabled")  # zero, every tau -1
        episodes = 0
        for k in range(10):
            truth = s.read(mpcq.SV_STATE)
            first = np.ones(B, np.int32) if k == 0 else s.read(mpcq.SV_FIRST)
            s.tick(None)
            r = _read(mpcq, s, ("SV_XREF", "SV_F0", "SV_FSTEPS", "SV_STATUS", "PV_STATE_END", "PV_F_EFF", "CV_EPOCH",
                               "CV_TICK", "CV_ROBOTS", "MV_DONE"))
            got = _hv(mpcq, s)
            # a robot whose episode ended with this tick has been reset behind it: its SV_XREF,
            # SV_F0 and SV_FSTEPS no longer tell what the tick computed.  Its observation is still
            # checked; its force rows of the model (dead state: the next tick, a first one,
            # rewrites them) are taken from the device
            live = r["MV_DONE"] == 0
            obs = CM.observe(m, st, truth, first=first)
            assert same(got["obs"], obs), k
            assert same(np.ascontiguousarray(r["SV_XREF"][:, :, 0])[live], obs[live]), k
            cmd = CM.actuate(m, st, r["SV_F0"])
            for key in ("f_cmd", "f_ring"):
                st[key][~live] = got[key][~live]
            assert same(got["f_cmd"][live], cmd[live]), k
            _hv_same(got, st, k)
            assert np.array_equal(got["clock"][:, 0], r["CV_EPOCH"]) and np.array_equal(got["clock"][:, 1], r["CV_TICK"]), k
            feet = np.ascontiguousarray(r["SV_FSTEPS"][:, 0, 1:].reshape(B, 4, 3).transpose(0, 2, 1))
            end, f_eff = plant.step(truth, feet, cmd, robots=r["CV_ROBOTS"])
            ok = live & (r["SV_STATUS"] == mpcq.STATUS_SOLVED)
            assert ok.sum() > B // 2 or not live.any(), (k, r["SV_STATUS"])
            assert same(r["PV_STATE_END"][ok], end[ok]) and same(r["PV_F_EFF"][ok], f_eff[ok]), k
            assert not live.any() or not same(r["SV_F0"][live], cmd[live])  # (the command is not the solve's result)
            episodes += int((r["MV_DONE"] != 0).sum())
        assert episodes >= B and got["clock"][:, 0].min() >= 3  # ticks 3 and 7 end every episode


@pytest.mark.parametrize("B,n", [(17, 16), (5, 32)], ids=["N16", "N32"])
def test_zero_channel_changes_nothing(mpcq, B, n):
    names = SV + PV + MV
    mon = dict(max_ticks=4, auto_reset=1)
    with mpcq.Engine(n) as e:
        mk = lambda ch: _open_n(mpcq, e, n, B, ch, mon)  # noqa: E731
        with mk(None) as a, mk({}) as b, mk({}) as c:
            c.disable_channel()
            for k in range(6):
                truth = b.read(mpcq.SV_STATE)
                for s in (a, b, c):
                    s.tick(V_REF)
                ra, rb, rc = (_read(mpcq, s, names + ("SV_ORDER",)) for s in (a, b, c))
                _all_same(ra, rb, names, (k, "zero"))
                _all_same(ra, rc, names, (k, "disabled"))
                for r in (ra, rb, rc):
                    assert np.array_equal(np.sort(r["SV_ORDER"]), np.arange(B)), k
                live = rb["MV_DONE"] == 0  # (an ended episode's SV_F0 has been reset behind the tick)
                assert same(b.channel_read(mpcq.HV_OBS), truth), k
                assert same(b.channel_read(mpcq.HV_F_CMD)[live], rb["SV_F0"][live]), k
            assert (c.channel_read(mpcq.HV_CLOCK)[:, 1] == -1).all()  # never launched


def _open_n(mpcq, e, n, B, channel, monitor):
    from mpcq import synth
    sess = mpcq.Session(e, B, gait0=np.stack([synth.gait_table(("trot", "bound")[b % 2], n) for b in range(B)]))
    sess.enable_plant()
    sess.enable_monitor(**monitor)
    if channel is not None:
        sess.enable_channel(**channel)
    return sess


def test_latency_alone(mpcq, eng):
    B = 17
    with _open(mpcq, eng, B, dict(latency=1)) as a, _open(mpcq, eng, B, None) as b:
        prev = None
        for k in range(5):
            a.tick(V_REF)
            f0, cmd = a.read(mpcq.SV_F0), a.channel_read(mpcq.HV_F_CMD)
            assert same(cmd, np.tile(CM.F_INIT, (B, 1)) if k == 0 else prev), k
            if k == 0:  # the first solve has seen no effect of the channel yet
                b.tick(V_REF)
                assert same(f0, b.read(mpcq.SV_F0))
                assert not same(a.plant_read(mpcq.PV_STATE_END), b.plant_read(mpcq.PV_STATE_END))
            prev = f0


def test_reset_restarts_those_robots_only(mpcq, eng):
    B = 18
    ch = dict(ALL_ON, hold_prob=0.0)
    mask = (np.arange(B) % 3 == 0).astype(np.int32)
    keep = mask == 0
    with _open(mpcq, eng, B, ch) as a, _open(mpcq, eng, B, ch) as b:
        for k in range(8):
            if k == 5:
                a.reset(mask)
            truth = a.read(mpcq.SV_STATE)
            a.tick(V_REF)
            b.tick(V_REF)
            ha, hb = _hv(mpcq, a), _hv(mpcq, b)
            for key in KEYS:
                assert same(ha[key][keep], hb[key][keep]), (k, key)
            assert same(a.read(mpcq.SV_F0)[keep], b.read(mpcq.SV_F0)[keep]), k
            if k == 5:  # a new epoch from tau 0: rings refilled, the initial result back in force
                r = mask != 0
                assert ha["clock"][r].tolist() == [[2, 1]] * int(r.sum()) and hb["clock"][r].tolist() == [[1, 6]] * int(r.sum())
                assert same(ha["s_ring"][r], np.repeat(truth[r][:, None, :], 8, axis=1))
                ring = np.repeat(np.tile(CM.F_INIT, (int(r.sum()), 1))[:, None, :], 4, axis=1)
                ring[:, 0] = a.read(mpcq.SV_F0)[r]  # (slot tau % latency took this tick's f0)
                assert same(ha["f_ring"][r], ring)
                m = CM.params(**ch)
                idx = np.nonzero(r)[0]
                assert same(ha["draw"][r, :12], np.array(m.bias) * CM.sym(CM.philox(m, idx[:, None], 2, 0, CM.S_BIAS + np.arange(12))))
        assert ha["clock"].tolist() == [[2, 3] if x else [1, 8] for x in mask]


def test_enable_in_mid_run(mpcq, eng):
    B = 9
    m = CM.params(delay=2)
    with _open(mpcq, eng, B, None) as s:
        for k in range(4):
            s.tick(V_REF)
        s.enable_channel(delay=2)
        st = CM.new_state(B)
        _hv_same(_hv(mpcq, s), st, "enabled")
        for k in range(4, 8):
            truth = s.read(mpcq.SV_STATE)
            s.tick(V_REF)
            obs = CM.observe(m, st, truth)
            CM.actuate(m, st, s.read(mpcq.SV_F0))
            got = _hv(mpcq, s)
            _hv_same(got, st, k)
            if k == 4:  # primed: its own truth, epoch 0, tau counting from the enable
                assert same(got["obs"], truth) and got["clock"].tolist() == [[0, 1]] * B
            if k == 7:
                assert not same(obs, truth)
        s.enable_channel(delay=2, sigma=[0.01] * 12)  # the same depths: the amplitudes only
        assert (s.channel_read(mpcq.HV_CLOCK)[:, 1] == 4).all()
        s.enable_channel(delay=5)  # other depths: primes again
        assert (s.channel_read(mpcq.HV_CLOCK)[:, 1] == ~4).all()
        CM.arm(st)
        m = CM.params(delay=5)
        for k in range(8, 11):
            truth = s.read(mpcq.SV_STATE)
            s.tick(V_REF)
            obs = CM.observe(m, st, truth)
            CM.actuate(m, st, s.read(mpcq.SV_F0))
            _hv_same(_hv(mpcq, s), st, k)
            assert same(obs, truth) == (k == 8)
        with pytest.raises(mpcq.MpcqError, match="delay"):
            s.enable_channel(delay=9)
        assert s.channel_params.delay == 5  # the parameters in force stay
        truth = s.read(mpcq.SV_STATE)
        s.tick(V_REF)
        CM.observe(m, st, truth)
        CM.actuate(m, st, s.read(mpcq.SV_F0))
        _hv_same(_hv(mpcq, s), st, "after the refusal")


# ------------------------------------------------------------------------------- snapshots
SNAP_B = 17
EVERYTHING = dict(monitor=dict(max_ticks=5, auto_reset=1), scenario=SCEN, swing=True, tables=True)


def _ticks(mpcq, s, n):
    out = []
    for _ in range(n):
        s.tick(None)
        out.append(_read(mpcq, s, HV + ("SV_F0", "SV_STATE", "PV_F_EFF")))
    return out


def test_snapshot_save_restore_and_blob(mpcq, eng):
    names = HV + ("SV_F0", "SV_STATE", "PV_F_EFF")
    with _open(mpcq, eng, SNAP_B, ALL_ON, **EVERYTHING) as s:
        _ticks(mpcq, s, 6)
        snap = s.snapshot()
        want = _ticks(mpcq, s, 6)
        s.restore(snap)
        got = _ticks(mpcq, s, 6)
        for k in range(6):
            _all_same(got[k], want[k], names, k)
        blob = snap.tobytes()
        version, = struct.unpack_from("<I", blob, 8)
        flags, = struct.unpack_from("<I", blob, 28)
        part, = struct.unpack_from("<q", blob, 104)
        delay, latency = struct.unpack_from("<ii", blob, 112)
        assert version == 2 and flags & 256 and (delay, latency) == (3, 2)
        assert part == SNAP_B * (8 + 96 + 96 + 128 + 8 * 96 + 4 * 96)
        assert struct.unpack_from("<q", blob, 120) == (0,)
        # the part is the blob's tail: the six arrays, unpadded, by id
        tail = np.frombuffer(blob[-part:], np.uint8)
        s.restore(snap)
        hv = np.concatenate([s.channel_read(getattr(mpcq, n)).view(np.uint8).reshape(-1) for n in HV])
        assert np.array_equal(tail, hv)
        # export / import into a fresh session continues equally
        with _open(mpcq, eng, SNAP_B, ALL_ON, **EVERYTHING) as f:
            f.restore(f.snapshot_from(blob))
            got = _ticks(mpcq, f, 6)
            for k in range(6):
                _all_same(got[k], want[k], names, (k, "imported"))
        # other depths in force: refused before anything is launched
        with _open(mpcq, eng, SNAP_B, dict(ALL_ON, delay=2), **EVERYTHING) as o:
            _ticks(mpcq, o, 2)
            before = _read(mpcq, o, names)
            with pytest.raises(mpcq.MpcqError, match="delay"):
                o.restore(snap)
            with pytest.raises(mpcq.MpcqError, match="delay"):
                o.restore(o.snapshot_from(blob))
            _all_same(_read(mpcq, o, names), before, names, "refused")
        snap.close()
    # a session without a channel still writes version 1, nothing at the new offsets
    with _open(mpcq, eng, SNAP_B, None, **EVERYTHING) as p:
        for _ in range(2):
            p.tick(None)
        with p.snapshot() as snap1:
            blob1 = snap1.tobytes()
        assert struct.unpack_from("<I", blob1, 8) == (1,) and not struct.unpack_from("<I", blob1, 28)[0] & 256
        assert blob1[104:128] == bytes(24)
        with _open(mpcq, eng, SNAP_B, ALL_ON, **EVERYTHING) as q:
            with pytest.raises(mpcq.MpcqError, match="channel"):
                q.restore(q.snapshot_from(blob1))


def test_fork_branches_a_robot(mpcq, eng):
    """fork(r): every slot continues from robot r.  The tick after it, slot b's observation
    reads the ring (r's truths) under r's bias (HV_DRAW came along) with slot b's own noise, so
    the arrays that must match robot r of a twin right after the fork are the rows the gather
    copied -- all six HV arrays and the solver's state; after the next tick, HV_CLOCK, HV_DRAW
    and HV_S_RING still match (the truth has not diverged yet: it is the plant's state of the
    fork tick), HV_OBS matches the model fed slot b's draws."""
    r = 5
    ch = dict(ALL_ON, hold_prob=0.0)
    m = CM.params(**ch)
    with _open(mpcq, eng, SNAP_B, ch, **EVERYTHING) as a, _open(mpcq, eng, SNAP_B, ch, **EVERYTHING) as b:
        _ticks(mpcq, a, 6)
        _ticks(mpcq, b, 6)
        a.fork(r)
        ha, hb = _hv(mpcq, a), _hv(mpcq, b)
        for k in KEYS:
            assert same(ha[k], np.repeat(hb[k][r:r + 1], SNAP_B, axis=0)), k
        assert same(a.read(mpcq.SV_STATE), np.repeat(b.read(mpcq.SV_STATE)[r:r + 1], SNAP_B, axis=0))
        st = {k: v.copy() for k, v in ha.items()}
        truth = a.read(mpcq.SV_STATE)
        first = a.read(mpcq.SV_FIRST)
        a.tick(None)
        b.tick(None)
        ga, gb = _hv(mpcq, a), _hv(mpcq, b)
        obs = CM.observe(m, st, truth, first=first)
        assert same(ga["obs"], obs)
        for k in ("clock", "draw", "s_ring"):
            assert same(ga[k], np.repeat(gb[k][r:r + 1], SNAP_B, axis=0)), k
        assert same(ga["obs"][r], gb["obs"][r]) and not same(ga["obs"][0], gb["obs"][r])  # slot 0: its own noise
