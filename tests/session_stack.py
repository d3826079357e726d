"""A session with every stage and every table on, and the chain that checks one of its ticks
launch by launch (tests/test_gpu_session_stack.py).

``open_stack`` builds the session; ``Chain`` holds the stand-alone entry points on the same engine
(mpcq.Scenario, Channel, Estimator, Disturb, Gait, Engine.plan, Engine.solve, Plant, Monitor,
Swing: the kernels a session's tick launches) and ``Chain.check`` feeds each of them the arrays
the session's own tick read -- every array of every group is read before and after the tick -- and
compares with what the tick wrote, in session_tick's order.  Nothing compounds over ticks, so
every comparison is bit for bit except the plant against its numpy model (tests/plant_model.py),
which is held to test_gpu_plant.py's TOL.  What each launch must have read is in the comments of
``check``; a launch wired to another array (the plant to SV_F0 under a channel, the disturb stage
to the truth, the compensating solve to the user's table) fails its row.
"""
import numpy as np

import gait_cases as GC
import plant_model as PM
import weight_cases as WC
from monitor_model import OK_STATUS, same

PLANT_TOL = 1e-12  # test_gpu_plant.TOL: its bound for these formulas (ocml's sin / cos against numpy's)

SV = ("SV_F0", "SV_X", "SV_X_ROBOT", "SV_Q_W", "SV_COST", "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_STATUS", "SV_ITERS",
      "SV_RHO", "SV_Y", "SV_STATE", "SV_L_FEET", "SV_ROT_FLAG", "SV_H_ROT", "SV_ORDER", "SV_FIRST", "SV_SWING_REF",
      "SV_SWING_STATE", "SV_FRAME")
GROUPS = (("read", SV),
          ("plant_read", ("PV_STATE_END", "PV_F_EFF", "PV_WRENCH")),
          ("monitor_read", ("MV_DONE", "MV_EP", "MV_EP_TICKS", "MV_EPISODES", "MV_LAST", "MV_TOTALS")),
          ("scenario_read", ("CV_EPOCH", "CV_TICK", "CV_V_REF", "CV_PUSH", "CV_WRENCH", "CV_ROBOTS", "CV_DRAW")),
          ("channel_read", ("HV_CLOCK", "HV_OBS", "HV_F_CMD", "HV_DRAW", "HV_S_RING", "HV_F_RING")),
          ("estimator_read", ("EV_EST", "EV_ROW")),
          ("disturb_read", ("DV_DIST", "DV_ROW", "DV_RESID")),
          ("gait_state", ("GV_STATE",)))
# SV_ORDER: the order inside a bucket of iteration counts is arbitrary by design (LDS atomics)
UNORDERED = ("SV_ORDER",)

SCENARIO = dict(seed=20240611, commands=1, cmd_start=1, cmd_ramp=3, cmd_period=6,
                v_lo=[0.1, -0.1, -0.3], v_hi=[0.6, 0.1, 0.3],
                pushes=1, push_first=2, push_period=5, push_jitter=2, push_ticks=2, push_prob=0.6, push_flip=0b000011,
                wrench_lo=[2.0, -4.0, -6.0, -0.2, -0.2, -0.1], wrench_hi=[8.0, 4.0, 3.0, 0.2, 0.2, 0.1],
                robots=3, mass_scale_lo=0.9, mass_scale_hi=1.2, mu_lo=0.6, mu_hi=1.0)
CHANNEL = dict(seed=77, delay=2, latency=1, hold_prob=0.25, sigma=[1e-3] * 6 + [1e-2] * 6,
               bias=[2e-3] * 6 + [5e-3] * 6, f_gain=0.05, f_sigma=[0.05, 0.05, 0.1])
ESTIMATOR = dict(lag=2, f_lag=1, r=[1e-6] * 6 + [1e-4] * 6)
DISTURB = dict(alpha=0.3, f_lag=1, compensate=1)
MAX_TICKS = 13
LIBRARY = ("trot", "bound", "stand")


def config(mpcq, N, B, bad_gait=None, bad_tick=17):
    """The tables, parameters and the schedule of one stack session (a dict; host data only).
    ``bad_gait``: the robot whose table loses its terminator before tick ``bad_tick`` (None: none)."""
    from mpcq import synth
    rng = np.random.default_rng(500 + N + B)
    wrench = np.zeros((B, 6))
    wrench[1] = [4.0, -2.0, 0.0, 0.0, 0.1, 0.0]
    user = mpcq.disturbances(B, lin=rng.uniform(-0.4, 0.4, (B, 3)), ang=rng.uniform(-0.5, 0.5, (B, 3)))
    # requests ahead of ticks 3, 9, 22 and 30, for some robots (-1: none)
    requests = {3: [1, -1, 2] + [-1] * (B - 3), 9: [-1, 0, -1] + [-1] * (B - 3)}
    if B <= 4:  # (a short run: a request ahead of its second tick too)
        requests[1] = [2, 1, -1] + [-1] * (B - 3)
    else:
        requests.update({22: [-1] * (B - 2) + [1, 0], 30: [2] + [-1] * (B - 1)})
    return dict(
        N=N, B=B,
        gait0=np.stack([synth.gait_table(("trot", "bound")[b % 2], N) for b in range(B)]),
        robots=mpcq.robots(B, mass=rng.uniform(2.3, 2.7, B), mu=rng.uniform(0.7, 1.0, B)),
        plant_robots=mpcq.robots(B, mass=rng.uniform(2.2, 2.9, B), mu=rng.uniform(0.6, 1.0, B)),
        weights=WC.make_weights(N, B=B), user=user, wrench=wrench, requests=requests,
        bad_gait=bad_gait, bad_tick=bad_tick)


def open_stack(mpcq, eng, cfg, auto_reset):
    """The session of ``cfg`` on ``eng``: every table set, every stage enabled."""
    s = mpcq.Session(eng, cfg["B"], gait0=cfg["gait0"])
    s.set_robots(cfg["robots"])
    s.set_weights(cfg["weights"])
    s.set_disturbance(cfg["user"])
    s.set_plant_robots(cfg["plant_robots"])
    s.set_wrench(cfg["wrench"])
    s.enable_swing()
    s.enable_plant()
    s.enable_monitor(max_ticks=MAX_TICKS, auto_reset=int(auto_reset))
    s.enable_scenario(**SCENARIO)
    s.enable_channel(**CHANNEL)
    s.enable_estimator(**ESTIMATOR)
    s.enable_disturb(**DISTURB)
    s.enable_gait(list(LIBRARY))
    return s


def before_tick(mpcq, sess, cfg, k):
    """The schedule's interventions ahead of tick k: gait requests, and the lost terminator."""
    if k in cfg["requests"]:
        sess.set_gait(cfg["requests"][k])
    if cfg["bad_gait"] is not None and k == cfg["bad_tick"]:
        g = sess.read(mpcq.SV_GAIT)
        g[cfg["bad_gait"], :, 0] = 1.0  # no terminator: the reference planner raises
        sess.write(mpcq.SV_GAIT, g)


def intervention_ticks(cfg):
    t = set(cfg["requests"])
    if cfg["bad_gait"] is not None:
        t.add(cfg["bad_tick"])
    return sorted(t)


def read_all(mpcq, sess):
    """Every array of every group, by name."""
    out = {}
    for fn, names in GROUPS:
        for n in names:
            out[n] = getattr(sess, fn)() if fn == "gait_state" else getattr(sess, fn)(getattr(mpcq, n))
    return out


def same_reads(a, b, ctx):
    for n in a:
        if n in UNORDERED:
            assert sorted(a[n].tolist()) == sorted(b[n].tolist()), (ctx, n)
            continue
        x, y = (v.view(np.uint8) if v.dtype.names else v for v in (a[n], b[n]))
        assert same(x, y), (ctx, n)


def bits(a, b):
    """Equal bit for bit, a NaN equal to a NaN of any payload; structured arrays by their bytes."""
    if a.dtype.names:
        return a.tobytes() == b.tobytes()
    return a.shape == b.shape and same(a, b)


def feet_of(fsteps):
    """Row 0 of fsteps (B, 20, 13) laid out as l_feet (B, 3, 4)."""
    return np.ascontiguousarray(fsteps[:, 0, 1:].reshape(fsteps.shape[0], 4, 3).transpose(0, 2, 1))


def shifted(x, N):
    """The next tick's warm start of solutions x (B, 24N): states up one stage with the last
    zeroed, forces rolled by one stage (MPC.py:403-406): copies only."""
    n = 12 * N
    return np.concatenate([x[:, 12:n], np.zeros((x.shape[0], 12)), np.roll(x[:, n:], -12, axis=1)], axis=1)


class Chain:
    """The stand-alone entry points of one stack session, and what the test carries between ticks
    (the swing generators' state; the power counters)."""

    def __init__(self, mpcq, oracle, eng, sess, cfg):
        self.m, self.O, self.eng, self.sess, self.cfg = mpcq, oracle, eng, sess, cfg
        B = cfg["B"]
        self.scenario = mpcq.Scenario(eng, sess.scenario_params)
        self.channel = mpcq.Channel(eng, sess.channel_params)
        self.estimator = mpcq.Estimator(eng, sess.estimator_params)
        self.disturb = mpcq.Disturb(eng, sess.disturb_params)
        self.gait = mpcq.Gait(eng, sess.gait_cycles, sess.gait_params)
        self.plant = mpcq.Plant(eng, sess.plant_params)
        self.monitor = mpcq.Monitor(eng, sess.monitor_params)
        self.swing = mpcq.Swing(eng, B, sess.swing_params)
        self.oparams = [oracle.default_params(**WC.oracle_overrides(cfg["weights"][b])) for b in range(B)]
        self.shoulders = np.array(sess.planner_params.shoulders[:])
        self.plant_kw = dict(dt=sess.plant_params.dt, gravity=sess.plant_params.gravity, n_sub=sess.plant_params.n_sub,
                             integrator=sess.plant_params.integrator, clamp=sess.plant_params.clamp)
        self.worst_plant = 0.0
        self.trace = []
        self.seen = dict(first_late=0, held=0, pushed=0, switched=0, bad_gait=0, warm_solved=0, dist_differs=0,
                         plant_bits=0, failed_plant=0, statuses=set())

    def after_reset(self, mask):
        """The test's own reset of the robots in ``mask``: their swing generators start anew."""
        self.swing.state[np.asarray(mask) != 0] = 0.0

    def _solve(self, sel, xref, fsteps, dist, mode, **warm):
        e, c = self.eng, self.cfg
        e.set_robots(c["robots"][sel])
        e.set_weights(c["weights"][sel])
        e.set_disturbance(dist[sel])
        try:
            return e.solve(xref[sel], fsteps[sel], mode, want_x=True, want_y=True, **warm)
        finally:
            e.set_robots(None)
            e.set_weights(None)
            e.set_disturbance(None)

    def check(self, k, b4, now):
        """One tick: ``b4`` / ``now`` = read_all before / after it."""
        m, c, N, B = self.m, self.cfg, self.cfg["N"], self.cfg["B"]
        cp = lambda n: np.ascontiguousarray(b4[n]).copy()  # noqa: E731
        all_first = k == 0
        first = np.ones(B, bool) if all_first else b4["SV_FIRST"] != 0
        mask = None if all_first else first.astype(np.int32)
        failed_prev = ~np.isin(b4["SV_STATUS"], OK_STATUS)
        ctx = lambda what: (k, what)  # noqa: E731

        # ---- scenario: CV_* before, the first flags, base = the plant's robots, the user's wrench
        cv = dict(epoch=cp("CV_EPOCH"), tick=cp("CV_TICK"), robots=cp("CV_ROBOTS"), draw=cp("CV_DRAW"))
        v_ref, push, wrench, cv = self.scenario.step(cv, first=mask, all_first=all_first, base=c["plant_robots"],
                                                     wrench_in=b4["PV_WRENCH"])
        for n, want in (("CV_V_REF", v_ref), ("CV_PUSH", push), ("CV_WRENCH", wrench), ("CV_EPOCH", cv["epoch"]),
                        ("CV_TICK", cv["tick"]), ("CV_ROBOTS", cv["robots"]), ("CV_DRAW", cv["draw"])):
            assert bits(now[n], want), ctx(n)
        assert bits(now["PV_WRENCH"], b4["PV_WRENCH"]), ctx("PV_WRENCH")

        # ---- observe: the truth is SV_STATE before the tick
        hv = dict(clock=cp("HV_CLOCK"), obs=cp("HV_OBS"), f_cmd=cp("HV_F_CMD"), draw=cp("HV_DRAW"),
                  s_ring=cp("HV_S_RING"), f_ring=cp("HV_F_RING"))
        obs, hv = self.channel.observe(b4["SV_STATE"], hv, first=mask, all_first=all_first)
        for n, want in (("HV_OBS", obs), ("HV_S_RING", hv["s_ring"]), ("HV_CLOCK", hv["clock"])):
            assert bits(now[n], want), ctx(n)

        # ---- estimate: the observation, the previous f0 / feet / status, the model's robots
        feet_prev = feet_of(b4["SV_FSTEPS"])
        kw = dict(first=mask, all_first=all_first, failed_prev=failed_prev, robots=c["robots"])
        est, erow = self.estimator.step(now["HV_OBS"], b4["SV_F0"], feet_prev, cp("EV_ROW"), **kw)
        assert bits(now["EV_EST"], est), ctx("EV_EST")
        assert bits(now["EV_ROW"], erow), ctx("EV_ROW")

        # ---- disturb: the estimate (what the planner is about to read), not the truth or the observation
        dist, resid, drow = self.disturb.step(now["EV_EST"], b4["SV_F0"], feet_prev, cp("DV_ROW"), **kw)
        assert bits(now["DV_DIST"], dist), ctx("DV_DIST")
        assert bits(now["DV_RESID"], resid), ctx("DV_RESID")
        assert bits(now["DV_ROW"], drow), ctx("DV_ROW")

        # ---- gait + planner: state = EV_EST, feet = SV_L_FEET before, the command = CV_V_REF; the
        # gait stage rolls, the planner runs footsteps + reference states; first robots as k = 0
        # with the footsteps-only pass ahead of the roll
        gait, rot, hrot = cp("SV_GAIT"), cp("SV_ROT_FLAG"), cp("SV_H_ROT")
        xref, fsteps, gst = cp("SV_XREF"), cp("SV_FSTEPS"), cp("GV_STATE")
        plan_status = np.zeros(B, np.int32)
        pp = self.sess.planner_params

        def plan(sel, ops, kk):
            sub = [np.ascontiguousarray(a[sel]) for a in (gait, rot, hrot, xref, fsteps)]
            st = self.eng.plan(ops, kk, now["EV_EST"][sel], b4["SV_L_FEET"][sel], now["CV_V_REF"][sel], *sub, params=pp)
            for a, s in zip((gait, rot, hrot, xref, fsteps), sub):
                a[sel] = s
            return st

        if first.any():
            plan_status[first] = plan(first, m.PLAN_FOOTSTEPS, 0)
        gait, gst = self.gait.roll(gait, gst, v_ref=now["CV_V_REF"])
        ops = m.PLAN_FOOTSTEPS | m.PLAN_REFSTATES
        if first.any():
            st = plan(first, ops, 0)
            plan_status[first] = np.where(st != 0, st, plan_status[first])
        if (~first).any():
            plan_status[~first] = plan(~first, ops, k)
        for n, want in (("SV_GAIT", gait), ("GV_STATE", gst), ("SV_XREF", xref), ("SV_FSTEPS", fsteps),
                        ("SV_ROT_FLAG", rot), ("SV_H_ROT", hrot)):
            assert bits(now[n], want), ctx(n)
        assert np.array_equal(now["SV_STATUS"] == m.STATUS_BAD_GAIT, plan_status == m.STATUS_BAD_GAIT), ctx("plan status")

        # ---- solve: the planner's outputs under the robots and weights tables and DV_DIST (the
        # stage compensates: not the user's table); warm robots from the shifted SV_X / SV_Y /
        # SV_RHO before (zeros after a failed tick), first robots in set-up mode, cold
        x, y = np.empty((B, 24 * N)), np.empty((B, 44 * N))
        f0, rho = np.empty((B, 12)), np.empty(B)
        status, iters = np.empty(B, np.int32), np.empty(B, np.int32)
        warm = ~first
        if warm.any():
            wx = shifted(b4["SV_X"], N)
            wx[failed_prev] = 0.0
            r = self._solve(warm, now["SV_XREF"], now["SV_FSTEPS"], now["DV_DIST"], m.MODE_UPDATE, warm_x=wx[warm],
                            warm_y=b4["SV_Y"][warm], rho=b4["SV_RHO"][warm])
            x[warm], y[warm], f0[warm], rho[warm] = r["x"], r["y"], r["f0"], r["rho"]
            status[warm], iters[warm] = r["status"], r["iters"]
        if first.any():
            r = self._solve(first, now["SV_XREF"], now["SV_FSTEPS"], now["DV_DIST"], m.MODE_SETUP)
            x[first], y[first], f0[first], rho[first] = r["x"], r["y"], r["f0"], r["rho"]
            status[first], iters[first] = r["status"], r["iters"]
        # the retrieve's rule: the planner's status over the engine's; a failed robot restarts cold
        status = np.where(plan_status != 0, plan_status, status)
        failed = ~np.isin(status, OK_STATUS)
        y[failed] = 0.0
        rho[failed] = self.eng.params.rho
        for n, want in (("SV_X", x), ("SV_F0", f0), ("SV_ITERS", iters), ("SV_STATUS", status), ("SV_Y", y),
                        ("SV_RHO", rho)):
            assert bits(now[n], want), ctx(n)

        # ---- retrieve: x_robot and the cost components under the robot's own weights
        for b in range(B):
            o = self.O.retrieve(N, now["SV_X"][b], now["SV_XREF"][b], now["SV_FSTEPS"][b], now["SV_GAIT"][b],
                                b4["SV_Q_W"][b], failed=bool(failed[b]), params=self.oparams[b], shoulders=self.shoulders)
            assert bits(now["SV_X_ROBOT"][b], o["x_robot"]), ctx(("SV_X_ROBOT", b))
            assert bits(now["SV_COST"][b], o["cost"]), ctx(("SV_COST", b))
        assert not now["SV_FIRST"].any(), ctx("SV_FIRST")

        # ---- actuate: this tick's SV_F0 through the channel
        f_cmd, hv = self.channel.actuate(now["SV_F0"], hv)
        for n, want in (("HV_F_CMD", f_cmd), ("HV_F_RING", hv["f_ring"]), ("HV_DRAW", hv["draw"])):
            assert bits(now[n], want), ctx(n)

        # ---- plant: the truth under HV_F_CMD (not SV_F0), the scenario's wrench and robots
        ok = ~failed
        r = PM.session_tick(b4["SV_STATE"][ok], now["SV_FSTEPS"][ok], now["SV_GAIT"][ok], now["HV_F_CMD"][ok],
                            b4["SV_Q_W"][ok], now["CV_WRENCH"][ok], PM.from_table(now["CV_ROBOTS"][ok]),
                            shoulders=self.shoulders.reshape(2, 4), **self.plant_kw)
        assert bits(now["PV_F_EFF"][ok], r["f_eff"]), ctx("PV_F_EFF")
        for n, want in (("PV_STATE_END", r["end"]), ("SV_Q_W", r["q_w"]), ("SV_STATE", r["state"]),
                        ("SV_L_FEET", r["l_feet"])):
            d = float(np.abs(now[n][ok] - want).max(initial=0.0))
            self.worst_plant = max(self.worst_plant, d)
            assert d <= PLANT_TOL, (ctx(n), d)
        for n in ("SV_Q_W", "SV_STATE", "SV_L_FEET"):  # a failed robot keeps its pose and state
            assert bits(now[n][failed], b4[n][failed]), ctx((n, "failed"))
        assert np.isnan(now["PV_STATE_END"][failed]).all(), ctx("PV_STATE_END of the failed robots")
        calm = ok & ~now["CV_WRENCH"].any(axis=1)  # no wrench: the stand-alone step has the same inputs
        if calm.any():
            end, f_eff = self.plant.step(b4["SV_STATE"][calm], feet_of(now["SV_FSTEPS"][calm]), now["HV_F_CMD"][calm],
                                         None, now["CV_ROBOTS"][calm])
            assert bits(now["PV_STATE_END"][calm], end), ctx("PV_STATE_END against Plant.step")
            assert bits(now["PV_F_EFF"][calm], f_eff), ctx("PV_F_EFF against Plant.step")

        # ---- monitor: the arrays the plant left, the scenario's command
        acc = dict(ep=cp("MV_EP"), ep_ticks=cp("MV_EP_TICKS"), episodes=cp("MV_EPISODES"), last=cp("MV_LAST"),
                   totals=cp("MV_TOTALS"))
        done, acc, tr = self.monitor.step(now["SV_Q_W"], now["SV_STATUS"], now["SV_ITERS"], now["SV_F0"], now["SV_COST"],
                                          now["SV_STATE"], now["CV_V_REF"], acc)
        for n, want in (("MV_DONE", done), ("MV_EP", acc["ep"]), ("MV_EP_TICKS", acc["ep_ticks"]),
                        ("MV_EPISODES", acc["episodes"]), ("MV_LAST", acc["last"]), ("MV_TOTALS", acc["totals"])):
            assert bits(now[n], want), ctx(n)
        self.trace.append(tr)

        # ---- order: a permutation of the robots
        assert sorted(now["SV_ORDER"].tolist()) == list(range(B)), ctx("SV_ORDER")

        # ---- swing: this tick's gait and fsteps in the frame of the pose before the tick
        frame = np.ascontiguousarray(b4["SV_Q_W"][:, [0, 1, 5]])
        assert bits(now["SV_FRAME"], frame), ctx("SV_FRAME")
        ref = self.swing.advance(now["SV_GAIT"], now["SV_FSTEPS"], frame, 0, int(self.sess.swing_params.k_mpc))
        assert bits(now["SV_SWING_REF"], ref), ctx("SV_SWING_REF")
        assert bits(now["SV_SWING_STATE"], self.swing.state), ctx("SV_SWING_STATE")

        # ---- what the run met
        s = self.seen
        s["first_late"] += int(first.sum()) if k > 0 else 0
        # a held frame: the observation is the previous one again on a tick that is neither first nor priming
        s["held"] += int((~first & (now["HV_OBS"] == b4["HV_OBS"]).all(axis=1) & (b4["HV_CLOCK"][:, 1] > 0)).sum())
        s["pushed"] += int(now["CV_PUSH"].any())
        s["switched"] += int((now["GV_STATE"][:, 1] != b4["GV_STATE"][:, 1]).sum())
        s["bad_gait"] += int((status == m.STATUS_BAD_GAIT).sum())
        s["warm_solved"] += int((warm & (status == m.STATUS_SOLVED)).sum())
        s["dist_differs"] += int(sum(now["DV_DIST"]["a"][b].any() and not np.array_equal(now["DV_DIST"]["a"][b], c["user"]["a"][b])
                                     for b in range(B)))
        s["plant_bits"] += int(calm.sum())
        s["failed_plant"] += int(failed.sum())
        s["statuses"] |= set(status.tolist())
