"""Generate tests/golden/swing_golden.npz (run where the reference tree is; never by a test).

    MPC_TSID_REFERENCE=<reference checkout> python tests/golden/gen_swing_golden.py

Imports the UNMODIFIED reference files FootTrajectoryGenerator.py, FootstepPlanner.py and
TSID_Debug_controller_four_legs_fb_vel.py.  The controller module imports pinocchio, tsid,
pybullet, utils and matplotlib at its top; empty stand-ins go into ``sys.modules`` (plus
``np.int = int``, removed in numpy 2).  ``controller.update_footsteps`` (TSID:471-487) and
``controller.update_feet_tasks`` (TSID:247-327) then run *unbound* on a plain stub object that
holds ``k_mpc, dt, t_swing, mgoals, goals, vgoals, agoals, ftgs`` and no-op stand-ins for
``sampleFeet / feetTask / feetGoal``.  The SE3 stand-in for ``interface.oMl`` is
``R(yaw) @ p + t`` in numpy.  The generators are a recording subclass of the reference
``Foot_trajectory_generator`` (it notes the arguments of each call and, in the extended run,
hands ``np.longdouble`` copies of them to the unmodified method).

Step cases (``step_*``): whole swings of 0.14 s and 0.16 s, every call from t0 = 0 to the last
step t0 = t1 - dt, re-targeted at random every step, so adaptive and locked mode and t1 - t0 on
both sides of t_lock (0.14 - 0.09 = 0.05000000000000002 > 0.05 is adaptive; 0.16 - 0.11 = 0.05
is locked), plus locked calls on a new generator.  Per case: the ten inputs, the pre-state
(lastCoeffs, x1, y1), the float64 outputs and post-state, and the outputs / post-state of the
same class fed ``np.longdouble`` copies of the same inputs and pre-state.

Free-running scenarios (``<name>_sub_*``: the frame moves every substep; ``<name>_tick_*``: the
same scenario regenerated with the frame held per tick): the reference FootstepPlanner drives
24 ticks x 20 substeps of trot, bounding, side-walking, static and a two-period trot with
random v_ref and random measured feet at lift-off.  Per tick: gait, fsteps, the generators'
state after the tick.  Per substep: frame, feet0 (NaN where the reference does not read it),
t0, t_swing, mode, goals / vgoals / agoals (NaN for stance feet).  Each scenario runs a second
time with ``np.longdouble`` mgoals and generator state; the script asserts both runs take the
same branches and stores max |float64 - longdouble| per class (``free_err``: positions,
velocities, accelerations; ``step_err``: the same plus the coefficients, each coefficient slot
relative to its largest magnitude over the step cases, ``step_coef_scale``).

Tables (``tab_*``): gait tables that exercise the timing walk (random phases, a swing that wraps
over the table's end, blank rows) at random substeps, with whether the reference raises
(IndexError: a swing foot without a stance row; the empty table) and t0 / t_swing otherwise.

``params`` sub-command (``python tests/golden/gen_swing_golden.py params``): writes
tests/golden/swing_params_golden.npz, the same capture under every case of
tests/swing_param_cases.py (non-default dt, k_mpc, max_height, t_lock, mean_feet_z), keys
``<case>_...``.  Per case: trot (``sub`` and ``tick``) and bounding (``tick``) for 10 ticks of
the case's k_mpc substeps (the planner stays FootstepPlanner(0.02, n_periods): it only produces
the tables, the swing code scales them by dt * k_mpc), with the case's own ``free_err``; one
whole swing, re-targeted every step, for each t1 these scenarios produce, with the case's own
``step_err`` / ``step_coef_scale``; and ``<case>_params`` = dt, max_height, t_lock, feet_z,
k_mpc.  A plain run writes swing_golden.npz as before.

Only data leaves this script.
"""
from __future__ import annotations

import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
T_TICKS = 24
K_MPC = 20
DT = 0.001
MAX_H = 0.05
T_LOCK = 0.05
SHOULDERS = np.array([[0.19, 0.19, -0.19, -0.19], [0.15005, -0.15005, 0.15005, -0.15005]])
MASKS = {
    "trot": ((1, 1, 1, 1), (1, 0, 0, 1), (1, 1, 1, 1), (0, 1, 1, 0)),
    "bound": ((1, 1, 1, 1), (1, 1, 0, 0), (1, 1, 1, 1), (0, 0, 1, 1)),
    "side": ((1, 1, 1, 1), (1, 0, 1, 0), (1, 1, 1, 1), (0, 1, 0, 1)),
}
LD = np.longdouble
# the reference's constants (TSID:96-97, 107; Interface.py:91; main.py:21): the plain run
DEF = NS(k_mpc=K_MPC, dt=DT, max_height=MAX_H, t_lock=T_LOCK, feet_z=0.0, ticks=T_TICKS)


def import_reference():
    ref = os.environ.get("MPC_TSID_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set MPC_TSID_REFERENCE to the reference checkout")
    np.int = int
    pin = types.ModuleType("pinocchio")
    pin.switchToNumpyMatrix = lambda: None
    pyb = types.ModuleType("pybullet")
    pyb.resetBasePositionAndOrientation = lambda *a, **k: None
    sys.modules.setdefault("pinocchio", pin)
    sys.modules.setdefault("pybullet", pyb)
    sys.modules.setdefault("tsid", types.ModuleType("tsid"))
    sys.modules.setdefault("utils", types.ModuleType("utils"))
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:  # noqa: BLE001
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"] = mpl
        sys.modules["matplotlib.pyplot"] = mpl.pyplot
    if ref not in sys.path:
        sys.path.insert(0, ref)
    import FootstepPlanner  # noqa: E402
    import FootTrajectoryGenerator as ftg  # noqa: E402
    import TSID_Debug_controller_four_legs_fb_vel as tsid_ctl  # noqa: E402
    return FootstepPlanner, ftg, tsid_ctl


def recording_class(ftg):
    class Rec(ftg.Foot_trajectory_generator):
        extended = False
        last = None

        def get_next_foot(self, *args):
            self.last = tuple(float(a) for a in args)
            if self.extended:
                args = tuple(LD(a) for a in args)
            return super().get_next_foot(*args)

    return Rec


def gen_state(g):
    return np.array(list(g.lastCoeffs) + [g.x1, g.y1])


# ----------------------------------------------------------------------------- step cases
def step_cases(ftg, P=DEF, t1s=(0.14, 0.16), swings=2, seed=4100,
               fresh=((0.14, 0.10), (0.16, 0.159), (0.14, 0.09 + 1e-3))):
    """``swings`` whole swings per t1 of ``t1s``, then the (t1, t0) of ``fresh`` on new generators."""
    rng = np.random.default_rng(seed)
    rec = {k: [] for k in ("in", "pre", "out", "post", "out_ld", "post_ld")}

    def one(g64, gld, args):
        rec["in"].append(np.array(args[:10]))
        rec["pre"].append(gen_state(g64))
        gld.lastCoeffs = [LD(v) for v in g64.lastCoeffs]
        gld.x1, gld.y1 = LD(g64.x1), LD(g64.y1)
        o = g64.get_next_foot(*args)
        ol = gld.get_next_foot(*[LD(a) for a in args])
        rec["out"].append(np.array(o, np.float64))
        rec["post"].append(gen_state(g64))
        rec["out_ld"].append(np.array(ol, LD))
        rec["post_ld"].append(np.array(list(gld.lastCoeffs) + [gld.x1, gld.y1], LD))
        return o

    for t1 in t1s:
        for _ in range(swings):
            g64 = ftg.Foot_trajectory_generator(P.max_height, P.t_lock)
            gld = ftg.Foot_trajectory_generator(P.max_height, P.t_lock)
            p = [rng.uniform(-0.3, 0.3), rng.normal(0, 0.05), rng.normal(0, 0.5),
                 rng.uniform(-0.3, 0.3), rng.normal(0, 0.05), rng.normal(0, 0.5)]
            tgt = np.array([p[0], p[3]]) + rng.uniform(-0.08, 0.08, 2)
            n = int(round(t1 / P.dt))
            for k in range(n):
                t0 = float(np.round(k * P.dt, 3))
                tgt = tgt + rng.normal(0, 0.001, 2)  # the planner re-targets every step
                o = one(g64, gld, (p[0], p[1], p[2], p[3], p[4], p[5], tgt[0], tgt[1], t0, t1, P.dt))
                p = [float(v) for v in o[:6]]
    for t1, t0 in fresh:  # locked on a new generator
        g64 = ftg.Foot_trajectory_generator(P.max_height, P.t_lock)
        gld = ftg.Foot_trajectory_generator(P.max_height, P.t_lock)
        one(g64, gld, (0.1, 0.2, 0.3, -0.1, 0.0, 0.1, 0.15, -0.12, t0, t1, P.dt))
    out = {}
    f64 = {k: np.array(rec[k], np.float64) for k in ("in", "pre", "out", "post")}
    old, pld = np.array(rec["out_ld"], LD), np.array(rec["post_ld"], LD)
    mode = (f64["in"][:, 9] - f64["in"][:, 8]) > P.t_lock
    mode_ld = (f64["in"][:, 9].astype(LD) - f64["in"][:, 8].astype(LD)) > LD(P.t_lock)
    assert np.array_equal(mode, mode_ld)
    e = np.abs(f64["out"].astype(LD) - old)
    scale = np.abs(pld[:, :24]).max(axis=0)
    ce = (np.abs(f64["post"][:, :24].astype(LD) - pld[:, :24]) / scale).max()
    out["step_in"], out["step_pre"], out["step_out"], out["step_post"] = (f64[k] for k in ("in", "pre", "out", "post"))
    out["step_out_ld"], out["step_post_ld"] = old.astype(np.float64), pld.astype(np.float64)
    out["step_mode"] = mode
    out["step_coef_scale"] = scale.astype(np.float64)
    out["step_err"] = np.array([e[:, [0, 3, 6]].max(), e[:, [1, 4, 7]].max(), e[:, [2, 5, 8]].max(), ce], np.float64)
    return out


# ----------------------------------------------------------------------------- free running
class Frame:
    """interface.oMl: R(yaw) p + t."""

    def __init__(self, x, y, yaw):
        c, s = np.cos(yaw), np.sin(yaw)
        self.R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        self.t = np.array([[x], [y], [0.0]])

    def __mul__(self, p):
        return self.R @ p + self.t


class NoOp:
    def __getattr__(self, name):
        return lambda *a, **k: None


def make_stub(Rec, extended, P=DEF):
    dt_ = LD if extended else np.float64
    st = types.SimpleNamespace()
    st.k_mpc, st.dt = P.k_mpc, P.dt
    st.t_swing = np.zeros((4,))
    st.mgoals = np.zeros((6, 4), dt_)
    st.goals, st.vgoals, st.agoals = (np.full((3, 4), np.nan, dt_) for _ in range(3))
    st.footsteps = SHOULDERS.copy()
    st.ftgs = [Rec(P.max_height, P.t_lock) for _ in range(4)]
    for g in st.ftgs:
        g.extended = extended
    st.sampleFeet = [NoOp() for _ in range(4)]
    st.feetTask = [NoOp() for _ in range(4)]
    st.feetGoal = [types.SimpleNamespace(translation=None) for _ in range(4)]
    return st


def table(kind, n_periods, dt=0.02):
    g = np.zeros((20, 5))
    half = int(0.5 * 0.32 / dt)
    if kind == "static":
        g[0, 0] = 2 * half * n_periods
        g[0, 1:] = 1
    else:
        for i in range(n_periods):
            g[4 * i:4 * i + 4, 0] = (1, half - 1, 1, half - 1)
            g[4 * i:4 * i + 4, 1:] = MASKS[kind]
    return g


def draw_script(seed, held, P=DEF):
    """Everything random of a scenario, drawn once so the float64 and the extended run (and
    the planner) see the same numbers."""
    rng = np.random.default_rng(seed)
    s = {"v_ref": [], "state": [], "l_feet": [], "frame": [], "o": [], "ov": [], "oa": []}
    pose = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3, 3)])
    for _ in range(P.ticks):
        v_ref = np.zeros((6, 1))
        v_ref[0, 0], v_ref[1, 0], v_ref[5, 0] = rng.uniform(-0.5, 1.0), rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5)
        s["v_ref"].append(v_ref)
        lC = np.array([[0.0], [0.0], [0.2027682 + rng.uniform(-0.01, 0.01)]])
        abg = np.array([[rng.normal(0, 0.02)], [rng.normal(0, 0.02)], [0.0]])
        s["state"].append((lC, abg, rng.normal(0, 0.2, (3, 1)), rng.normal(0, 0.2, (3, 1))))
        s["l_feet"].append(np.vstack([SHOULDERS + rng.uniform(-0.03, 0.03, (2, 4)), np.zeros((1, 4))]))
        fr = []
        for ks in range(P.k_mpc):
            c, sn = np.cos(pose[2]), np.sin(pose[2])
            pose = pose + P.dt * np.array([c * v_ref[0, 0] - sn * v_ref[1, 0], sn * v_ref[0, 0] + c * v_ref[1, 0],
                                         v_ref[5, 0]]) + rng.normal(0, 1e-4, 3)
            fr.append(pose.copy() if not (held and ks) else fr[0].copy())
        s["frame"].append(fr)
        # measured feet (world): near the shoulders of the frame, moving
        o = np.empty((P.k_mpc, 3, 4))
        for ks in range(P.k_mpc):
            F = Frame(*fr[ks])
            o[ks] = F * np.vstack([SHOULDERS, np.zeros((1, 4))]) + np.vstack([rng.normal(0, 0.01, (2, 4)), np.zeros((1, 4))])
        s["o"].append(o)
        s["ov"].append(rng.normal(0, 0.05, (P.k_mpc, 3, 4)))
        s["oa"].append(rng.normal(0, 0.5, (P.k_mpc, 3, 4)))
    return s


def run_scenario(FP, ctl, Rec, kind, n_periods, script, extended, P=DEF):
    pl = FP.FootstepPlanner(0.02, n_periods)
    pl.gait = table(kind, n_periods)
    st = make_stub(Rec, extended, P)
    cast = (lambda a: a.astype(LD)) if extended else (lambda a: a)
    rec = {k: [] for k in ("gait", "fsteps", "gen", "frame", "feet0", "t0", "t_swing", "mode", "ref")}
    for j in range(P.ticks):
        lC, abg, lV, lW = script["state"][j]
        v_ref, l_feet = script["v_ref"][j], script["l_feet"][j]
        pl.update_fsteps(0 if j == 0 else j * P.k_mpc + 1, l_feet, np.vstack((lV, lW)), v_ref, lC[2, 0], None, None, False)
        gait, fsteps = pl.gait.copy(), pl.fsteps.copy()
        rec["gait"].append(gait)
        rec["fsteps"].append(fsteps)
        for ks in range(P.k_mpc):
            fr = script["frame"][j][ks]
            itf = types.SimpleNamespace(oMl=Frame(*fr), o_feet=cast(script["o"][j][ks]), ov_feet=cast(script["ov"][j][ks]),
                                        oa_feet=cast(script["oa"][j][ks]), mean_feet_z=P.feet_z)
            for g in st.ftgs:
                g.last = None
            st.goals[:], st.vgoals[:], st.agoals[:] = np.nan, np.nan, np.nan
            ctl.controller.update_footsteps(st, itf, fsteps)
            ctl.controller.update_feet_tasks(st, j * P.k_mpc + ks, gait, 0, itf, [0, 0, 0, 0])
            t0 = np.full(4, np.nan)
            ts = np.full(4, np.nan)
            mode = np.full(4, np.nan)
            feet0 = np.full((4, 6), np.nan)
            ref = np.full((4, 9), np.nan, LD if extended else np.float64)
            for i in range(4):
                a = st.ftgs[i].last
                if a is None:
                    assert gait[0, 1 + i] != 0
                    continue
                t0[i], ts[i] = a[8], a[9]
                assert ts[i] == st.t_swing[i] and a[10] == P.dt
                mode[i] = float((LD(a[9]) - LD(a[8])) > LD(P.t_lock)) if extended else float((a[9] - a[8]) > P.t_lock)
                if t0[i] == 0:
                    feet0[i] = (script["o"][j][ks][0, i], script["ov"][j][ks][0, i], script["oa"][j][ks][0, i],
                                script["o"][j][ks][1, i], script["ov"][j][ks][1, i], script["oa"][j][ks][1, i])
                ref[i, 0:3], ref[i, 3:6], ref[i, 6:9] = st.goals[:, i], st.vgoals[:, i], st.agoals[:, i]
            rec["frame"].append(fr)
            rec["feet0"].append(feet0)
            rec["t0"].append(t0)
            rec["t_swing"].append(ts)
            rec["mode"].append(mode)
            rec["ref"].append(ref)
        rec["gen"].append(np.array([[float(v) for v in gen_state(g)] for g in st.ftgs]))
    sh = (P.ticks, P.k_mpc)
    out = {"gait": np.array(rec["gait"]), "fsteps": np.array(rec["fsteps"]), "gen": np.array(rec["gen"])}
    for k in ("frame", "feet0", "t0", "t_swing", "mode", "ref"):
        a = np.array(rec[k])
        out[k] = a.reshape(sh + a.shape[1:])
    return out


def nan_equal(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


# ----------------------------------------------------------------------------- tables
def timing_tables(ctl, Rec):
    rng = np.random.default_rng(4200)
    tabs = []
    tabs.append(np.zeros((20, 5)))  # the empty table
    g = table("trot", 1)
    g[:, 3] = 0.0  # foot 2 never in stance
    tabs.append(g)
    g = np.zeros((20, 5))  # a full table whose swing wraps over the end (Python's gait[-1], [-2])
    g[:, 0] = rng.integers(1, 4, 20)
    g[:, 1:] = 1.0
    g[0:3, 1] = 0.0
    g[17:20, 1] = 0.0
    g[0, 4] = 0.0
    g[19, 4] = 0.0
    tabs.append(g)
    g = table("trot", 2)
    g = np.roll(g, -1, axis=0)  # starts in a swing row; blank rows at the end
    tabs.append(g)
    for _ in range(36):
        g = np.zeros((20, 5))
        nph = int(rng.integers(1, 21))
        g[:nph, 0] = rng.integers(1, 9, nph)
        g[:nph, 1:] = rng.integers(0, 2, (nph, 4))
        if rng.random() < 0.3:
            g[:nph, 1 + int(rng.integers(0, 4))] = 0.0
        tabs.append(g)
    rec = {k: [] for k in ("gait", "k_sub", "raises", "t0", "t_swing")}
    fsteps = np.zeros((20, 13))
    fsteps[0, 1:] = np.vstack([SHOULDERS, np.zeros((1, 4))]).ravel(order="F")
    for g in tabs:
        for k_sub in (0, int(rng.integers(1, K_MPC))):
            st = make_stub(Rec, False)
            itf = types.SimpleNamespace(oMl=Frame(0.0, 0.0, 0.0), o_feet=np.zeros((3, 4)), ov_feet=np.zeros((3, 4)),
                                        oa_feet=np.zeros((3, 4)), mean_feet_z=0.0)
            ctl.controller.update_footsteps(st, itf, fsteps)
            name = ""
            try:
                ctl.controller.update_feet_tasks(st, k_sub, g, 0, itf, [0, 0, 0, 0])
            except Exception as e:  # noqa: BLE001
                name = type(e).__name__
            t0, ts = np.full(4, np.nan), np.full(4, np.nan)
            if not name:
                for i in range(4):
                    if st.ftgs[i].last is not None:
                        t0[i], ts[i] = st.ftgs[i].last[8], st.ftgs[i].last[9]
            rec["gait"].append(g)
            rec["k_sub"].append(k_sub)
            rec["raises"].append(name)
            rec["t0"].append(t0)
            rec["t_swing"].append(ts)
    return {f"tab_{k}": np.array(v) for k, v in rec.items()}


def run_pair(FP, ctl, Rec, kind, n_periods, seed, held, P, tag):
    """A scenario in float64 and with np.longdouble state: the float64 arrays and
    max |float64 - longdouble| of positions, velocities, accelerations."""
    script = draw_script(seed, held, P)
    a = run_scenario(FP, ctl, Rec, kind, n_periods, script, False, P)
    b = run_scenario(FP, ctl, Rec, kind, n_periods, script, True, P)
    # both runs take the same branches
    for k in ("t0", "t_swing", "mode", "gait", "fsteps", "feet0"):
        assert nan_equal(a[k], b[k]), (tag, k)
    assert np.array_equal(np.isnan(a["ref"]), np.isnan(b["ref"]))
    d = np.abs(np.nan_to_num(a["ref"].astype(LD) - b["ref"]))
    return a, np.array([d[..., 0:3].max(), d[..., 3:6].max(), d[..., 6:9].max()], LD)


def main(path=None):
    FP, ftg, ctl = import_reference()
    Rec = recording_class(ftg)
    arrs = step_cases(ftg)
    arrs.update(timing_tables(ctl, Rec))
    names = []
    free_err = np.zeros(3, LD)
    for name, kind, n_periods, seed in (("trot", "trot", 1, 4301), ("bound", "bound", 1, 4302), ("side", "side", 1, 4303),
                                        ("static", "static", 1, 4304), ("trot2", "trot", 2, 4305)):
        names.append(name)
        for var, held in (("sub", False), ("tick", True)):
            a, err = run_pair(FP, ctl, Rec, kind, n_periods, seed, held, DEF, (name, var))
            free_err = np.maximum(free_err, err)
            for k, v in a.items():
                arrs[f"{name}_{var}_{k}"] = v
    arrs["scenarios"] = np.array(names)
    arrs["free_err"] = free_err.astype(np.float64)
    arrs["params"] = np.array([DT, MAX_H, T_LOCK, 0.0, K_MPC])
    path = path or os.path.join(HERE, "swing_golden.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("step cases", arrs["step_in"].shape[0], "adaptive", int(arrs["step_mode"].sum()), "step_err", arrs["step_err"])
    print("free_err", arrs["free_err"], "tables raising", sorted(set(arrs["tab_raises"].tolist())))


def main_params(path=None):
    """swing_params_golden.npz: every case of tests/swing_param_cases.py."""
    sys.path.insert(0, os.path.dirname(HERE))
    import swing_param_cases as SC
    FP, ftg, ctl = import_reference()
    Rec = recording_class(ftg)
    seeds = {"trot": 4301, "bound": 4302}
    arrs = {}
    for ci, case in enumerate(SC.NAMES):
        v = SC.full(case)
        P = NS(k_mpc=v["k_mpc"], dt=v["dt"], max_height=v["max_height"], t_lock=v["t_lock"], feet_z=v["feet_z"],
               ticks=SC.TICKS)
        free_err = np.zeros(3, LD)
        t1s = set()
        for name, var in SC.FREE:
            a, err = run_pair(FP, ctl, Rec, name, 1, seeds[name], var == "tick", P, (case, name, var))
            free_err = np.maximum(free_err, err)
            t1s.update(np.unique(a["t_swing"][~np.isnan(a["t_swing"])]).tolist())
            lift = a["t0"] == 0
            assert lift.any() and (a["mode"] == 1).any() and (a["mode"] == 0).any(), (case, name, var)
            for k in ("gait", "fsteps", "frame", "feet0", "t0", "t_swing", "mode", "ref"):
                arrs[f"{case}_{name}_{var}_{k}"] = a[k]
        # one whole swing for each t1 the case's scenarios produce
        st = step_cases(ftg, P, sorted(t1s), swings=1, seed=4110 + ci, fresh=())
        assert st["step_mode"].any() and (~st["step_mode"]).any() and (st["step_in"][:, 8] == 0).any(), case
        for k, a in st.items():
            arrs[f"{case}_{k}"] = a
        arrs[f"{case}_free_err"] = free_err.astype(np.float64)
        arrs[f"{case}_params"] = np.array([v[f] for f in SC.FIELDS], np.float64)
        print(case, "t1", sorted(t1s), "step cases", st["step_in"].shape[0], "adaptive", int(st["step_mode"].sum()),
              "step_err", st["step_err"], "free_err", arrs[f"{case}_free_err"])
    arrs["cases"] = np.array(SC.NAMES)
    path = path or os.path.join(HERE, "swing_params_golden.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    argv = sys.argv[1:]
    out = argv[argv.index("--out") + 1] if "--out" in argv else None  # default: next to this script
    (main_params if "params" in argv[:1] else main)(out)
