"""Host model of the disturbance stage (mpc-tsid_amd/csrc/mpcq_disturb.hip), in numpy.

A restatement of what mpcq_disturb_step_batch computes per robot, written from the rules of
include/mpcq.h in the kernel's operation order: the stage's row [DIST_ROW] is the device's, word
for word, so rows compare bit for bit where no sin / cos enters (the integer words, prev and the
ring) and up to the device library's sin / cos, divided by dt, elsewhere (the estimate d and the
sample).  The model step is estimator_model's M: plant_model's MODEL step (no clamp, no wrench)
followed by the state part of the frame change.
"""
from types import SimpleNamespace

import numpy as np

import estimator_model as EM

MAX_F_LAG = 4
D, PREV, CLOCK, RING, SLOTS, ROW = 0, 6, 18, 20, 5, 80
F_INIT = EM.F_INIT  # MPC_Wrapper.py:78


def params(**over):
    """mpcq_default_disturb_params, with overrides (a scalar fills an array field)."""
    p = dict(alpha=[0.2] * 6, d_max=[5.0] * 3 + [30.0] * 3, f_lag=0, compensate=1, skip_repeats=1, reserved=[0] * 5)
    for k, v in over.items():
        if k not in p:
            raise AttributeError(k)
        if isinstance(p[k], list):
            v = [v] * len(p[k]) if np.isscalar(v) else list(v)
            assert len(v) == len(p[k]), k
        p[k] = v
    return SimpleNamespace(**p)


def new_rows(B):
    return np.zeros((B, ROW))


def clock(rows):
    """(B, 4) int32 view: valid, tau_next, zero, zero."""
    return rows[:, CLOCK:CLOCK + 2].view(np.int32)


def ring(rows):
    """(B, 5, 12) view: slot j % 5 = tick j's f0."""
    return rows[:, RING:].reshape(rows.shape[0], SLOTS, 12)


def step(p, rows, meas, f_prev, feet_prev, first=None, all_first=False, failed=None, consts=None, dt=0.02,
         gravity=9.81):
    """One tick for B robots; rows (B, ROW) updated in place.  Returns (d (B, 6), resid (B, 6)):
    what the solve reads, and the raw sample (NaN where none was taken)."""
    y = np.array(meas, np.float64).reshape(-1, 12)
    B = y.shape[0]
    assert rows.shape == (B, ROW) and rows.dtype == np.float64
    f_last = np.array(f_prev, np.float64).reshape(B, 12)
    feet_last = np.array(feet_prev, np.float64).reshape(B, 3, 4)
    alpha, d_max = np.array(p.alpha, np.float64), np.array(p.d_max, np.float64)
    f_lag = int(p.f_lag)
    ck, rg = clock(rows), ring(rows)
    valid, tau_next = ck[:, 0].copy(), ck[:, 1].astype(np.int64)
    prev = rows[:, PREV:PREV + 12].copy()
    d = rows[:, D:D + 6].copy()
    fi = np.ones(B, bool) if all_first else (np.zeros(B, bool) if first is None else np.asarray(first) != 0)
    fa = np.zeros(B, bool) if failed is None else np.asarray(failed) != 0
    init = fi | (valid == 0) | (tau_next < 1)
    tau = np.where(init, 0, tau_next)
    ar = np.arange(B)
    # record (not by a robot that initialises)
    rec = np.flatnonzero(~init)
    rg[rec, (tau[rec] - 1) % SLOTS] = f_last[rec]
    # the force acting during tick tau - 1
    fj = tau - 1 - f_lag
    f_act = np.where((fj >= 0)[:, None], rg[ar, fj % SLOTS], F_INIT[None, :])
    skip = fa | ~np.isfinite(y).all(axis=1) | ~np.isfinite(prev).all(axis=1)
    if p.skip_repeats:
        skip |= (y.view(np.int64) == np.ascontiguousarray(prev).view(np.int64)).all(axis=1)
    with np.errstate(all="ignore"):
        pred = EM.model_step(prev, feet_last, f_act, consts, dt, gravity)
        r = (y[:, 6:] - pred[:, 6:]) / dt
        psi = prev[:, 5] + dt * prev[:, 11]
        c, s = np.cos(psi), np.sin(psi)
        rot = d.copy()
        rot[:, 0] = c * d[:, 0] + s * d[:, 1]
        rot[:, 1] = -s * d[:, 0] + c * d[:, 1]
        rot[:, 3] = c * d[:, 3] + s * d[:, 4]
        rot[:, 4] = -s * d[:, 3] + c * d[:, 4]
        d = np.where(np.isfinite(psi)[:, None], rot, d)  # (a non-finite yaw: d stays as it is)
        upd = ~skip & np.isfinite(r).all(axis=1)
        d = np.where(upd[:, None], d + alpha * (r - d), d)
        d = np.where(d > d_max, d_max, d)
        d = np.where(d < -d_max, -d_max, d)
    resid = np.where((~init & ~skip)[:, None], r, np.nan)
    d = np.where(init[:, None], 0.0, d)
    rows[:, D:D + 6] = d
    rows[:, PREV:PREV + 12] = y
    ck[:, 0] = 1
    ck[:, 1] = tau + 1
    ck[:, 2] = 0
    ck[:, 3] = 0
    return d.copy(), resid


def run(p, meas, f, feet, rows=None, consts=None, first=None, failed=None, dt=0.02, gravity=9.81):
    """The stage over meas (T,B,12) with the loop's own f / feet as the previous tick's inputs;
    first / failed: (T,B) masks or None (tick 0 is first for all).  Returns (d (T,B,6),
    resid (T,B,6), rows)."""
    T, B = meas.shape[:2]
    rows = new_rows(B) if rows is None else rows
    d, res = np.zeros((T, B, 6)), np.zeros((T, B, 6))
    for t in range(T):
        fp = f[t - 1] if t else np.zeros((B, 12))
        ft = feet[t - 1] if t else np.zeros((B, 3, 4))
        d[t], res[t] = step(p, rows, meas[t], fp, ft, first=None if first is None else first[t], all_first=t == 0,
                            failed=None if failed is None else failed[t], consts=consts, dt=dt, gravity=gravity)
    return d, res, rows


# ---- the closed loop on the oracle's pieces ------------------------------------------------------

def closed_loop(oracle, T=80, N=16, vx=0.2, p=None, compensate=True, true_mass=1.0, wrench_world=None,
                integrator=None, clamp=0, gait="trot"):
    """One robot's closed loop from the oracle's pieces: Planner.plan -> formulate -> the shift of
    the dynamics bounds by the stage's estimate -> qp_solve (warm) -> retrieve -> plant_model's
    session tick, whose end state the next tick measures.  ``p`` None: no stage at all;
    ``compensate`` False: the stage estimates, the solve does not use it.  ``true_mass``: the
    plant's mass over the model's; ``wrench_world`` (6,): a constant world-frame push.  Returns
    dict(status (T,), state (T,12) what each tick's planner read, d (T,6), h_ref)."""
    import plant_model as PM
    from mpcq import synth
    integrator = PM.MODEL if integrator is None else integrator
    prm = oracle.default_params()
    pl = oracle.Planner(N, synth.gait_table(gait, N))
    v_ref = np.array([vx, 0.0, 0.0, 0.0, 0.0, 0.0])
    consts = PM.constants(1, mass=PM.MASS * true_mass)
    wr = None if wrench_world is None else np.asarray(wrench_world, np.float64).reshape(1, 6)
    state = np.zeros(12)
    state[2] = pl.p.h_ref
    sh = np.array(pl.p.shoulders[:]).reshape(2, 4)
    l_feet = np.vstack([sh, np.zeros((1, 4))])
    q_w = np.array([0.0, 0.0, 0.2027682, 0.0, 0.0, 0.0])
    y, rho, warm_x = np.zeros(44 * N), prm.rho, np.zeros(24 * N)
    rows = new_rows(1)
    f_prev, failed = np.zeros(12), False
    out = dict(status=[], state=[], d=[], h_ref=float(pl.p.h_ref))
    for k in range(T):
        d = np.zeros(6)
        if p is not None:
            feet_prev = pl.fsteps[0, 1:].reshape(4, 3).T if k else np.zeros((3, 4))  # (as l_feet; before this tick's planner)
            dd, _ = step(p, rows, state[None], f_prev[None], feet_prev[None], all_first=k == 0,
                         failed=[failed], dt=prm.dt, gravity=prm.gravity)
            d = dd[0]
        if k == 0:
            pl.plan(oracle.PLAN_FOOTSTEPS, 0, state, l_feet, v_ref)
        pl.plan(oracle.PLAN_TICK, k, state, l_feet, v_ref)
        Ax, l, u = oracle.formulate(pl.xref, pl.fsteps, 1 if k == 0 else 0, prm)
        if p is not None and compensate:
            sft = -(prm.dt * d)
            for kk in range(N):
                l[12 * kk + 6:12 * kk + 12] += sft
                u[12 * kk + 6:12 * kk + 12] += sft
        warm = {} if k == 0 or failed else dict(warm_x=warm_x, warm_y=y, rho=rho)
        r = oracle.qp_solve(N, Ax, l, u, prm, **warm)
        failed = r["status"] not in (1, 2, -2)
        o = oracle.retrieve(N, r["x"], pl.xref, pl.fsteps, pl.gait, q_w, failed, prm, pl.p.shoulders[:])
        warm_x, y, rho = o["warm_x"], r["y"], r["rho"]
        f_prev = r["x"][12 * N:12 * N + 12].copy()
        out["status"].append(r["status"])
        out["state"].append(state.copy())
        out["d"].append(d.copy())
        if failed:
            y, rho = np.zeros(44 * N), prm.rho
            continue
        pt = PM.session_tick(pl.xref[None, :, 0], pl.fsteps[None], pl.gait[None], f_prev[None], q_w[None], wr, consts,
                             dt=prm.dt, gravity=prm.gravity, integrator=integrator, clamp=clamp)
        q_w, state, l_feet = pt["q_w"][0], pt["state"][0], pt["l_feet"][0]
    return {k: np.array(v) if isinstance(v, list) else v for k, v in out.items()}
