"""Host model of the swing-foot kernels (mpc-tsid_amd/csrc/mpcq_swing.hip), in numpy.

A restatement of what mpcq_swing_step_batch / mpcq_swing_batch compute per (robot, foot):

  next_foot   Foot_trajectory_generator.get_next_foot (FootTrajectoryGenerator.py:222-380) on
              the 40-double state of include/mpcq.h; the polynomials use products where the
              reference calls pow(), so they are held to a tolerance, not to bits
  timing      the scalar chain of update_feet_tasks (TSID:260-282): the first stance row, the
              cumulative durations, t_swing with Python's negative indexing, in the
              reference's operation order (its decisions are exact)
  advance     update_footsteps + update_feet_tasks over substeps, plus the rules the
              reference does not define: stance feet are NaN, the last world (x, y) kept in
              slots 35/36, lift-off from there when feet0 is None, BAD_GAIT

The fixtures (tests/golden/swing_golden.npz) pin this model to the reference
(tests/test_swing_model.py); the GPU tests use it where the reference has no counterpart.
"""
import os

import numpy as np

# Tolerance rule of the swing tests: per class of quantity (positions, velocities,
# accelerations, coefficients -- the last relative to each coefficient slot's largest
# magnitude over the step cases) the yardstick is the reference's own rounding error on the
# fixture set, max |float64 - longdouble| as stored by gen_swing_golden.py (step_err,
# free_err); the bound is TOL_FACTOR times it.  The kernel evaluates the same ill-conditioned
# sums in the same precision in another order, so its error is of that size; the factor
# covers the error compounding through the fed-back state over a swing.
TOL_FACTOR = 16.0


def load_golden():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swing_golden.npz"))
    return {k: d[k] for k in d.files}


def error_ratios(got, want, yard):
    """max |got - want| over yard, per class, of outputs laid out [..., 9] = pos xyz, vel xyz,
    acc xyz (NaN where both are NaN)."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    d = np.abs(np.nan_to_num(got - want))
    return np.array([d[..., 0:3].max(), d[..., 3:6].max(), d[..., 6:9].max()]) / yard


def step_ratios(out, post, g):
    """The four ratios (positions, velocities, accelerations, coefficients) of step outputs
    [n][11] and post-state coefficients [n][24] against the fixture's float64 reference."""
    n = len(out)  # the first n cases
    d = np.abs(out - g["step_out"][:n])
    ce = (np.abs(post - g["step_post"][:n, :24]) / g["step_coef_scale"]).max()
    return np.array([d[:, [0, 3, 6]].max(), d[:, [1, 4, 7]].max(), d[:, [2, 5, 8]].max(), ce]) / g["step_err"]


STATE = 40
BAD_GAIT = -11
DEFAULTS = dict(dt=0.001, max_height=0.05, t_lock=0.05, feet_z=0.0, k_mpc=20)


def _axis_coeffs(a, b, den, p, v, acc):
    a2, a3, a4 = a * a, a * a * a, (a * a) * (a * a)
    b2, b3, b4 = b * b, b * b * b, (b * b) * (b * b)
    b5 = b4 * b
    d5 = (acc * a2 - 2 * acc * a * b - 6 * v * a + acc * b2 + 6 * v * b + 12 * p) / den
    d4 = (-30 * a * p - 30 * b * p - 2 * a3 * acc - 3 * b3 * acc + 14 * a2 * v - 16 * b2 * v + 2 * a * b * v
          + 4 * a * b2 * acc + a2 * b * acc) / den
    d3 = (a4 * acc + 3 * b4 * acc - 8 * a3 * v + 12 * b3 * v + 20 * a2 * p + 20 * b2 * p + 80 * a * b * p
          + 4 * a3 * b * acc + 28 * a * b2 * v - 32 * a2 * b * v - 8 * a2 * b2 * acc) / den
    d2 = -(b5 * acc + 4 * a * b4 * acc + 3 * a4 * b * acc + 36 * a * b3 * v - 24 * a3 * b * v + 60 * a * b2 * p
           + 60 * a2 * b * p - 8 * a2 * b3 * acc - 12 * a2 * b2 * v) / den
    d1 = -(2 * b5 * v - 2 * a * b5 * acc - 10 * a * b4 * v + a2 * b4 * acc + 4 * a3 * b3 * acc
           - 3 * a4 * b2 * acc - 16 * a2 * b3 * v + 24 * a3 * b2 * v - 60 * a2 * b2 * p) / den
    d0 = (-acc * a4 * b3 + 2 * acc * a3 * b4 + 8 * v * a3 * b3 - acc * a2 * b5 - 10 * v * a2 * b4
          - 20 * p * a2 * b3 + 2 * v * a * b5 + 10 * p * a * b4 - 2 * p * b5) / den
    return [d5, d4, d3, d2, d1, d0]


def _axis_eval(c, d, x1, e):
    e2, e3, e4 = e * e, e * e * e, (e * e) * (e * e)
    e5 = e4 * e
    c5, c4, c3, c2, c1, c0 = c
    d5, d4, d3, d2, d1, d0 = d
    p = x1 * (c0 + c1 * e + c2 * e2 + c3 * e3 + c4 * e4 + c5 * e5) + d0 + d1 * e + d2 * e2 + d3 * e3 + d4 * e4 + d5 * e5
    v = x1 * (c1 + 2 * c2 * e + 3 * c3 * e2 + 4 * c4 * e3 + 5 * c5 * e4) + d1 + 2 * d2 * e + 3 * d3 * e2 + 4 * d4 * e3 + 5 * d5 * e4
    a = x1 * (2 * c2 + 6 * c3 * e + 12 * c4 * e2 + 20 * c5 * e3) + 2 * d2 + 6 * d3 * e + 12 * d4 * e2 + 20 * d5 * e3
    return p, v, a


def next_foot(st, x0, dx0, ddx0, y0, dy0, ddy0, x1, y1, t0, t1, dt, h, t_lock):
    """get_next_foot on the state ``st`` (40 doubles, updated in place); returns the 11 outputs."""
    adaptive = (t1 - t0) > t_lock
    if adaptive:
        a, b = t0, t1
        den = 2 * (a - b) ** 2 * (a * a * a - 3 * (a * a) * b + 3 * a * (b * b) - b * b * b)
        c = [(-12) / den, (30 * a + 30 * b) / den, (-20 * a * a - 20 * b * b - 80 * a * b) / den,
             -(-60 * a * (b * b) - 60 * (a * a) * b) / den, -(60 * (a * a) * (b * b)) / den,
             (20 * (a * a * a) * (b * b) + 2 * ((a * a) * (a * a) * a) - 10 * ((a * a) * (a * a)) * b) / den]
        st[0:6] = c
        st[12:18] = c
        st[6:12] = _axis_coeffs(a, b, den, x0, dx0, ddx0)
        st[18:24] = _axis_coeffs(a, b, den, y0, dy0, ddy0)
        st[24], st[25] = x1, y1
    st[34] = 1.0 if adaptive else 0.0
    zd = (t1 / 2) ** 3 * (t1 - t1 / 2) ** 3
    Az6, Az5, Az4, Az3 = -h / zd, (3 * t1 * h) / zd, -(3 * t1 * t1 * h) / zd, (t1 * t1 * t1 * h) / zd
    e = t0 + dt
    px, vx, ax = _axis_eval(st[0:6], st[6:12], st[24], e)
    py, vy, ay = _axis_eval(st[12:18], st[18:24], st[25], e)
    z = Az3 * e ** 3 + Az4 * e ** 4 + Az5 * e ** 5 + Az6 * e ** 6
    dz = 3 * Az3 * e ** 2 + 4 * Az4 * e ** 3 + 5 * Az5 * e ** 4 + 6 * Az6 * e ** 5
    ddz = 6 * Az3 * e + 12 * Az4 * e ** 2 + 20 * Az5 * e ** 3 + 30 * Az6 * e ** 4
    return np.array([px, vx, ax, py, vy, ay, z, dz, ddz, st[24], st[25]])


def timing(gait, f, dt, k_mpc):
    """Of swing foot ``f`` (gait[0][1+f] == 0): (bad, cumulative durations up to the next stance
    row, t_swing).  bad: no stance row anywhere in the column (the reference's forward walk
    leaves the table: IndexError)."""
    col = gait[:, 1 + f]
    if np.all(col == 0):
        return True, 0.0, 0.0
    ones = np.flatnonzero(col == 1)
    index = int(ones[0]) if len(ones) else -1
    cs = np.float64(np.cumsum(gait[:index, 0])[-1])
    ts = np.float64(gait[0, 0])
    i = 1
    while col[i] == 0:
        ts = ts + gait[i, 0]
        i += 1
    i = -1
    while col[i] == 0:  # Python's negative indexing: rows 19, 18, ... over the blank rows
        ts = ts + gait[i, 0]
        i -= 1
    ts = ts * (dt * k_mpc)
    return False, cs, ts


def t0_of(cs, ts, k_sub, dt, k_mpc):
    remaining = cs * k_mpc - k_sub
    return np.round(ts - remaining * dt, decimals=3)


def target_row(fsteps, f):
    for i in range(20):
        v = fsteps[i, 3 * f + 1]
        if not (v == 0) and not np.isnan(v):
            return i
    return 19


def to_world(frame, px, py):
    c, s = np.cos(frame[2]), np.sin(frame[2])
    return (c * px - s * py) + frame[0], (s * px + c * py) + frame[1]


def advance_one(p, gait, fsteps, frame, feet0, state, k_sub0, n_sub):
    """One robot: returns (ref [n_sub][4][9], t0 [n_sub][4], status); ``state`` [4][40] in place."""
    ref = np.full((n_sub, 4, 9), np.nan, state.dtype)
    t0s = np.full((n_sub, 4), np.nan)
    swing = [gait[0, 1 + f] == 0 for f in range(4)]
    tim = [timing(gait, f, p["dt"], p["k_mpc"]) if swing[f] else None for f in range(4)]
    if any(t is not None and t[0] for t in tim):
        return ref, t0s, BAD_GAIT
    for f in range(4):
        st = state[f]
        row = target_row(fsteps, f)
        tx, ty = to_world(frame, fsteps[row, 3 * f + 1], fsteps[row, 3 * f + 2])
        qx, qy = fsteps[0, 3 * f + 1], fsteps[0, 3 * f + 2]
        for k in range(n_sub):
            if swing[f]:
                _, cs, ts = tim[f]
                t0 = t0_of(cs, ts, k_sub0 + k, p["dt"], p["k_mpc"])
                if t0 == 0:
                    start = feet0[f] if feet0 is not None else (st[35], 0.0, 0.0, st[36], 0.0, 0.0)
                else:
                    start = st[26:32].copy()
                g = next_foot(st, *start, tx, ty, t0, ts, p["dt"], p["max_height"], p["t_lock"])
                st[26:32] = g[0:6]
                st[32], st[33] = ts, t0
                ref[k, f] = (g[0], g[3], g[6] + p["feet_z"], g[1], g[4], g[7], g[2], g[5], g[8])
                t0s[k, f] = t0
                st[35], st[36] = g[0], g[3]
            elif not (np.isnan(qx) or np.isnan(qy)):
                st[35], st[36] = to_world(frame, qx, qy)
    return ref, t0s, 0


def advance(gait, fsteps, frame, state, k_sub0=0, n_sub=None, feet0=None, params=None):
    """A batch: gait [B][20][5], fsteps [B][20][13], frame [B][3], state [B][4][40] (in place),
    feet0 [B][4][6] or None.  Returns ref [B][n_sub][4][9], t0 [B][n_sub][4], status [B].
    With fsteps, frame and state (and feet0) in np.longdouble the polynomials are evaluated in
    that precision on the float64 run's branches (gait, the timing chain and t0 stay float64):
    max |float64 - longdouble| is the model's own rounding error, the yardstick where no
    fixture of the reference exists."""
    p = dict(DEFAULTS, **(params or {}))
    n = p["k_mpc"] - k_sub0 if n_sub is None else n_sub
    B = gait.shape[0]
    ref = np.empty((B, n, 4, 9), state.dtype)
    t0 = np.empty((B, n, 4))
    status = np.zeros(B, np.int32)
    for b in range(B):
        keep = state[b].copy()
        ref[b], t0[b], status[b] = advance_one(p, gait[b], fsteps[b], frame[b], None if feet0 is None else feet0[b],
                                               state[b], k_sub0, n)
        if status[b]:
            state[b] = keep
    return ref, t0, status


def step(args, state, params=None):
    """mpcq_swing_step_batch: args [B][4][10], state [B][4][40] in place; returns [B][4][11]."""
    p = dict(DEFAULTS, **(params or {}))
    B = args.shape[0]
    out = np.full((B, 4, 11), np.nan)
    for b in range(B):
        for f in range(4):
            a = args[b, f]
            if np.isnan(a[8]):
                continue
            out[b, f] = next_foot(state[b, f], *a, p["dt"], p["max_height"], p["t_lock"])
    return out
