"""Inputs of the monitor's batch test (tests/test_gpu_monitor.py), and the worst-case push
computation of its session tests; both need no device, so their properties are checked on the
CPU too (tests/test_monitor_model.py)."""
import numpy as np

import monitor_model as MM
import plant_model as PM

STATUSES = (1, 2, 3, 4, -2, -3, -4, -10, -11, -12, -13)  # every MPCQ_STATUS_* value
PARAMS = dict(max_tilt=0.5, min_height=0.1, max_ticks=2)
CALLS = 3


def exact_robots(B):
    """The robots that sit exactly at the roll, pitch and height thresholds in every call."""
    return 0, 1 % B, 2 % B


def batch_calls(B, seed):
    """CALLS consecutive ticks of made-up inputs for B robots: poses around the thresholds,
    every status value, NaN and infinite entries; the robots of exact_robots(B) solved, benign
    but for sitting exactly at a threshold."""
    rng = np.random.default_rng(seed)
    out = []
    i_r, i_p, i_z = exact_robots(B)
    for c in range(CALLS):
        q_w = np.empty((B, 6))
        q_w[:, 0:2] = rng.uniform(-2.0, 2.0, (B, 2))
        q_w[:, 2] = rng.uniform(0.08, 0.3, B)
        q_w[:, 3:5] = rng.uniform(-0.55, 0.55, (B, 2))
        q_w[:, 5] = rng.uniform(-np.pi, np.pi, B)
        p = np.full(len(STATUSES), 0.4 / (len(STATUSES) - 1))
        p[0] = 0.6
        status = rng.choice(np.array(STATUSES, np.int32), B, p=p).astype(np.int32)
        iters = rng.integers(0, 4001, B).astype(np.int32)
        f0 = rng.uniform(-10.0, 25.0, (B, 12))
        cost = rng.uniform(0.0, 50.0, (B, 13))
        state = rng.uniform(-1.0, 1.0, (B, 12))
        v_ref = rng.uniform(-0.5, 0.5, (B, 6))
        failed = ~np.isin(status, MM.OK_STATUS) & (rng.random(B) < 0.5)
        f0[failed] = np.nan  # what an infeasible exit leaves
        cost[failed] = np.nan
        if B >= 16:
            q_w[(5 + c) % B, c % 6] = np.nan
            q_w[(7 + c) % B, 3] = np.inf
            q_w[(9 + c) % B, 2] = -np.inf
            q_w[(11 + c) % B, 4] = -np.inf
            state[(13 + c) % B, 6] = np.nan  # a NaN that stays in the robot's accumulator
        for i in {i_r, i_p, i_z}:
            q_w[i, 2:5] = [0.2, 0.1, -0.1]
            status[i] = 1
            f0[i] = rng.uniform(0.0, 10.0, 12)
            cost[i] = rng.uniform(0.0, 5.0, 13)
        q_w[i_r, 3] = PARAMS["max_tilt"]
        q_w[i_p, 4] = -PARAMS["max_tilt"]
        q_w[i_z, 2] = PARAMS["min_height"]
        out.append(dict(q_w=q_w, status=status, iters=iters, f0=f0, cost=cost, state=state, v_ref=v_ref))
    return out


def model_calls(calls, B):
    """The model over those calls: [(done, trace, the accumulators after the call)]."""
    acc = MM.new_state(B)
    out = []
    for c in calls:
        done, trace = MM.step(acc=acc, **c, **PARAMS)
        out.append((done, trace, MM.copy_state(acc)))
    return out


# ---------------------------------------------------------------- the session tests' pushes
H_REF = 0.2027682
DOWN_FORCE = 250.0   # N, along -z
ROLL_TORQUE = 25.0   # N m, about +x


def worst_case(kind, ticks=4):
    """Where a standing robot is after `ticks` ticks of the push if every foot is in stance and
    resists with all the plant's clamp lets through: against the downward force every foot
    pushes up with fz_max; against the roll torque the feet on the side going down (y < 0) push
    up with fz_max and the others not at all.  Returns (z, |roll|) after each tick."""
    x = np.zeros((1, 12))
    x[0, 2] = H_REF
    feet = np.vstack([PM.SHOULDERS, np.zeros((1, 4))])[None]
    f = np.zeros((1, 4, 3))
    w = np.zeros((1, 6))
    if kind == "height":
        f[0, :, 2] = PM.FZ_MAX
        w[0, 2] = -DOWN_FORCE
    else:
        f[0, PM.SHOULDERS[1] < 0, 2] = PM.FZ_MAX
        w[0, 3] = ROLL_TORQUE
    out = []
    for _ in range(ticks):
        x, _ = PM.step(x, feet, f.reshape(1, 12), w)
        out.append((float(x[0, 2]), float(abs(x[0, 3]))))
    return out
