"""Shared cases of the gait tests (CPU model tests and the GPU tests): the cycles, random
tables and state rows for the batch entry point, the trot -> bound -> stand -> trot schedule
and the closed loop composed from the oracle's pieces with the model's roll in the planner's
place."""
import functools

import numpy as np

import gait_model as GM

MASKS = {"trot": ((1, 1, 1, 1), (1, 0, 0, 1), (1, 1, 1, 1), (0, 1, 1, 0)),
         "bound": ((1, 1, 1, 1), (1, 1, 0, 0), (1, 1, 1, 1), (0, 0, 1, 1)),
         "pace": ((1, 1, 1, 1), (1, 0, 1, 0), (1, 1, 1, 1), (0, 1, 0, 1))}


def cycle(name, half=8):
    """One period [1 all][half - 1 A][1 all][half - 1 B]; "stand": the one-row cycle."""
    g = np.zeros((20, 5))
    if name == "stand":
        g[0] = 1.0
        return g
    g[:4, 0] = (1, half - 1, 1, half - 1)
    g[:4, 1:] = MASKS[name]
    return g


def table(name, N, half=8):
    """The table a planner runs at horizon N: N / (2 half) periods of the cycle."""
    g = np.zeros((20, 5))
    if name == "stand":
        g[0] = (N, 1, 1, 1, 1)
        return g
    n = N // (2 * half)
    assert n * 2 * half == N and 4 * n <= 19
    for i in range(n):
        g[4 * i:4 * i + 4] = cycle(name, half)[:4]
    return g


LIB = np.stack([cycle("trot"), cycle("bound"), cycle("stand"), cycle("pace")])  # ids 0..3
TROT, BOUND, STAND, PACE = range(4)


# ---------------------------------------------------------------- the batch entry point
def random_tables(rng, B, N=16):
    """(gait (B, 20, 5), state (B, 4) int32): tables among periodic ones at a random phase of
    their period, single-row tables, tables with 18 and 19 rows in use, tables with no zero row;
    state rows valid or with out-of-range want / active / phase."""
    gait = np.zeros((B, 20, 5))
    state = GM.new_state(B)
    plain = GM.params(n_gaits=1)
    for b in range(B):
        kind = int(rng.integers(0, 8))
        if kind < 4:  # a periodic table, rolled by the reference's rule to some phase
            g = table(("trot", "bound", "pace", "stand")[kind], N)
            st = GM.new_state(1)[0]
            for _ in range(int(rng.integers(0, 17))):
                GM.roll_one(plain, LIB[:1], None, g, st)
        elif kind == 4:  # a single row
            g = np.zeros((20, 5))
            g[0] = (N, *rng.integers(0, 2, 4))
        elif kind in (5, 6):  # 18 or 19 rows in use: alternating contacts, counts of 1 and 2
            rows = 18 if kind == 5 else 19
            g = np.zeros((20, 5))
            for r in range(rows):
                g[r] = (1 + int(rng.integers(0, 2)), r % 2, 1, (r + 1) % 2, 1)
        else:  # no zero row: must come back untouched
            g = np.zeros((20, 5))
            for r in range(20):
                g[r] = (1 + int(rng.integers(0, 3)), r % 2, 1, (r + 1) % 2, 1)
        gait[b] = g
        mode = int(rng.integers(0, 4))
        if mode == 1:  # a running gait with a request
            state[b] = (int(rng.integers(-1, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 16)), int(rng.integers(0, 9)))
        elif mode == 2:  # a request only
            state[b] = (int(rng.integers(0, 4)), -1, 0, 0)
        elif mode == 3:  # out of range: the defensive reads
            state[b] = (int(rng.choice([-7, -2, 4, 8, 99, 2 ** 31 - 1])), int(rng.choice([-9, -2, 4, 7, 1000, -2 ** 31])),
                        int(rng.choice([-1, -17, 16, 1217, 2 ** 31 - 1, -2 ** 31])), int(rng.integers(-3, 3)))
    return gait, state


THRESHOLDS = (0.25, 0.5, 1.0)  # stand < 0.25 <= trot < 0.5 <= bound < 1.0 <= pace, with SPEED_LIB
SPEED_LIB = np.stack([cycle("stand"), cycle("trot"), cycle("bound"), cycle("pace")])
HYSTERESIS = 0.0625


def speed_vrefs(rng, B):
    """v_ref (B, 6) on, just above and just below the thresholds and the hysteresis edges (all
    exactly representable: vy = wz = 0 makes s = |vx|), some with yaw, a NaN and an inf."""
    edges = [t + d for t in THRESHOLDS for d in (0.0, HYSTERESIS, -HYSTERESIS)]
    pts = [np.nextafter(e, s) for e in edges for s in (-np.inf, np.inf)] + edges + [0.0, 2.0]
    v = np.zeros((B, 6))
    v[:, 0] = rng.choice(pts, B) * rng.choice([-1.0, 1.0], B)
    yaw = rng.random(B) < 0.25
    v[yaw, 5] = rng.uniform(-2.0, 2.0, int(yaw.sum()))
    v[yaw, 1] = rng.uniform(-0.3, 0.3, int(yaw.sum()))
    if B > 2:
        v[int(rng.integers(0, B)), 0] = np.nan
        v[int(rng.integers(0, B)), 5] = np.inf
    return v


# ---------------------------------------------------------------- the schedule
SCHEDULE = ((3, BOUND), (30, STAND), (55, TROT), (58, BOUND))  # (tick the request is made before, id)
SCHEDULE_TICKS = 70


def requests(B, never=None, stagger=2):
    """{tick: ids (B,) int32 with -2 = leave this robot's want alone}: robot b makes SCHEDULE's
    requests `stagger * b` ticks late; robot `never` makes none."""
    out = {}
    for b in range(B):
        if b == never:
            continue
        for t, g in SCHEDULE:
            t += stagger * b
            if t < SCHEDULE_TICKS:
                out.setdefault(t, np.full(B, -2, np.int32))[b] = g
    return out


def apply_requests(state, ids):
    """set_gait on the model's rows: want <- ids where ids != -2."""
    m = ids != -2
    state[m, 0] = ids[m]


def model_run(gait0, lib, p, ticks, reqs=None, v_ref=None):
    """The tables and rows after every tick: (ticks, B, 20, 5), (ticks, B, 4)."""
    gait, state = gait0.copy(), GM.new_state(gait0.shape[0])
    gs, ss = [], []
    for t in range(ticks):
        if reqs and t in reqs:
            apply_requests(state, reqs[t])
        GM.roll(p, lib, None if v_ref is None else v_ref[t], gait, state)
        gs.append(gait.copy())
        ss.append(state.copy())
    return np.stack(gs), np.stack(ss)


# ---------------------------------------------------------------- the composed closed loop
def oracle_tick(O, o, k, v_ref, p, lib, st):
    """oracle.Session.tick (virtual robot) with the gait model's roll in the planner's place:
    plan(FOOTSTEPS) on tick 0, the model's roll, plan(FOOTSTEPS | REFSTATES), then formulate /
    qp_solve / retrieve as oracle.Session.tick does."""
    s, lf = o.state, o.l_feet
    pst = 0
    if k == 0:
        pst = o.planner.plan(O.PLAN_FOOTSTEPS, 0, s, lf, v_ref)
    GM.roll_one(p, lib, v_ref, o.planner.gait, st)
    pst = o.planner.plan(O.PLAN_FOOTSTEPS | O.PLAN_REFSTATES, k, s, lf, v_ref) or pst
    N = o.N
    Ax, l, u = O.formulate(o.planner.xref, o.planner.fsteps, 1 if k == 0 else 0, o.p)
    if k == 0:
        r = O.qp_solve(N, Ax, l, u, o.p)
    else:
        r = O.qp_solve(N, Ax, l, u, o.p, warm_x=o.warm_x, warm_y=o.y, rho=o.rho)
    o.x, o.y, o.rho = r["x"], r["y"], r["rho"]
    o.status, o.iters = r["status"], r["iters"]
    failed = o.status not in (1, 2, -2) or pst != 0
    out = O.retrieve(N, o.x, o.planner.xref, o.planner.fsteps, o.planner.gait, o.q_w, failed, o.p,
                     o.planner.p.shoulders[:])
    o.x_robot, o.cost, o.warm_x = out["x_robot"], out["cost"], out["warm_x"]
    if failed:
        o.y = np.zeros(44 * N)
        o.rho = o.p.rho
    else:
        o.q_w = out["q_w"]
        o.state, o.l_feet = out["state"], out["l_feet"]
    if pst:
        o.status = pst
    o.f0 = o.x[12 * N:12 * N + 12]
    return o.status


CLOSED_V_REF = np.array([0.3, 0.0, 0.0, 0.0, 0.0, 0.1])


@functools.lru_cache(maxsize=None)
def closed_loop(B=5, never=4, N=16):
    """The schedule in closed loop on the oracle, robot by robot, once: per tick and robot the
    status, iteration count, f0, x, table and state row."""
    from oracle import oracle as O
    O.build()
    p = GM.params(n_gaits=3)
    lib = LIB[:3]
    reqs = requests(B, never)
    ors = [O.Session(N, table("trot", N)) for _ in range(B)]
    state = GM.new_state(B)
    rec = dict(status=[], iters=[], f0=[], x=[], gait=[], state=[])
    for k in range(SCHEDULE_TICKS):
        if k in reqs:
            apply_requests(state, reqs[k])
        for b, o in enumerate(ors):
            oracle_tick(O, o, k, CLOSED_V_REF, p, lib, state[b])
        rec["status"].append([o.status for o in ors])
        rec["iters"].append([o.iters for o in ors])
        rec["f0"].append(np.stack([o.f0 for o in ors]))
        rec["x"].append(np.stack([o.x for o in ors]))
        rec["gait"].append(np.stack([o.planner.gait for o in ors]))
        rec["state"].append(state.copy())
    return {k: np.array(v) for k, v in rec.items()}
