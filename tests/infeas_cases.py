"""Infeasible and inaccurate exits shared by test_oracle_infeas.py (CPU) and test_gpu_infeas.py
(GPU): OSQP's primal / dual infeasibility tests deciding the outcome, at one horizon per engine
layout.

MPC.py's QPs are feasible and bounded, so on ordinary inputs with the default eps_prim_inf =
eps_dual_inf = 1e-4 the infeasibility arithmetic of a termination check never decides anything.
Each case here makes it decide: a hand-made contradictory row (a swing foot's friction row asked
for fz >= 10 while its swing row holds the force at 0), the two tolerances moved off their
defaults, max_iter placed so that the 10x-relaxed second look at max_iter reports one of the
inaccurate statuses, and loose tolerances on ordinary feasible batches, where the test fires on
some instances and not on others at iterations spread over the solve -- the outcome then hangs on
the actual values of the reductions.

Every batch has B = 8 instances.  ``CASES[name]`` is a dict:
  entry   "qp" (mpcq_qp_solve_batch on the oracle's formulation) or "fused" (mpcq_solve_batch)
  gaits   the gaits of synth.make_batch(8, N, gaits=gaits, seed=300 + N)
  seeds   (optional) {N: seed} where 300 + N does not meet the case's condition
  where   None, or where the hand-made row goes on the even instances ("first", "mid", "last")
  params  {N: overrides}: the (case, N) pairs of the table; a pair that is absent was dropped,
          with the reason in a comment next to it
``EXPECT[name](N, o, base)`` asserts, from the oracle's result o and its result base on the same
instances under the default parameters, the condition that gives the case its power.  The numbers
in the table were chosen on the CPU so that the conditions hold and so that every status and
iteration count stays the same when the two tolerances are scaled by 1 +- 1e-3
(tests/test_oracle_infeas.py): the GPU differs from the oracle by ~1e-9 relative on these solves,
so no instance here can flip for a rounding difference.
"""
import numpy as np

B = 8

# 7 two waves with a phantom row; 12 exit status from LDS; 16 the explicit-inverse loop; 17 three
# phantom rows, exit status re-derived; 20 sliceable; 32 the largest LDS layout; 33 global
# workspace, phantom rows; 49 thirteen waves; 50 constraint values in the workspace
HORIZONS = (7, 12, 16, 17, 20, 32, 33, 49, 50)

SOLVED, SOLVED_INACC, PINF_INACC, DINF_INACC = 1, 2, 3, 4
MAX_ITER, PINF, DINF = -2, -3, -4
NAN_STATUSES = (PINF, DINF, PINF_INACC, DINF_INACC)   # osqp store_solution: x = y = NaN


def swing_feet(N, fsteps):
    """Per stage k < N, the feet whose fsteps entry is NaN (in swing) at that stage."""
    out, k, i = [], 0, 0
    while k < N and i < fsteps.shape[0] and fsteps[i, 0] > 0:
        feet = [f for f in range(4) if np.isnan(fsteps[i, 1 + 3 * f])]
        for _ in range(int(fsteps[i, 0])):
            if k < N:
                out.append(feet)
                k += 1
        i += 1
    assert k == N, (k, N)
    return out


def infeasible_row(N, fsteps, where):
    """(stage, foot) of the hand-made row: the first stage with a swing foot, the one nearest the
    middle of the horizon, or the last one (stage N - 1 whenever a foot swings there: the stage
    the engine's phantom rows copy).  None when no foot ever swings."""
    sw = swing_feet(N, fsteps)
    ks = [k for k in range(N) if sw[k]]
    if not ks:
        return None
    k = {"first": ks[0], "mid": min(ks, key=lambda j: (abs(j - N // 2), j)), "last": ks[-1]}[where]
    return k, sw[k][0]


def infeasible_instance(N, Ax, l, u, fsteps, where="first"):
    """A copy of (Ax, l, u) with fz >= 10 N demanded of a foot its swing row holds at 0: row 5 of
    the foot's friction block, -fz <= u, at the stage infeasible_row picks.  None without a
    swinging foot."""
    kf = infeasible_row(N, fsteps, where)
    if kf is None:
        return None
    k, f = kf
    Ax, l, u = Ax.copy(), l.copy(), u.copy()
    u[24 * N + 20 * k + 5 * f + 4] = -10.0
    return Ax, l, u


def make_batch(N, name):
    """The case's batch at horizon N: synth.make_batch(8, N, gaits, seed 300 + N unless the case
    names another for that horizon)."""
    from mpcq import synth
    c = CASES[name]
    return synth.make_batch(B, N, gaits=c["gaits"], seed=c.get("seeds", {}).get(N, 300 + N))


def hand_mask():
    """The hand-made rows go on the even instances; the odd ones stay feasible in the same launch."""
    return np.arange(B) % 2 == 0


def make_qp(oracle, N, name, params=None):
    """(Ax, l, u, hand, stages) of a case: the oracle's formulation of the case's batch with the
    hand-made row on the even instances (hand is all-False without one); stages[b] is the stage
    of instance b's row, -1 where it has none."""
    c = CASES[name]
    s = make_batch(N, name)
    p = params if params is not None else oracle.default_params(**c["params"][N])
    hand = hand_mask() if c["where"] else np.zeros(B, bool)
    Ax, l, u, stages = [], [], [], []
    for b in range(B):
        q = oracle.formulate(s["xref"][b], s["fsteps"][b], 0, params=p)
        k = -1
        if hand[b]:
            k = infeasible_row(N, s["fsteps"][b], c["where"])[0]
            q = infeasible_instance(N, *q, s["fsteps"][b], c["where"])
        Ax.append(q[0]), l.append(q[1]), u.append(q[2]), stages.append(k)
    return np.stack(Ax), np.stack(l), np.stack(u), hand, np.array(stages)


def oracle_solve(oracle, N, name, scale=1.0, robots=None, extra=None, base=False):
    """The oracle's result on every instance of (name, N), one qp_solve each on the oracle's own
    formulation (the fused cases too: that is what oracle.solve_batch does, and it yields y and
    rho as well).  scale multiplies the case's eps_prim_inf / eps_dual_inf (the robustness runs);
    robots: a per-instance table (robot_cases.oracle_params); extra: further overrides; base: the
    case's tolerances and max_iter left at their defaults."""
    c = CASES[name]
    ov = dict(c["params"][N], **(extra or {}))
    if base:
        ov = {k: v for k, v in ov.items() if k not in TOL_FIELDS}
    for k in ("eps_prim_inf", "eps_dual_inf"):
        if k in ov:
            ov[k] = ov[k] * scale
    s = make_batch(N, name)
    hand = hand_mask() if c["where"] else np.zeros(B, bool)
    rs, stages = [], []
    for b in range(B):
        if robots is None:
            p = oracle.default_params(**ov)
        else:
            import robot_cases as RC
            p = RC.oracle_params(oracle, robots[b], **ov)
        q = oracle.formulate(s["xref"][b], s["fsteps"][b], 0, params=p)
        if hand[b]:
            q = infeasible_instance(N, *q, s["fsteps"][b], c["where"])
        stages.append(infeasible_row(N, s["fsteps"][b], c["where"])[0] if hand[b] else -1)
        rs.append(oracle.qp_solve(N, *q, params=p))
    out = {k: np.array([r[k] for r in rs]) for k in rs[0]}
    out["f0"] = out["x"][:, 12 * N:12 * N + 12].copy()
    out["hand"], out["stages"] = hand, np.array(stages)
    for v in out.values():
        v.flags.writeable = False
    return out


def _all(ov):
    return {n: dict(ov) for n in HORIZONS}


TROT, MIXED = ("trot",), ("trot", "bound", "pace")

# status 3 wants max_iter inside the window between the 10x-relaxed test's first success and the
# strict one's, for all four hand-made instances at once: up to N = 32 that is 150 / 160 at
# eps_prim_inf = 1e-5 (strict detection at 225); beyond, detection spreads over the instances
# (N = 33: 225, 225, 325, 225) and only eps_prim_inf = 1e-3 leaves a common window, around 100
# (an unchecked max_iter first runs the strict test there, which at N = 33 / 50 succeeds by 110;
# at N = 49 the relaxed test has not yet fired on one instance by 90)
def _pinf_inacc(mi_small, mi_big):
    return {n: (dict(eps_prim_inf=1e-5, max_iter=mi_small) if n <= 32 else
                dict(eps_prim_inf=1e-3, max_iter=mi_big[n])) for n in HORIZONS}


CASES = {
    "hand_first": dict(entry="qp", gaits=TROT, where="first", params=_all({})),
    "hand_mid": dict(entry="qp", gaits=TROT, where="mid", params=_all({})),
    "hand_last": dict(entry="qp", gaits=TROT, where="last", params=_all({})),
    # the default 1e-4 detects at iteration 125 (N <= 33; 125..425 at 49 / 50)
    "epi_tight": dict(entry="qp", gaits=TROT, where="mid", params=_all(dict(eps_prim_inf=1e-7))),
    "epi_loose": dict(entry="qp", gaits=TROT, where="mid", params=_all(dict(eps_prim_inf=1e-2))),
    "pinf_inacc_checked": dict(entry="qp", gaits=TROT, where="mid", params=_pinf_inacc(150, {33: 100, 49: 100, 50: 100})),
    "pinf_inacc_unchecked": dict(entry="qp", gaits=TROT, where="mid", params=_pinf_inacc(160, {33: 90, 49: 110, 50: 90})),
    # max_iter some tens of iterations before most instances converge (both on and off a check)
    "solved_inacc": dict(entry="qp", gaits=TROT, where=None,
                         params={7: dict(max_iter=290), 12: dict(max_iter=520), 16: dict(max_iter=700),
                                 17: dict(max_iter=670), 20: dict(max_iter=800), 32: dict(max_iter=800),
                                 33: dict(max_iter=720), 49: dict(max_iter=550), 50: dict(max_iter=1000)}),
    # N = 7, 12, 20: dropped.  No instance of the trot batch reports -4 for any eps_dual_inf up to
    # 0.95, and from 1.0 on every instance does at the first check (dinf_first): no value gives a
    # later detection next to a solve.  (fused_edi reaches -4 at these horizons on mixed gaits.)
    "dinf": dict(entry="qp", gaits=TROT, where=None,
                 params={16: dict(eps_dual_inf=0.7), 17: dict(eps_dual_inf=0.7), 32: dict(eps_dual_inf=0.9),
                         33: dict(eps_dual_inf=0.7), 49: dict(eps_dual_inf=0.8), 50: dict(eps_dual_inf=0.7)}),
    # (at 49 / 50 stages 1.0 .. 2.0 still leaves some instances to a later check)
    "dinf_first": dict(entry="qp", gaits=TROT, where=None, params=_all(dict(eps_dual_inf=3.0))),
    "dinf_inacc": dict(entry="qp", gaits=TROT, where=None, params=_all(dict(eps_dual_inf=0.3, max_iter=60))),
    # seed 349 gives at most two distinct detection iterations at N = 49 for every eps_prim_inf
    # between 0.028 (nothing fires) and 1.0 (six instances fire at iteration 50 from 0.035 on)
    "fused_epi": dict(entry="fused", gaits=MIXED, where=None, seeds={49: 849},
                      params={7: dict(eps_prim_inf=0.22), 12: dict(eps_prim_inf=0.15), 16: dict(eps_prim_inf=0.1),
                              17: dict(eps_prim_inf=0.1), 20: dict(eps_prim_inf=0.1), 32: dict(eps_prim_inf=0.055),
                              33: dict(eps_prim_inf=0.3), 49: dict(eps_prim_inf=0.033), 50: dict(eps_prim_inf=0.032)}),
    "fused_edi": dict(entry="fused", gaits=MIXED, where=None,
                      params={7: dict(eps_dual_inf=0.95), 12: dict(eps_dual_inf=0.8), 16: dict(eps_dual_inf=0.8),
                              17: dict(eps_dual_inf=0.8), 20: dict(eps_dual_inf=0.9), 32: dict(eps_dual_inf=0.8),
                              33: dict(eps_dual_inf=0.9), 49: dict(eps_dual_inf=0.8), 50: dict(eps_dual_inf=0.8)}),
}

PAIRS = [(name, N) for name, c in CASES.items() for N in HORIZONS if N in c["params"]]


def _hand_all(o, status):
    h = o["hand"]
    assert h.sum() == B // 2
    assert (o["status"][h] == status).all(), o["status"].tolist()


def _neighbours_as_base(o, base):
    """The untouched instances of a hand-made batch end as under the defaults."""
    h = o["hand"]
    assert (base["status"][~h] == SOLVED).all(), base["status"].tolist()
    assert np.array_equal(o["status"][~h], base["status"][~h]) and np.array_equal(o["iters"][~h], base["iters"][~h])


def _expect_hand(N, o, base):
    """Every hand-made instance ends -3 at a termination check; its neighbours solve."""
    _hand_all(o, PINF)
    assert (o["iters"][o["hand"]] % 25 == 0).all() and (o["iters"][o["hand"]] < 4000).all()
    _neighbours_as_base(o, base)


def _expect_hand_last(N, o, base):
    """... and off a multiple of 4 at least one row sits on stage N - 1, which the phantom rows copy."""
    _expect_hand(N, o, base)
    if N % 4:
        assert (o["stages"][o["hand"]] == N - 1).any(), o["stages"].tolist()


def _expect_epi(side):
    def f(N, o, base):
        """Every hand-made instance is detected strictly later (tight) / earlier (loose) than at 1e-4."""
        _expect_hand(N, o, base)
        _hand_all(base, PINF)
        h = o["hand"]
        assert (side * (o["iters"][h] - base["iters"][h]) > 0).all(), (o["iters"].tolist(), base["iters"].tolist())
    return f


def _expect_pinf_inacc(N, o, base):
    """Every hand-made instance ends 3 at max_iter; the others reach max_iter unsolved."""
    _hand_all(o, PINF_INACC)
    assert (o["status"][~o["hand"]] == MAX_ITER).all(), o["status"].tolist()
    assert (o["iters"] == o["iters"][0]).all()


def _expect_solved_inacc(N, o, base):
    """At least three instances end 2 at max_iter; the rest are solved or plainly out of iterations."""
    assert (base["status"] == SOLVED).sum() >= B - 1, base["status"].tolist()
    assert (o["status"] == SOLVED_INACC).sum() >= 3, o["status"].tolist()
    assert np.isin(o["status"], (SOLVED, SOLVED_INACC, MAX_ITER)).all(), o["status"].tolist()


def _expect_dinf(N, o, base):
    """At least one instance ends -4 at a check after the first while at least one other solves."""
    late = (o["status"] == DINF) & (o["iters"] > 25)
    assert late.any() and (o["status"] == SOLVED).any(), (o["status"].tolist(), o["iters"].tolist())
    assert np.isin(o["status"], (SOLVED, SOLVED_INACC, DINF)).all()


def _expect_dinf_first(N, o, base):
    """Every instance ends -4 at the first check."""
    assert (o["status"] == DINF).all() and (o["iters"] == 25).all(), (o["status"].tolist(), o["iters"].tolist())


def _expect_dinf_inacc(N, o, base):
    """Every instance ends 4 at max_iter."""
    assert (o["status"] == DINF_INACC).all() and (o["iters"] == 60).all(), (o["status"].tolist(), o["iters"].tolist())


def _expect_fused(status, n_min, n_iters):
    def f(N, o, base):
        """At least n_min of 8 end with the status, at least one is SOLVED, and the detections
        fall on at least n_iters distinct iterations."""
        hit = o["status"] == status
        assert hit.sum() >= n_min and (o["status"] == SOLVED).any(), o["status"].tolist()
        assert len(set(o["iters"][hit].tolist())) >= n_iters, o["iters"].tolist()
        assert np.isin(base["status"], (SOLVED, SOLVED_INACC)).all()   # feasible: only the tolerance does it
    return f


EXPECT = {
    "hand_first": _expect_hand, "hand_mid": _expect_hand, "hand_last": _expect_hand_last,
    "epi_tight": _expect_epi(+1), "epi_loose": _expect_epi(-1),
    "pinf_inacc_checked": _expect_pinf_inacc, "pinf_inacc_unchecked": _expect_pinf_inacc,
    "solved_inacc": _expect_solved_inacc,
    "dinf": _expect_dinf, "dinf_first": _expect_dinf_first, "dinf_inacc": _expect_dinf_inacc,
    "fused_epi": _expect_fused(PINF, 3, 3), "fused_edi": _expect_fused(DINF, 2, 2),
}

TOL_FIELDS = ("eps_prim_inf", "eps_dual_inf", "max_iter")


def base_solve(oracle, N, name):
    """The oracle on the case's instances with the case's tolerances and max_iter at their defaults."""
    return oracle_solve(oracle, N, name, base=True)


# ---------------------------------------------------------------------------- sessions
# Six robots, five host-fed ticks on test_gpu_session.py's inputs under a loose eps_prim_inf: some
# robots fail with -3 on a tick, restart cold and solve on a later one.  (0.1 at N = 20 changes an
# iteration count when scaled by 0.999; 0.15 does not.)
SESSION_B, SESSION_T = 6, 5
SESSION_EPI = {16: 0.1, 20: 0.15}


def session_gaits(N):
    from mpcq import synth
    return np.stack([synth.gait_table(("trot", "bound", "pace")[b % 3], N) for b in range(SESSION_B)])


def session_inputs(N):
    """Per tick (k, state, l_feet, v_ref, reduced): test_gpu_session.py's _inputs on its generator."""
    from test_gpu_session import _inputs
    rng = np.random.default_rng(11 + N)
    for k in range(SESSION_T):
        state, l_feet, v_ref = _inputs(rng, SESSION_B, k)
        yield k, state, l_feet, v_ref, (np.arange(SESSION_B) % 5 == 0).astype(np.int32)


def oracle_sessions(oracle, N, scale=1.0):
    gaits = session_gaits(N)
    return [oracle.Session(N, gaits[b], params=oracle.default_params(eps_prim_inf=SESSION_EPI[N] * scale))
            for b in range(SESSION_B)]


def oracle_session_run(oracle, N, scale=1.0):
    """(status, iters), each (T, B), of the oracle's sessions."""
    ors = oracle_sessions(oracle, N, scale)
    st, it = [], []
    for k, state, l_feet, v_ref, red in session_inputs(N):
        for b, o in enumerate(ors):
            o.tick(k, v_ref[b], state=state[b], l_feet=l_feet[b], reduced=bool(red[b]))
        st.append([o.status for o in ors])
        it.append([o.iters for o in ors])
    return np.array(st), np.array(it)


def expect_session(status):
    """At least one robot fails on a tick and solves on a later one, and on at least one tick
    failed and solved robots coexist."""
    failed, ok = np.isin(status, NAN_STATUSES), status == SOLVED
    assert np.isin(status, NAN_STATUSES + (SOLVED, SOLVED_INACC)).all(), status.tolist()
    assert any(failed[k, b] and ok[k + 1:, b].any() for k in range(status.shape[0]) for b in range(status.shape[1]))
    assert (failed.any(axis=1) & ok.any(axis=1)).any()
