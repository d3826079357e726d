"""Non-default mpcq_swing_params: the cases of the swing parameter tests.

One dict of overrides per case; the same kwargs go to ``mpcq.default_swing_params(**ov)``, to
``swing_model.advance(..., params=ov)`` and to ``tests/golden/gen_swing_golden.py params``,
which captures the unmodified reference under each case into
``tests/golden/swing_params_golden.npz``.  Five cases move one field each, ``all`` moves all
five.  ``k30`` makes 30 substeps per call (seven full 4-substep output chunks of the kernel and
a partial one), ``all`` 7 (one full chunk and a partial one; a [B][7] stride differs from
[B][20] at every robot but the first).
"""
import os

import numpy as np

FIELDS = ("dt", "max_height", "t_lock", "feet_z", "k_mpc")  # the order of <case>_params
DEFAULTS = dict(dt=0.001, max_height=0.05, t_lock=0.05, feet_z=0.0, k_mpc=20)

CASES = {
    "dt2ms": dict(dt=0.002),
    "k30": dict(k_mpc=30),
    "h8cm": dict(max_height=0.08),
    "lock20ms": dict(t_lock=0.02),
    "feetz": dict(feet_z=0.017),
    "all": dict(dt=0.002, k_mpc=7, max_height=0.03, t_lock=0.01, feet_z=-0.25),
}
NAMES = tuple(CASES)

# free-running fixtures per case: (scenario, variant); 10 ticks of the case's k_mpc substeps
FREE = (("trot", "sub"), ("trot", "tick"), ("bound", "tick"))
TICKS = 10


# Closed-loop sessions with swing enabled (test_session_swing_under_params): B virtual robots in
# mixed trot / bound / pace for SESSION_TICKS ticks.  "n8" is the reference's other time base
# (FootstepPlanner(0.04, 1), N = 8: 40 substeps of 1 ms per tick), as in the N = 8 planner fixtures.
SESSION_B, SESSION_TICKS, SESSION_BAD = 17, 6, 9
SESSIONS = {
    "n16": dict(N=16, dt=0.02, swing=CASES["all"]),
    "n8": dict(N=8, dt=0.04, swing=dict(dt=0.001, k_mpc=40, max_height=0.08, t_lock=0.03, feet_z=0.017)),
}


SESSION_PHASES = (15, 7, 12, 4)  # sixteenths of a period


def session_gaits(N, B=SESSION_B):
    """Robot b walks (trot, bound, pace)[b % 3], each triple from another phase of the period:
    two that stand on all four feet in the first tick and then lift one pair each, two that
    begin in the middle of a swing, lock, stand and lift the other pair.  Within SESSION_TICKS
    ticks the session so meets both modes, stance feet and lift-offs from where a foot stood."""
    from mpcq import synth
    per = synth.period_steps(N)
    return np.stack([synth.rolled_table(synth.GAITS[b % 3], N, SESSION_PHASES[(b // 3) % 4] * per // 16)
                     for b in range(B)])


def session_swing_inputs(name):
    """The oracle's closed loop (CPU) on the robots of session ``name``: per tick the (gait,
    fsteps, frame) the swing launch of that tick reads."""
    from oracle import oracle as O
    c = SESSIONS[name]
    gaits, v_ref = session_gaits(c["N"]), session_v_ref()
    ors = [O.Session(c["N"], gaits[b], params=O.default_params(dt=c["dt"]),
                     planner_params=O.default_planner_params(dt=c["dt"])) for b in range(SESSION_B)]
    out = []
    for k in range(SESSION_TICKS):
        frame = np.stack([o.q_w[[0, 1, 5]] for o in ors])  # q_w before the tick moves it
        for b, o in enumerate(ors):
            o.tick(k, v_ref[b])
        out.append((np.stack([o.planner.gait for o in ors]), np.stack([o.planner.fsteps for o in ors]), frame))
    return out


# The model's own rounding error (positions, velocities, accelerations) on the n8 session's
# inputs, max |float64 - longdouble| over session_swing_inputs("n8") (measured 1.196e-11,
# 3.937e-10, 4.575e-8; test_swing_params_model.py recomputes it): the yardstick of that
# session, which has no fixture of the reference.
SESSION_N8_YARD = np.array([1.2e-11, 4.0e-10, 4.6e-8])


def session_v_ref(B=SESSION_B, seed=41):
    rng = np.random.default_rng(seed)
    v = np.zeros((B, 6))
    v[:, 0], v[:, 1], v[:, 5] = rng.uniform(-0.3, 0.8, B), rng.uniform(-0.2, 0.2, B), rng.uniform(-0.4, 0.4, B)
    return v


def full(case):
    """All five values of a case."""
    return dict(DEFAULTS, **CASES[case])


def load_golden():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swing_params_golden.npz"))
    return {k: d[k] for k in d.files}


def case_view(g, case):
    """The case's arrays under the key names of swing_golden.npz (step_in, trot_sub_ref,
    step_err, free_err, ...), so that swing_model.step_ratios / error_ratios apply as they are."""
    pre = case + "_"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
