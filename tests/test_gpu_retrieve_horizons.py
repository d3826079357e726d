"""GPU: retrieve_kernel<N> (mpcq_session.hip) at each of the 61 compiled horizons, on its own
inputs, against the oracle's epilogue (oracle.retrieve), which test_retrieve_model.py ties to
numpy's own summation at every horizon.

The kernel has no stand-alone entry point; a session of three robots (trot / bound / pace, a
weights table with distinct rows, a command with a yaw rate) runs three ticks of the virtual
robot, and after each tick the oracle's epilogue is fed the arrays the kernel read:

- SV_X_ROBOT and SV_COST bit for bit.  The cost components are pairwise<N> / pairwise<12N> sums
  whose shape changes with N (a plain loop below 8 terms, eight partial sums up to 128, halves
  rounded to a multiple of 8 above): a left-to-right sum differs in the last bits at every N >= 8
  (test_retrieve_model.test_a_left_to_right_sum_differs), far below what a whole-session
  comparison at 1e-6 relative sees.
- SV_Q_W, SV_STATE, SV_L_FEET within PLAN_TOL * max(1, |reference|): test_gpu_planner.py's bound,
  by its argument -- the only sources are the device library's cos / sin against the host's.
- the private warm start (SP_WARM_X) through its only consumer: Engine.solve in update mode from
  the oracle's shifted x of the previous tick, with the session's previous SV_Y and SV_RHO,
  reproduces this tick's SV_X, SV_ITERS and SV_RHO bit for bit.  A wrong shift at one horizon
  changes the iteration path.

At N = 16 one robot gets a NaN command at tick 1 (MPCQ_STATUS_NONFINITE: a status, not a fault):
its duals are zeroed, its rho is the parameter's, its pose stays and its next solve starts cold.

Measured on an MI355X: the largest pose difference over all horizons is printed per case
(DESIGN.md section 2.1 has the table)."""
import numpy as np
import pytest

import weight_cases as WC
from horizon_cases import ALL_HORIZONS
from monitor_model import OK_STATUS, same
from test_gpu_planner import PLAN_TOL
from test_gpu_session import _gaits

pytestmark = pytest.mark.gpu

B, TICKS = 3, 3
V_REF = np.array([[0.3, 0.05, 0.0, 0.0, 0.0, 0.25], [0.5, -0.05, 0.0, 0.0, 0.0, -0.3], [0.2, 0.1, 0.0, 0.0, 0.0, 0.15]])
NAMES = ("SV_X", "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_X_ROBOT", "SV_COST", "SV_Q_W", "SV_STATE", "SV_L_FEET", "SV_Y",
         "SV_RHO", "SV_ITERS", "SV_STATUS")


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def _run(mpcq, oracle, N, nan_at=None):
    """Three ticks; returns the largest pose difference.  ``nan_at``: (tick, robot) of a NaN command."""
    weights = WC.make_weights(N, B=B)
    params = [oracle.default_params(**WC.oracle_overrides(weights[b])) for b in range(B)]
    worst, statuses = 0.0, []
    with mpcq.Engine(N) as eng, mpcq.Session(eng, B, gait0=_gaits(B, N)) as sess:
        sh = np.array(sess.planner_params.shoulders[:])
        sess.set_weights(weights)
        eng.set_weights(weights)  # (the engine's own table, for the stand-alone solves below)
        prev, warm_x = None, None
        for k in range(TICKS):
            pose = {n: sess.read(getattr(mpcq, n)) for n in ("SV_Q_W", "SV_STATE", "SV_L_FEET")}
            v = V_REF.copy()
            if nan_at is not None and nan_at[0] == k:
                v[nan_at[1], 0] = np.nan
            sess.tick(v)
            now = {n: sess.read(getattr(mpcq, n)) for n in NAMES}
            failed = ~np.isin(now["SV_STATUS"], OK_STATUS)
            statuses.append(now["SV_STATUS"].tolist())
            o = [oracle.retrieve(N, now["SV_X"][b], now["SV_XREF"][b], now["SV_FSTEPS"][b], now["SV_GAIT"][b],
                                 pose["SV_Q_W"][b], failed=bool(failed[b]), params=params[b], shoulders=sh)
                 for b in range(B)]
            for b in range(B):
                assert same(now["SV_X_ROBOT"][b], o[b]["x_robot"]), (N, k, b)
                assert same(now["SV_COST"][b], o[b]["cost"]), (N, k, b, now["SV_COST"][b] - o[b]["cost"])
                if failed[b]:  # pose and virtual state untouched, a cold restart
                    for n in pose:
                        assert same(now[n][b], pose[n][b]), (N, k, b, n)
                    assert not now["SV_Y"][b].any() and now["SV_RHO"][b] == eng.params.rho, (N, k, b)
                    continue
                for n, want in (("SV_Q_W", o[b]["q_w"]), ("SV_STATE", o[b]["state"]), ("SV_L_FEET", o[b]["l_feet"])):
                    d = _rel(now[n][b], want)
                    worst = max(worst, d)
                    assert d <= PLAN_TOL, (N, k, b, n, d)
            if k > 0:  # SP_WARM_X of the previous tick, through the solve that consumed it
                r = eng.solve(now["SV_XREF"], now["SV_FSTEPS"], mpcq.MODE_UPDATE, warm_x=warm_x, warm_y=prev["SV_Y"],
                              rho=prev["SV_RHO"], want_x=True)
                for n, key in (("SV_X", "x"), ("SV_ITERS", "iters"), ("SV_RHO", "rho")):
                    # (a robot that failed this tick: the retrieve has reset its rho after the solve)
                    assert same(now[n][~failed], r[key][~failed]), (N, k, n)
                assert same(now["SV_X"], r["x"]) and same(now["SV_ITERS"], r["iters"]), (N, k)
            prev, warm_x = now, np.stack([o[b]["warm_x"] for b in range(B)])
    return worst, statuses


@pytest.mark.parametrize("N", ALL_HORIZONS)
def test_retrieve_vs_oracle(mpcq, oracle, N):
    assert tuple(ALL_HORIZONS) == tuple(mpcq.supported_horizons())
    worst, statuses = _run(mpcq, oracle, N)
    print(f"N={N}: max |q_w, state, l_feet - oracle| / max(1, |oracle|) over {TICKS} ticks = {worst:.2e}")
    assert all(s in OK_STATUS for row in statuses for s in row), statuses


def test_nan_command_restarts_cold(mpcq, oracle):
    """N = 16, robot 1's command is NaN at tick 1: _run asserts on that robot that the duals are
    zero, rho is the parameter's, the pose and virtual state are untouched, and that tick 2's
    solve is the stand-alone solve from a zero warm start (the oracle's warm_x of a failed tick)."""
    _, statuses = _run(mpcq, oracle, 16, nan_at=(1, 1))
    assert statuses[1][1] == mpcq.STATUS_NONFINITE and statuses[1][0] in OK_STATUS, statuses
    assert all(s in OK_STATUS for s in statuses[0] + statuses[2]), statuses
