"""GPU: what the stage kernels share (mpcq_stage16.h, solve_failed), each pinned by running one
kernel along two paths that must give the same bits, so none of it needs a tolerance:

- the robot the controller believes, from a table filled with mpcq_default_robot or from no table;
- the previous tick's feet, from ``feet_prev`` (a stand-alone step) or from row 0 of ``fsteps`` (a
  session's tick);
- the failed decision, from the ``failed_prev`` mask (a stand-alone step) or from the previous
  tick's status and planner status (a session's tick), with the retrieve and the plant of the
  same session deciding the same robots failed.

Batch tails (B = 1, 3, 4, 5: below, at and over the four robots of a wave) of the stand-alone
estimator and disturb steps are test_kernel_alone_vs_model's in test_gpu_estimator.py and
test_gpu_disturb.py, against the numpy models; nothing is added for them here.
"""
import numpy as np
import pytest

import estimator_model as EM
from monitor_model import OK_STATUS, same

pytestmark = pytest.mark.gpu

N = 16
SIGMA = np.array([1e-3] * 6 + [1e-2] * 6)
EST = dict(lag=0, f_lag=0)
DIS = dict(f_lag=0, alpha=0.3)


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


# ------------------------------------------------------------------------------- robots: null or default
def test_default_table_is_no_table(mpcq):
    """B = 5 (two waves, the second with one robot), 10 ticks with a first flag and a failed tick."""
    B, T, lag, f_lag = 5, 10, 2, 1
    rng = np.random.default_rng(17)
    f, feet = EM.trot(T, B=B, seed=17)
    truth = EM.rollout(EM.start(B, 17), f, feet, f_lag=f_lag)
    obs = EM.delayed(truth, lag) + SIGMA * rng.standard_normal((T, B, 12))
    first = np.zeros((T, B), np.int32)
    first[5, 0] = 1
    failed = np.zeros((T, B), np.int32)
    failed[7, B - 1] = 1
    with mpcq.Engine(N) as eng:
        table = mpcq.robots(B, params=eng.params)
        est_k = mpcq.Estimator(eng, mpcq.default_estimator_params(lag=lag, f_lag=f_lag, r=list(SIGMA ** 2)))
        dis_k = mpcq.Disturb(eng, mpcq.default_disturb_params(f_lag=f_lag, alpha=0.4))
        er = [mpcq.estimator.new_rows(B) for _ in range(2)]
        dr = [mpcq.disturb.new_rows(B) for _ in range(2)]
        sampled = 0
        for t in range(T):
            fp = f[t - 1] if t else np.zeros((B, 12))
            ft = feet[t - 1] if t else np.zeros((B, 3, 4))
            kw = dict(first=first[t], all_first=t == 0, failed_prev=failed[t])
            e0, er[0] = est_k.step(obs[t], fp, ft, er[0], robots=None, **kw)
            e1, er[1] = est_k.step(obs[t], fp, ft, er[1], robots=table, **kw)
            assert same(e0, e1) and same(er[0], er[1]), t
            d0, r0, dr[0] = dis_k.step(obs[t], fp, ft, dr[0], robots=None, **kw)
            d1, r1, dr[1] = dis_k.step(obs[t], fp, ft, dr[1], robots=table, **kw)
            assert d0.tobytes() == d1.tobytes() and same(r0, r1) and same(dr[0], dr[1]), t
            if t:
                assert not same(e0, obs[t])  # (the model ran: the estimate is not the observation)
            sampled += int(np.isfinite(r0).all(axis=1).sum())
        assert sampled >= (T - 3) * B  # (the model ran in the disturb step too)
        assert (mpcq.estimator.unpack(er[0])["tau_next"] > 1).all()




# ------------------------------------------------------------------------------- feet and failed: either source
B = 6         # two waves, the second with two robots
BAD_PLAN = 4  # its gait loses its terminator before tick 2: the planner fails, the engine solves the stale buffers
BAD_CMD = 1   # its command is NaN at tick 4: the solve fails (MPCQ_STATUS_NONFINITE), the planner does not
INJECT = 6    # the tick before which MPCQ_SV_STATUS is overwritten
TICKS = 8
# what the estimator and the disturb stage read at tick INJECT: each non-failing status, a failing
# one, and (robot BAD_PLAN) a solved status beside a planner status that is not 0
INJECTED = np.array([1, 2, -2, -3, 1, 2], np.int32)
# under it the ticks of this session end in all three non-failing statuses (robot 0 needs 175 to
# 225 iterations from tick 1 on, the others 275 to 700)
MAX_ITER = 259


def _feet(fsteps):
    return np.ascontiguousarray(fsteps[:, 0, 1:].reshape(fsteps.shape[0], 4, 3).transpose(0, 2, 1))


def _not_ok(status):
    return ~np.isin(status, OK_STATUS)


def _session(mpcq, max_iter):
    """TICKS ticks of a session with plant, estimator and disturb stage.  Every tick, the session's
    estimator and disturb outputs must equal, bit for bit, a stand-alone step on the arrays the
    tick read, with the feet as ``feet_prev`` and the failed robots as a mask; and the robots the
    retrieve restarted cold and the plant left alone must be those of the status rule.  Returns
    the (status, failed) pairs the retrieve and the plant met, and the (status, planner failed,
    failed) triples the two stages met."""
    from mpcq import synth
    v_ref = np.zeros((B, 6))
    v_ref[:, 0] = np.linspace(0.0, 0.8, B)
    v_ref[:, 5] = np.linspace(-0.3, 0.3, B)
    gait0 = np.stack([synth.gait_table(("trot", "bound")[b % 2], N) for b in range(B)])
    seen, stage_seen = set(), set()
    with mpcq.Engine(N, max_iter=max_iter) as eng, mpcq.Session(eng, B, gait0=gait0) as s:
        est_k = mpcq.Estimator(eng, mpcq.default_estimator_params(**EST))
        dis_k = mpcq.Disturb(eng, mpcq.default_disturb_params(**DIS))
        s.enable_plant()
        s.enable_estimator(**EST)
        s.enable_disturb(**DIS)
        plan_failed = np.zeros(B, bool)  # by the planner status of the tick that passed
        for k in range(TICKS):
            if k == 2:
                g = s.read(mpcq.SV_GAIT)
                g[BAD_PLAN, :, 0] = 1.0
                s.write(mpcq.SV_GAIT, g)
            if k == INJECT:
                s.write(mpcq.SV_STATUS, INJECTED)
            status_prev = s.read(mpcq.SV_STATUS)
            state, f_prev, feet_prev = s.read(mpcq.SV_STATE), s.read(mpcq.SV_F0), _feet(s.read(mpcq.SV_FSTEPS))
            erow, drow = s.estimator_read(mpcq.EV_ROW), s.disturb_read(mpcq.DV_ROW)
            q_w = s.read(mpcq.SV_Q_W)
            failed_prev = _not_ok(status_prev) | plan_failed
            if k:
                stage_seen |= set(zip(status_prev.tolist(), plan_failed.tolist(), failed_prev.tolist()))
            v = v_ref.copy()
            if k == 4:
                v[BAD_CMD] = np.nan

            s.tick(v)

            # estimator and disturb stage: status / planner status / fsteps against mask / feet_prev
            est, erow = est_k.step(state, f_prev, feet_prev, erow, all_first=k == 0, failed_prev=failed_prev)
            assert same(s.estimator_read(mpcq.EV_EST), est) and same(s.estimator_read(mpcq.EV_ROW), erow), k
            dist, resid, drow = dis_k.step(est, f_prev, feet_prev, drow, all_first=k == 0, failed_prev=failed_prev)
            assert s.disturb_read(mpcq.DV_DIST).tobytes() == dist.tobytes(), k
            assert same(s.disturb_read(mpcq.DV_RESID), resid) and same(s.disturb_read(mpcq.DV_ROW), drow), k
            # (the mask decides: a failed robot's filter starts again, the others' go on)
            assert np.array_equal(mpcq.estimator.unpack(erow)["tau_next"] == 1, failed_prev | (k == 0)), k
            assert np.isnan(resid[failed_prev]).all(), k

            # retrieve and plant: the same robots by the same rule
            status = s.read(mpcq.SV_STATUS)
            failed = _not_ok(status)
            plan_failed = np.arange(B) == (BAD_PLAN if k >= 2 else -1)
            if k >= 2:  # the planner's status over the engine's, which solved the stale buffers
                assert status[BAD_PLAN] == mpcq.STATUS_BAD_GAIT, status
                assert np.isfinite(s.read(mpcq.SV_F0)[BAD_PLAN]).all() and s.read(mpcq.SV_ITERS)[BAD_PLAN] > 0, k
            if k == 4:
                assert status[BAD_CMD] == mpcq.STATUS_NONFINITE, status
            end = s.plant_read(mpcq.PV_STATE_END)
            assert np.array_equal(np.isnan(end).all(axis=1), failed) and np.isfinite(end[~failed]).all(), (k, status)
            y, rho = s.read(mpcq.SV_Y), s.read(mpcq.SV_RHO)
            assert np.array_equal(~y.any(axis=1), failed), (k, status)  # the retrieve's cold restart
            assert (rho[failed] == eng.params.rho).all(), k
            now = s.read(mpcq.SV_Q_W)
            assert same(now[failed], q_w[failed]), k  # neither moved a failed robot
            assert not any(same(now[b], q_w[b]) for b in np.flatnonzero(~failed)), k
            assert same(s.read(mpcq.SV_STATE)[failed], state[failed]), k
            seen |= set(zip(status.tolist(), failed.tolist()))
    return seen, stage_seen


def test_session_tick_and_step_agree_on_feet_and_failed(mpcq):
    """max_iter = MAX_ITER: the ticks end SOLVED, SOLVED_INACCURATE and MAX_ITER_REACHED (which of
    them depends on the robot and the tick), so the retrieve and the plant meet every non-failing
    status, two failing ones (MPCQ_STATUS_NONFINITE; the planner's MPCQ_STATUS_BAD_GAIT beside an
    engine that solved: the retrieve reads its status before overwriting it, the plant after).
    The estimator and the disturb stage meet those and the injected row."""
    seen, stage_seen = _session(mpcq, MAX_ITER)
    print("statuses after a tick:", sorted(seen), " read by the stages:", sorted(stage_seen))
    assert {st for st, f in seen if not f} == set(OK_STATUS), seen
    assert {st for st, f in seen if f} == {mpcq.STATUS_NONFINITE, mpcq.STATUS_BAD_GAIT}, seen
    for st in OK_STATUS:
        assert (st, False, False) in stage_seen, stage_seen
    assert (-3, False, True) in stage_seen and (1, True, True) in stage_seen, stage_seen
