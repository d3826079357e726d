"""CPU: the estimator's host model (tests/estimator_model.py) on a synthetic 64-tick trajectory --
prescribed trot forces with swing feet (no QP), the truth made by plant_model's MODEL step plus
the frame change, the observations delayed by L.  What the filter promises is checked here in
exact arithmetic of the model; tests/test_gpu_estimator.py then pins the kernel to the model."""
import numpy as np
import pytest

import estimator_model as EM

T = 64
SIGMA = np.array([1e-3] * 6 + [1e-2] * 6)
NOISE_SEED = 20  # chosen with the model: any seed tried passed; the ratios are in DESIGN.md 4.14


def _loop(lag, f_lag, B=1, seed=3, ticks=T):
    f, feet = EM.trot(ticks, B=B, seed=seed)
    truth = EM.rollout(EM.start(B), f, feet, f_lag=f_lag)
    return f, feet, truth, EM.delayed(truth, lag)


@pytest.mark.parametrize("lag,f_lag", [(0, 0), (2, 0), (3, 1), (8, 4)])
def test_exact_case_recovers_the_truth(lag, f_lag):
    f, feet, truth, obs = _loop(lag, f_lag)
    est, rows = EM.run(EM.params(lag=lag, f_lag=f_lag), obs, f, feet)
    assert np.isfinite(est).all()
    err = np.abs(est - truth[:T]).max()
    raw = np.abs(obs - truth[:T]).max()
    print(f"lag {lag} f_lag {f_lag}: max |est - truth| {err}, max |obs - truth| {raw}")
    assert err == 0.0
    if lag:
        assert raw > 0.05  # the delay is visible in the raw observation
    ck = EM.clock(rows)
    assert ck[0, 0] == 1 and ck[0, 1] == max(T - 1 - lag, 0) and ck[0, 2] == T and ck[0, 3] == 0


@pytest.mark.parametrize("lag,f_lag", [(0, 0), (3, 1), (8, 4)])
def test_zero_gain_is_the_pure_rollout(lag, f_lag):
    f, feet, truth, obs = _loop(lag, f_lag)
    rng = np.random.default_rng(5)
    noisy = obs + 0.1 * rng.standard_normal(obs.shape)
    est, rows = EM.run(EM.params(lag=lag, f_lag=f_lag, p0=0.0, q=0.0), noisy, f, feet)
    # from the first observation on nothing but the model: the rollout from noisy[0]
    roll = EM.rollout(noisy[0], f, feet, f_lag=f_lag)
    assert np.array_equal(est, roll[:T])
    assert not rows[:, EM.P_OFF:EM.P_OFF + 18].any()  # every P entry stays exactly 0


@pytest.mark.parametrize("lag,f_lag", [(0, 0), (2, 1), (8, 4)])
def test_noise_is_reduced_in_every_component(lag, f_lag):
    f, feet, truth, obs = _loop(lag, f_lag)
    rng = np.random.default_rng(NOISE_SEED)
    noisy = obs + SIGMA * rng.standard_normal(obs.shape)
    est, _ = EM.run(EM.params(lag=lag, f_lag=f_lag, r=list(SIGMA ** 2)), noisy, f, feet)
    rms = lambda a: np.sqrt((a ** 2).mean(axis=(0, 1)))  # noqa: E731
    r_est, r_obs = rms(est - truth[:T]), rms(noisy - truth[:T])
    print(f"lag {lag} f_lag {f_lag}: RMS ratios", np.round(r_est / r_obs, 3))
    assert (r_est < r_obs).all(), r_est / r_obs


def _mixed(B=3, ticks=30, lag=2, f_lag=1, **over):
    """A case that exercises every rule: noise, a repeated row, a NaN row, a failed tick, a first
    flag in mid-run."""
    f, feet, truth, obs = _loop(lag, f_lag, B=B, seed=7, ticks=ticks)
    rng = np.random.default_rng(11)
    obs = obs + SIGMA * rng.standard_normal(obs.shape)
    obs[9, 1] = obs[8, 1]       # a repeated frame
    obs[13, 0, 4] = np.nan      # a missing one
    first = np.zeros((ticks, B), np.int32)
    failed = np.zeros((ticks, B), np.int32)
    first[17, 2] = 1
    failed[21, 0] = 1
    args = dict(lag=lag, f_lag=f_lag, r=list(SIGMA ** 2))
    args.update(over)
    est, rows = EM.run(EM.params(**args), obs, f, feet, first=first, failed=failed)
    return est, rows, obs


def test_rule_coverage():
    est, rows, obs = _mixed()
    # a first flag and a failed previous tick initialise: the estimate is the observation, bit for bit
    assert np.array_equal(est[17, 2], obs[17, 2]) and np.array_equal(est[21, 0], obs[21, 0])
    assert not np.array_equal(est[17, 1], obs[17, 1]) and not np.array_equal(est[21, 1], obs[21, 1])
    # a NaN row is a missing frame: the estimate stays finite and is the model's forecast
    assert np.isfinite(est[13, 0]).all() and np.isfinite(est[14:, 0]).all()
    # a repeated row: skipped with skip_repeats, used without
    est_off, _, _ = _mixed(skip_repeats=0)
    assert np.array_equal(est[:9], est_off[:9]) and np.array_equal(est[9, [0, 2]], est_off[9, [0, 2]])
    assert not np.array_equal(est[9, 1], est_off[9, 1])
    # tau restarts at an initialisation
    ck = EM.clock(rows)
    assert list(ck[:, 2]) == [30 - 21, 30, 30 - 17] and list(ck[:, 0]) == [1, 1, 1]


def test_lag_changed_in_mid_run_reinitialises():
    f, feet, truth, obs = _loop(3, 1, ticks=30)
    rows = EM.new_rows(1)
    a, b = EM.params(lag=3, f_lag=1), EM.params(lag=5, f_lag=1)
    for t in range(30):
        p = a if t < 12 else b
        est = EM.step(p, rows, obs[t], f[t - 1] if t else 0.0 * f[0], feet[t - 1] if t else 0.0 * feet[0], all_first=t == 0)
        ck = EM.clock(rows)[0]
        if t == 12:  # the stored s is not the one lag 5 would have left: rule 1
            assert np.array_equal(est, obs[t]) and tuple(ck[:3]) == (1, 0, 1)
        if t == 11:
            assert tuple(ck[:3]) == (1, 8, 12) and np.array_equal(est, truth[t])


def test_ring_wraps():
    """36 ticks at (8, 4): every slot is written three times, and the force of tick tau - 13 is
    read from the slot that the record of tick tau - 1 then takes."""
    f, feet, truth, obs = _loop(8, 4, ticks=36)
    est, rows = EM.run(EM.params(lag=8, f_lag=4), obs, f, feet)
    assert np.array_equal(est, truth[:36])
    rg = EM.ring(rows)[0]
    for j in range(23, 35):  # the last 12 recorded ticks, by absolute tick
        assert np.array_equal(rg[j % 12, :12], f[j, 0])
        assert np.array_equal(rg[j % 12, 12:], feet[j, 0].reshape(12), equal_nan=True)


FIELDS = [dict(lag=3), dict(f_lag=0), dict(skip_repeats=0)] + \
    [dict(q=[1e-6 if j != i else 1e-3 for j in range(6)] + [1e-4] * 6) for i in (2, 3, 4)] + \
    [dict(q=[1e-6] * 6 + [1e-4 if j != i else 1e-2 for j in range(6)]) for i in range(6)] + \
    [dict(r=[SIGMA[j] ** 2 * (50.0 if j == i else 1.0) for j in range(12)]) for i in range(12)] + \
    [dict(p0=[1e-2 if j != i else 1.0 for j in range(12)]) for i in range(12)]


def test_field_sensitivity():
    """Changing any one field of the mixed case changes the output (q of x, y and yaw is what the
    frame change pins their variance to: it acts through the gain as the others do)."""
    base, _, _ = _mixed()
    pinned = [dict(q=[1e-6 if j != i else 1e-3 for j in range(6)] + [1e-4] * 6) for i in EM.PINNED]
    for over in FIELDS + pinned:
        est, _, _ = _mixed(**over)
        assert est.shape == base.shape and not np.array_equal(est, base, equal_nan=True), over
