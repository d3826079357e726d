"""CPU: the host model of the rigid-body plant (tests/plant_model.py) against closed forms,
and its PLANT_MODEL integrator against the oracle's closed loop: the MPC's own one-step map,
evaluated from xref[:, 0], row 0 of fsteps and f_applied, must land on the QP's x_robot[:, 0].

The oracle bound is 5e-5: the gap is OSQP's residual at eps 1e-7 (4.0e-6 at worst on these
16 ticks), not rounding, while the step itself is 1e-2 to 1 -- a wrong frame, sign or layout
shows five orders of magnitude above it."""
import numpy as np
import pytest

import plant_model as PM

V_REF = np.array([0.3, 0.1, 0.0, 0.0, 0.0, 0.4])
FEET = np.vstack([PM.SHOULDERS, np.zeros((1, 4))])  # under the shoulders, on the ground


def _level(B=1, h=0.2027682):
    x = np.zeros((B, 12))
    x[:, 2] = h
    return x


@pytest.mark.parametrize("n_sub", [1, 7, 20])
def test_free_fall_closed_form(n_sub):
    x = _level()
    x[:, 8] = 0.3
    feet = np.full((1, 3, 4), np.nan)  # no stance foot
    f = np.ones((1, 12))  # forces at swing feet are not applied
    out, fe = PM.step(x, feet, f, n_sub=n_sub)
    h = 0.02 / n_sub
    want = x[0, 2] + n_sub * h * 0.3 - 9.81 * h * h * n_sub * (n_sub + 1) / 2
    # up to 20 additions to quantities below 0.3, each rounded to half an ulp (2.8e-17 at most),
    # and c_z sums the velocities' errors again: below 20 x 20 x 2.8e-17 = 1.1e-14 in all
    assert abs(out[0, 2] - want) < 1.1e-14
    assert abs(out[0, 8] - (0.3 - 9.81 * 0.02)) < 1.1e-14
    assert not fe.any()
    assert np.array_equal(out[0, [0, 1, 3, 4, 5, 6, 7, 9, 10, 11]], np.zeros(10))


@pytest.mark.parametrize("integrator", [PM.MODEL, PM.RIGID])
def test_standing_still(integrator):
    x = _level()
    f = np.tile([0.0, 0.0, PM.MASS * 9.81 / 4], 4)[None]
    out, fe = PM.step(x, FEET[None], f, integrator=integrator)
    assert np.array_equal(fe, f)
    assert np.abs(out - x).max() < 1e-15


@pytest.mark.parametrize("axis", [0, 2])
def test_torque_free_spin_about_a_principal_axis(axis):
    gI = np.diag([0.03, 0.05, 0.07])
    x = _level()
    x[:, 9 + axis] = 1.5
    feet = np.full((1, 3, 4), np.nan)
    out, _ = PM.step(x, feet, np.zeros((1, 12)), consts=PM.constants(1, gI=gI), gravity=0.0)
    assert np.array_equal(out[0, 9:12], x[0, 9:12])  # the angular velocity is kept exactly
    want = np.zeros(3)
    want[axis] = 1.5 * 0.02
    assert np.abs(out[0, 3:6] - want).max() < 1e-15


def test_clamp():
    mu, fz_max = np.array([0.9]), np.array([25.0])
    inside = np.array([[1.0, -2.0, 10.0, 0.0, 0.0, 0.0, 6.3, 6.3, 9.9, -3.0, 4.0, 25.0]])
    fe, swing = PM.effective(FEET[None], inside, mu, fz_max, 1)
    assert not swing.any() and np.array_equal(fe.reshape(1, 12), inside)  # in the cone: bit-identical
    outside = np.array([[9.0, 12.0, 10.0, -8.0, 0.0, 5.0, 1.0, 1.0, 30.0, 30.0, -40.0, 26.0]])
    fe, _ = PM.effective(FEET[None], outside, mu, fz_max, 1)
    fe = fe[0]
    assert fe[:, 2].tolist() == [10.0, 5.0, 25.0, 25.0]  # fz limited to [0, fz_max]
    t = np.hypot(fe[:, 0], fe[:, 1])
    assert np.abs(t[[0, 1, 3]] - 0.9 * fe[[0, 1, 3], 2]).max() < 1e-14  # onto the cone t = mu fz
    assert np.array_equal(fe[2, :2], [1.0, 1.0])
    d = outside.reshape(4, 3)
    assert np.abs(fe[:, 0] * d[:, 1] - fe[:, 1] * d[:, 0]).max() < 1e-12  # the direction is kept
    pulling = np.array([[3.0, -4.0, -1.0, 3.0, -4.0, 0.0, 0.0, 0.0, -5.0, 1.0, 1.0, 1e-3]])
    fe, _ = PM.effective(FEET[None], pulling, mu, fz_max, 1)
    assert np.array_equal(fe[0, :3], np.zeros((3, 3)))  # fz <= 0: no force at all
    # without the clamp only swing feet are zeroed
    feet = FEET[None].copy()
    feet[0, 1, 2] = np.nan
    fe, swing = PM.effective(feet, outside, mu, fz_max, 0)
    want = outside.reshape(4, 3).copy()
    want[2] = 0.0
    assert swing.tolist() == [[False, False, True, False]] and np.array_equal(fe[0], want)


def test_nan_stays_in_its_robot():
    rng = np.random.default_rng(0)
    x = _level(3) + 0.01 * rng.standard_normal((3, 12))
    f = np.tile([1.0, -1.0, 6.0], (3, 4))
    ref, _ = PM.step(x, np.tile(FEET, (3, 1, 1)), f)
    f[1, 4] = np.nan
    out, fe = PM.step(x, np.tile(FEET, (3, 1, 1)), f)
    assert np.array_equal(out[[0, 2]], ref[[0, 2]])
    assert np.isnan(out[1]).any() and np.isnan(fe[1, 4])


@pytest.mark.parametrize("gait", ["trot", "bound"])
def test_model_integrator_reproduces_the_mpc_prediction(gait):
    from mpcq import synth
    from oracle import oracle as O
    N = 16
    s = O.Session(N, synth.gait_table(gait, N))
    worst = 0.0
    for k in range(8):
        q_w_prev = s.q_w.copy()
        assert s.tick(k, V_REF) == 1, k
        xref, fsteps = s.planner.xref, s.planner.fsteps
        r = PM.session_tick(xref[None, :, 0], fsteps[None], s.planner.gait[None], s.f0[None], q_w_prev[None],
                            integrator=PM.MODEL, clamp=0)
        err = float(np.abs(r["end"][0] - s.x_robot[:, 0]).max())
        worst = max(worst, err)
        assert err <= 5e-5, (k, err)
        # and the tail on the prediction itself is the retrieve's
        q_w, ns, lf = PM.tail(s.x_robot[None, :, 0], q_w_prev[None], fsteps[None], s.planner.gait[None])
        assert np.abs(q_w[0] - s.q_w).max() < 1e-15
        assert np.abs(ns[0] - s.state).max() < 1e-15 and np.abs(lf[0] - s.l_feet).max() < 1e-15
    print(f"{gait}: max |MODEL - x_robot[:, 0]| = {worst:.2e}")
