"""CPU: the swing-foot additions of the C ABI are exported, their default parameters are the
reference's constants, and the numpy host model (tests/swing_model.py) reproduces every
fixture of tests/golden/swing_golden.npz (the unmodified reference, gen_swing_golden.py):
t0, t_swing, the mode and the BAD_GAIT cases exactly, the polynomial outputs within the
tolerance rule (swing_model.TOL_FACTOR times the reference's own float64 - longdouble error).
No kernel is launched."""
import numpy as np
import pytest

import swing_model as M

NEW = ("mpcq_default_swing_params", "mpcq_swing_step_batch", "mpcq_swing_batch", "mpcq_session_enable_swing")


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as m
    m.build()
    return m


@pytest.fixture(scope="module")
def g():
    return M.load_golden()


def test_exports_swing_symbols(mpcq):
    lib = mpcq.lib()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in mpcq._lib.EXPORTS
    assert mpcq.Swing and mpcq.SwingParams and mpcq.SWING_STATE == M.STATE
    assert (mpcq.SV_SWING_REF, mpcq.SV_SWING_STATE, mpcq.SV_FRAME) == (17, 18, 19)
    assert lib.mpcq_abi_version() == 3


def test_default_swing_params(mpcq, g):
    p = mpcq.default_swing_params()
    assert (p.dt, p.max_height, p.t_lock, p.feet_z, p.k_mpc) == (0.001, 0.05, 0.05, 0.0, 20)
    assert all(v == 0 for v in p.reserved)
    assert np.array_equal(g["params"], [p.dt, p.max_height, p.t_lock, p.feet_z, p.k_mpc])
    assert M.DEFAULTS == dict(dt=p.dt, max_height=p.max_height, t_lock=p.t_lock, feet_z=p.feet_z, k_mpc=p.k_mpc)


def test_fixture_covers_the_cases(g):
    a = g["step_in"]
    assert a.shape[0] >= 300
    dif = a[:, 9] - a[:, 8]
    assert set(np.unique(a[:, 9])) == {0.14, 0.16}
    assert (a[:, 8] == 0).any() and (np.abs(dif - 0.001) < 1e-12).any()
    assert g["step_mode"].any() and (~g["step_mode"]).any()
    i = np.flatnonzero((a[:, 9] == 0.14) & (a[:, 8] == 0.09))
    assert len(i) and g["step_mode"][i].all()  # 0.14 - 0.09 = 0.05000000000000002: still adaptive
    i = np.flatnonzero((a[:, 9] == 0.16) & (a[:, 8] == 0.11))
    assert len(i) and not g["step_mode"][i].any()  # 0.16 - 0.11 = 0.05: locked
    assert list(g["scenarios"]) == ["trot", "bound", "side", "static", "trot2"]
    assert g["trot_sub_t0"].shape == (24, 20, 4)
    assert np.nanmax(g["trot_sub_t_swing"]) == 0.14  # 7 x 0.02 s
    assert set(g["tab_raises"].tolist()) == {"", "IndexError"}
    # the reference's own rounding error, the yardstick of the tolerances
    assert (g["step_err"] > 0).all() and (g["free_err"] > 0).all()
    assert (g["step_err"][:3] < [1e-11, 1e-9, 1e-7]).all() and (g["free_err"] < [1e-10, 1e-8, 1e-6]).all()


def test_model_step_cases(g):
    n = g["step_in"].shape[0]
    state = np.zeros((n, 1, M.STATE))
    state[:, 0, :26] = g["step_pre"]
    args = g["step_in"][:, None, :]
    out = np.empty((n, 11))
    dt, max_height, t_lock = (float(x) for x in g["params"][:3])
    for i in range(n):
        out[i] = M.next_foot(state[i, 0], *args[i, 0], dt, max_height, t_lock)
    assert np.array_equal(out[:, 9:11], g["step_out"][:, 9:11])  # gx, gy
    assert np.array_equal(state[:, 0, 24:26], g["step_post"][:, 24:26])
    assert np.array_equal(state[:, 0, 34] == 1.0, g["step_mode"])
    r = M.step_ratios(out, state[:, 0, :24], g)
    print("model / reference error over the reference's own (pos, vel, acc, coeffs):", r)
    assert (r <= M.TOL_FACTOR).all(), r
    # a locked call leaves the coefficients alone
    lock = ~g["step_mode"]
    assert np.array_equal(state[lock, 0, :26], g["step_pre"][lock])


def test_model_step_skips_nan_t0(g):
    args = np.tile(g["step_in"][:8].reshape(2, 4, 10), (1, 1, 1))
    args[0, 2, 8] = np.nan
    state = np.zeros((2, 4, M.STATE))
    state[0, 2, :5] = 7.0
    out = M.step(args, state)
    assert np.isnan(out[0, 2]).all() and np.array_equal(state[0, 2, :5], [7.0] * 5) and not state[0, 2, 5:].any()
    assert np.isfinite(np.delete(out.reshape(8, 11), 2, axis=0)).all()


def test_model_timing_tables(g):
    seen_bad = 0
    for gait, k_sub, name, t0, ts in zip(g["tab_gait"], g["tab_k_sub"], g["tab_raises"], g["tab_t0"], g["tab_t_swing"]):
        fsteps = np.zeros((20, 13))
        state = np.zeros((4, M.STATE))
        state[:, 35] = 3.0
        keep = state.copy()
        ref, mt0, status = M.advance(gait[None], fsteps[None], np.zeros((1, 3)), state[None], int(k_sub), 1)
        if name:
            assert name == "IndexError" and status[0] == M.BAD_GAIT
            assert np.isnan(ref).all() and np.isnan(mt0).all() and np.array_equal(state, keep)
            seen_bad += 1
        else:
            assert status[0] == 0
            assert np.array_equal(np.isnan(mt0[0, 0]), np.isnan(t0))
            sw = ~np.isnan(t0)
            assert np.array_equal(mt0[0, 0][sw], t0[sw])
            assert np.array_equal(state[sw, 32], ts[sw])
            assert np.array_equal(sw, gait[0, 1:] == 0)
    assert seen_bad >= 4
    assert not g["tab_gait"][0].any() and g["tab_raises"][0] == "IndexError"  # the empty table


@pytest.mark.parametrize("var", ["sub", "tick"])
@pytest.mark.parametrize("name", ["trot", "bound", "side", "static", "trot2"])
def test_model_free_running(g, name, var):
    """Every substep of every scenario, one robot: n_sub = 1 calls with the recorded frames."""
    k = lambda f: g[f"{name}_{var}_{f}"]  # noqa: E731
    T, K = k("t0").shape[:2]
    assert (T, K) == (24, 20)
    state = np.zeros((1, 4, M.STATE))
    ref = np.empty((T, K, 4, 9))
    rng = np.random.default_rng(7)
    for j in range(T):
        for ks in range(K):
            feet0 = k("feet0")[j, ks].copy()
            # the reference reads the measured foot at lift-off only: anything elsewhere
            feet0[np.isnan(feet0)] = rng.normal(0, 1, int(np.isnan(feet0).sum()))
            r, t0, status = M.advance(k("gait")[j][None], k("fsteps")[j][None], k("frame")[j, ks][None], state, ks, 1,
                                      feet0=feet0[None])
            assert status[0] == 0
            sw = k("gait")[j][0, 1:] == 0
            assert np.array_equal(np.isnan(t0[0, 0]), ~sw) and np.array_equal(np.isnan(k("t0")[j, ks]), ~sw)
            assert np.array_equal(t0[0, 0][sw], k("t0")[j, ks][sw])
            assert np.array_equal(state[0, sw, 32], k("t_swing")[j, ks][sw])
            assert np.array_equal(state[0, sw, 34], k("mode")[j, ks][sw])
            assert np.isnan(r[0, 0][~sw]).all()
            ref[j, ks] = r[0, 0]
    if name == "static":
        assert np.isnan(ref).all()
    else:
        assert np.isfinite(ref).any()
    ratios = M.error_ratios(ref, k("ref"), g["free_err"])
    print(name, var, "model / reference error over the reference's own (pos, vel, acc):", ratios)
    assert (ratios <= M.TOL_FACTOR).all(), ratios
    if var == "tick":
        assert all(np.array_equal(k("frame")[:, 0], k("frame")[:, ks]) for ks in range(K))
        # the frame is held per tick: one call over the whole tick gives the same bits
        # (a swing lifts off on a tick's first substep, so that substep's measured feet serve)
        state2 = np.zeros((1, 4, M.STATE))
        ref2 = np.empty_like(ref)
        for j in range(T):
            feet0 = np.nan_to_num(k("feet0")[j, 0])
            ref2[j], t0, _ = M.advance(k("gait")[j][None], k("fsteps")[j][None], k("frame")[j, 0][None], state2, 0, K,
                                       feet0=feet0[None])
            assert np.array_equal(t0[0], k("t0")[j], equal_nan=True)
        assert np.array_equal(ref2, ref, equal_nan=True) and np.array_equal(state2, state)


def test_model_last_xy_and_null_feet0(g):
    """The rules without a reference counterpart: stance feet record frame . fsteps row 0,
    a swing foot its goal, and feet0 = None lifts off from there at rest."""
    gait, fsteps = g["trot_tick_gait"], g["trot_tick_fsteps"]
    frame = g["trot_tick_frame"][:, 0]
    state = np.zeros((1, 4, M.STATE))
    j = 0
    ref, t0, _ = M.advance(gait[j][None], fsteps[j][None], frame[j][None], state)
    assert np.isnan(ref).all()  # all four feet in stance on the first tick
    for f in range(4):
        wx, wy = M.to_world(frame[j], fsteps[j][0, 3 * f + 1], fsteps[j][0, 3 * f + 2])
        assert (state[0, f, 35], state[0, f, 36]) == (wx, wy)
    assert not state[0, :, :35].any()
    last = state[0, :, 35:37].copy()
    ref, t0, _ = M.advance(gait[1][None], fsteps[1][None], frame[1][None], state)
    sw = np.flatnonzero(gait[1][0, 1:] == 0)
    assert len(sw) == 2 and (t0[0, 0, sw] == 0).all()
    for f in sw:
        # lift-off at rest from the last stance position: the first goal is within the first
        # millisecond's motion of it, the velocity still tiny
        assert np.abs(ref[0, 0, f, 0:2] - last[f]).max() < 1e-5
        assert np.array_equal(state[0, f, 35:37], ref[0, -1, f, 0:2])
