"""CPU: the swing fixtures under non-default mpcq_swing_params
(tests/golden/swing_params_golden.npz: the unmodified reference under every case of
tests/swing_param_cases.py, gen_swing_golden.py params) against the numpy host model
(tests/swing_model.py).

Tolerance rule: as test_swing_model.py, but per case -- the yardstick of a case is the
reference's own float64 - longdouble error on that case's fixtures (``<case>_step_err``,
``<case>_free_err``), never the default fixture's and never anything measured on the kernel.
t0, t_swing, the mode and NaN patterns are exact.

Power: for every field a case moves, the model with that field alone put back to its default
misses the case's fixtures (an exact quantity differs, or a polynomial class is beyond
100 x TOL_FACTOR x the yardstick), in the step cases where get_next_foot reads the field and in
every free-running run.  A kernel that ignored the field computes what that model computes, so
it cannot pass test_gpu_swing_params.py.  No kernel is launched."""
import numpy as np
import pytest

import swing_model as M
import swing_param_cases as SC

STEP_FIELDS = ("dt", "max_height", "t_lock")  # what get_next_foot reads; k_mpc and feet_z: advance only


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as m
    m.build()
    return m


@pytest.fixture(scope="module")
def g():
    return SC.load_golden()


def ratios_or_inf(got, want, yard):
    """error_ratios for a model that may be wrong: a differing NaN pattern counts as inf."""
    d = np.abs(got - want)
    d[np.isnan(got) & np.isnan(want)] = 0.0
    d[np.isnan(d)] = np.inf
    return np.array([d[..., 0:3].max(), d[..., 3:6].max(), d[..., 6:9].max()]) / yard


def model_steps(v, p):
    """The case's step cases through the model's next_foot under params p: (out [n][11],
    state [n][40], exact: gx / gy, x1 / y1 and the mode as recorded)."""
    n = v["step_in"].shape[0]
    state = np.zeros((n, M.STATE))
    state[:, :26] = v["step_pre"]
    out = np.empty((n, 11))
    for i in range(n):
        out[i] = M.next_foot(state[i], *v["step_in"][i], p["dt"], p["max_height"], p["t_lock"])
    exact = (np.array_equal(out[:, 9:11], v["step_out"][:, 9:11]) and np.array_equal(state[:, 24:26], v["step_post"][:, 24:26])
             and np.array_equal(state[:, 34] == 1.0, v["step_mode"]))
    return out, state, exact


def step_ratios_or_inf(out, state, v):
    with np.errstate(invalid="ignore"):
        r = M.step_ratios(out, state[:, :24], v)
    return np.where(np.isnan(r), np.inf, r)


def model_free(v, name, var, p):
    """A free-running run of the case through the model's advance under params p, n_sub = 1
    calls with the recorded frames: (ref [T][K][4][9], final state, exact: t0, t_swing (slot
    32), the mode (slot 34) and the stance NaNs as recorded)."""
    k = lambda f: v[f"{name}_{var}_{f}"]  # noqa: E731
    T, K = k("t0").shape[:2]
    state = np.zeros((1, 4, M.STATE))
    ref = np.empty((T, K, 4, 9))
    rng = np.random.default_rng(7)
    exact = True
    for j in range(T):
        sw = k("gait")[j][0, 1:] == 0
        for ks in range(K):
            feet0 = k("feet0")[j, ks].copy()
            feet0[np.isnan(feet0)] = rng.normal(0, 1, int(np.isnan(feet0).sum()))  # read at lift-off only
            r, t0, status = M.advance(k("gait")[j][None], k("fsteps")[j][None], k("frame")[j, ks][None], state, ks, 1,
                                      feet0=feet0[None], params=p)
            exact = (exact and status[0] == 0 and np.array_equal(t0[0, 0], k("t0")[j, ks], equal_nan=True)
                     and np.array_equal(np.isnan(t0[0, 0]), ~sw)
                     and np.array_equal(state[0, sw, 32], k("t_swing")[j, ks][sw])
                     and np.array_equal(state[0, sw, 34], k("mode")[j, ks][sw])
                     and bool(np.isnan(r[0, 0][~sw]).all()))
            ref[j, ks] = r[0, 0]
    return ref, state, exact


def test_cases_and_params_round_trip(mpcq, g):
    assert list(g["cases"]) == list(SC.NAMES)
    assert SC.DEFAULTS == M.DEFAULTS
    for case in SC.NAMES:
        want = SC.full(case)
        assert np.array_equal(g[f"{case}_params"], [want[f] for f in SC.FIELDS]), case
        p = mpcq.default_swing_params(**SC.CASES[case])
        assert {f: getattr(p, f) for f in SC.FIELDS} == want, case
        assert isinstance(p.k_mpc, int) and all(x == 0 for x in p.reserved)
        moved = [f for f in SC.FIELDS if want[f] != SC.DEFAULTS[f]]
        assert sorted(moved) == sorted(SC.CASES[case]), case  # every override does move its field
    assert sum(len(c) for c in SC.CASES.values()) == 10
    with pytest.raises(AttributeError):
        mpcq.default_swing_params(height=0.1)


@pytest.mark.parametrize("case", SC.NAMES)
def test_fixture_reaches_both_modes_and_lifts_off(g, case):
    v, p = SC.case_view(g, case), SC.full(case)
    a = v["step_in"]
    assert v["step_mode"].any() and (~v["step_mode"]).any() and (a[:, 8] == 0).any()
    assert np.array_equal(v["step_mode"], (a[:, 9] - a[:, 8]) > p["t_lock"])
    t1 = np.unique(a[:, 9])
    for name, var in SC.FREE:
        k = lambda f: v[f"{name}_{var}_{f}"]  # noqa: E731
        assert k("t0").shape == (SC.TICKS, p["k_mpc"], 4) and k("ref").shape == (SC.TICKS, p["k_mpc"], 4, 9)
        assert (k("t0") == 0).any() and (k("mode") == 1).any() and (k("mode") == 0).any(), (name, var)
        ts = k("t_swing")
        assert np.isin(ts[~np.isnan(ts)], t1).all()  # the step cases swing over the scenarios' t1
        assert np.isfinite(k("ref")).sum() > 9 * 2 * p["k_mpc"] * 6
        held = all(np.array_equal(k("frame")[:, 0], k("frame")[:, ks]) for ks in range(p["k_mpc"]))
        assert held == (var == "tick")
    # one whole swing per t1: every t0 from 0 to t1 - dt
    for t in t1:
        i = a[:, 9] == t
        assert np.array_equal(a[i, 8], np.round(np.arange(int(round(t / p["dt"]))) * p["dt"], 3))
    assert (v["step_err"] > 0).all() and (v["free_err"] > 0).all()


@pytest.mark.parametrize("case", SC.NAMES)
def test_model_step_cases_under_params(g, case):
    v, p = SC.case_view(g, case), SC.full(case)
    out, state, exact = model_steps(v, p)
    assert exact
    r = M.step_ratios(out, state[:, :24], v)
    print(case, "model / reference error over the reference's own (pos, vel, acc, coeffs):", r)
    assert (r <= M.TOL_FACTOR).all(), r
    lock = ~v["step_mode"]
    assert np.array_equal(state[lock, :26], v["step_pre"][lock])  # locked: coefficients untouched
    # the batched entry point of the model takes the same params
    n = (len(out) // 4) * 4
    st = np.zeros((n // 4, 4, M.STATE))
    st[:, :, :26] = v["step_pre"][:n].reshape(n // 4, 4, 26)
    assert np.array_equal(M.step(v["step_in"][:n].reshape(n // 4, 4, 10), st, params=SC.CASES[case]).reshape(n, 11), out[:n])


@pytest.mark.parametrize("case", SC.NAMES)
def test_model_free_running_under_params(g, case):
    v, p = SC.case_view(g, case), SC.CASES[case]  # the overrides alone: the model fills in the rest
    K = SC.full(case)["k_mpc"]
    for name, var in SC.FREE:
        ref, state, exact = model_free(v, name, var, p)
        assert exact, (name, var)
        want = v[f"{name}_{var}_ref"]
        ratios = M.error_ratios(ref, want, v["free_err"])
        print(case, name, var, "model / reference error over the reference's own (pos, vel, acc):", ratios)
        assert (ratios <= M.TOL_FACTOR).all(), (name, var, ratios)
        if var == "tick":  # the frame is held per tick: one call over the whole tick, the same bits
            state2 = np.zeros((1, 4, M.STATE))
            ref2 = np.empty_like(ref)
            for j in range(SC.TICKS):
                feet0 = np.nan_to_num(v[f"{name}_{var}_feet0"][j, 0])
                ref2[j], t0, _ = M.advance(v[f"{name}_{var}_gait"][j][None], v[f"{name}_{var}_fsteps"][j][None],
                                           v[f"{name}_{var}_frame"][j, 0][None], state2, feet0=feet0[None], params=p)
                assert t0.shape == (1, K, 4) and np.array_equal(t0[0], v[f"{name}_{var}_t0"][j], equal_nan=True)
            assert np.array_equal(ref2, ref, equal_nan=True) and np.array_equal(state2, state)


@pytest.mark.parametrize("case,field", [(c, f) for c in SC.NAMES for f in SC.CASES[c]])
def test_every_case_has_power(g, case, field):
    """The model with ``field`` alone back at its default misses the case's fixtures."""
    v, p = SC.case_view(g, case), SC.full(case)
    assert p[field] != SC.DEFAULTS[field]
    p[field] = SC.DEFAULTS[field]
    bound = 100.0 * M.TOL_FACTOR
    if field in STEP_FIELDS:
        out, state, exact = model_steps(v, p)
        r = step_ratios_or_inf(out, state, v)
        print(case, field, "step cases: exact", exact, "ratios", r)
        assert (not exact) or (r > bound).any(), (case, field, r)
    for name, var in SC.FREE:
        ref, _, exact = model_free(v, name, var, p)
        r = ratios_or_inf(ref, v[f"{name}_{var}_ref"], v["free_err"])
        print(case, field, name, var, "exact", exact, "ratios", r)
        assert (not exact) or (r > bound).any(), (case, field, name, var, r)


def _model_own_error(name):
    """max |float64 - longdouble| of the model on the inputs of session ``name`` (the oracle's
    closed loop on the CPU), the modes met and the number of lift-offs."""
    LD = np.longdouble
    sw = SC.SESSIONS[name]["swing"]
    s64, sld = np.zeros((SC.SESSION_B, 4, M.STATE)), np.zeros((SC.SESSION_B, 4, M.STATE), LD)
    err, modes, lifts, stance = np.zeros(3), set(), 0, 0
    for gait, fsteps, frame in SC.session_swing_inputs(name):
        r64, t0, status = M.advance(gait, fsteps, frame, s64, params=sw)
        rld, t0l, _ = M.advance(gait, fsteps.astype(LD), frame.astype(LD), sld, params=sw)
        assert not status.any() and r64.shape == (SC.SESSION_B, sw["k_mpc"], 4, 9)
        assert np.array_equal(t0, t0l, equal_nan=True) and np.array_equal(np.isnan(r64), np.isnan(rld))
        assert np.array_equal(s64[:, :, 32:35], sld[:, :, 32:35].astype(np.float64))  # the same branches
        d = np.abs(np.nan_to_num((r64.astype(LD) - rld).astype(np.float64)))
        err = np.maximum(err, [d[..., 0:3].max(), d[..., 3:6].max(), d[..., 6:9].max()])
        swing = gait[:, 0, 1:] == 0
        modes |= set(s64[:, :, 34][swing].tolist())
        lifts += int((t0[:, 0] == 0).sum())
        stance += int((~swing).all(axis=1).sum())
    return err, modes, lifts, stance


@pytest.mark.parametrize("name", list(SC.SESSIONS))
def test_session_inputs_and_their_yardstick(g, name):
    """The sessions of test_session_swing_under_params, on the CPU (the oracle's closed loop):
    they meet both modes, all-stance ticks and lift-offs.  n8 has no fixture: its yardstick
    SESSION_N8_YARD is the model's own float64 - longdouble error on these inputs.  n16 runs
    case ``all`` and is held to that case's free_err; the model's own error there is below it,
    so these inputs are no harder than the fixture's."""
    err, modes, lifts, stance = _model_own_error(name)
    print(name, "model float64 - longdouble (pos, vel, acc):", err, "lift-offs", lifts, "all-stance robot ticks", stance)
    assert modes == {0.0, 1.0} and lifts >= SC.SESSION_B and stance >= SC.SESSION_B
    if name == "n8":
        assert (err <= SC.SESSION_N8_YARD).all() and (SC.SESSION_N8_YARD <= 1.1 * err).all(), err
    else:
        assert SC.SESSIONS[name]["swing"] == SC.CASES["all"]
        assert (err <= g["all_free_err"]).all(), err / g["all_free_err"]
