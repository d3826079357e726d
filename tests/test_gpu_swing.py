"""GPU: the batched swing-foot trajectories (mpcq_swing_step_batch / mpcq_swing_batch,
mpcq_swing.hip; Session.enable_swing) against the fixtures captured from the unmodified
reference (tests/golden/swing_golden.npz) and the host model (tests/swing_model.py).

Tolerance rule (swing_model.TOL_FACTOR): per class of quantity -- positions, velocities,
accelerations, coefficients (relative to each slot's largest magnitude) -- the bound is 16 x
the reference's own rounding error on the fixture set, max |float64 - longdouble|
(step_err / free_err).  t0, t_swing, the mode, gx / gy, NaN patterns and statuses are exact.
Every test prints its measured ratios before asserting."""
import ctypes as C

import numpy as np
import pytest

import swing_model as M

pytestmark = pytest.mark.gpu

SCENARIOS = ("trot", "bound", "side", "static", "trot2")


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as m
    return m


@pytest.fixture(scope="module")
def eng(mpcq):
    e = mpcq.Engine(16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def g():
    return M.load_golden()


def _step_batch(g, n_cases):
    """The first n_cases step cases as feet of ceil(n / 4) robots (the rest: t0 = NaN)."""
    B = (n_cases + 3) // 4
    args = np.full((B * 4, 10), np.nan)
    state = np.zeros((B * 4, M.STATE))
    args[:n_cases] = g["step_in"][:n_cases]
    state[:n_cases, :26] = g["step_pre"][:n_cases]
    state[n_cases:, :37] = 5.0  # skipped feet: must stay as they are
    return B, args.reshape(B, 4, 10), state.reshape(B, 4, M.STATE)


@pytest.mark.parametrize("n_cases", [4, 68, None])  # B = 1, 17 and the full set
def test_step_cases(mpcq, eng, g, n_cases):
    n = g["step_in"].shape[0] if n_cases is None else n_cases
    B, args, state = _step_batch(g, n)
    if n_cases == 68:  # a skipped foot in the middle of a wave
        args[3, 1, 8] = np.nan
    sw = mpcq.Swing(eng, B)
    sw.state[:] = state
    out = sw.step(args).reshape(B * 4, 11)
    post = sw.state.reshape(B * 4, M.STATE)
    pre = state.reshape(B * 4, M.STATE)
    skipped = np.isnan(args.reshape(B * 4, 10)[:, 8])
    assert np.isnan(out[skipped]).all() and np.array_equal(post[skipped], pre[skipped])
    live = ~skipped[:n]
    assert np.array_equal(out[:n, 9:11][live], g["step_out"][:n, 9:11][live])  # gx, gy
    assert np.array_equal(post[:n, 24:26][live], g["step_post"][:n, 24:26][live])
    assert np.array_equal(post[:n, 34][live] == 1.0, g["step_mode"][:n][live])
    assert np.array_equal(post[:n, 26:34], pre[:n, 26:34]) and np.array_equal(post[:n, 35:], pre[:n, 35:])
    o, p = out[:n].copy(), post[:n, :24].copy()
    o[~live], p[~live] = g["step_out"][:n][~live], g["step_post"][:n, :24][~live]
    r = M.step_ratios(o, p, g)
    print(f"step B={B}: kernel / reference error over the reference's own (pos, vel, acc, coeffs): {r}")
    assert (r <= M.TOL_FACTOR).all(), r
    lock = ~g["step_mode"][:n] & live
    assert np.array_equal(post[:n, :26][lock], g["step_pre"][:n][lock])  # locked: coefficients untouched


def _fill_feet0(f0, rng):
    f0 = f0.copy()
    m = np.isnan(f0)
    f0[m] = rng.normal(0, 1, int(m.sum()))  # read at lift-off only: anything elsewhere
    return f0


def _stack(g, var, field, j, ks=None):
    a = [g[f"{s}_{var}_{field}"][j] for s in SCENARIOS]
    return np.ascontiguousarray(np.stack(a) if ks is None else np.stack(a)[:, ks])


def test_free_running_per_substep(mpcq, eng, g):
    """Every scenario (one robot each), every substep, every swing foot: n_sub = 1 calls with
    the recorded per-substep frames."""
    B, T, K = len(SCENARIOS), 24, 20
    sw = mpcq.Swing(eng, B)
    rng = np.random.default_rng(11)
    ref = np.empty((B, T, K, 4, 9))
    for j in range(T):
        gait, fsteps = _stack(g, "sub", "gait", j), _stack(g, "sub", "fsteps", j)
        for ks in range(K):
            r = sw.advance(gait, fsteps, _stack(g, "sub", "frame", j, ks), ks, 1,
                           feet0=_fill_feet0(_stack(g, "sub", "feet0", j, ks), rng))
            assert not sw.status.any()
            want_t0 = _stack(g, "sub", "t0", j, ks)
            assert np.array_equal(sw.t0[:, 0], want_t0, equal_nan=True)
            swing = ~np.isnan(want_t0)
            assert np.array_equal(swing, gait[:, 0, 1:] == 0)
            assert np.array_equal(sw.state[:, :, 32][swing], _stack(g, "sub", "t_swing", j, ks)[swing])
            assert np.array_equal(sw.state[:, :, 34][swing], _stack(g, "sub", "mode", j, ks)[swing])
            assert np.array_equal(sw.state[:, :, 33][swing], want_t0[swing])
            assert np.isnan(r[:, 0][~swing]).all()  # stance feet
            ref[:, j, ks] = r[:, 0]
    want = np.stack([g[f"{s}_sub_ref"] for s in SCENARIOS])
    assert np.isfinite(want).sum() > 10000
    ratios = M.error_ratios(ref, want, g["free_err"])
    print("free-running, per substep: kernel / reference error over the reference's own (pos, vel, acc):", ratios)
    assert (ratios <= M.TOL_FACTOR).all(), ratios


def test_free_running_whole_tick(mpcq, eng, g):
    """The scenarios regenerated with the frame held per tick: one n_sub = 20 call per tick;
    substeps 0..6 then 7..19 give the single call's bits."""
    B, T, K = len(SCENARIOS), 24, 20
    one, two = mpcq.Swing(eng, B), mpcq.Swing(eng, B)
    rng = np.random.default_rng(12)
    ref = np.empty((B, T, K, 4, 9))
    for j in range(T):
        gait, fsteps = _stack(g, "tick", "gait", j), _stack(g, "tick", "fsteps", j)
        frame = _stack(g, "tick", "frame", j, 0)
        feet0 = _fill_feet0(_stack(g, "tick", "feet0", j, 0), rng)  # a swing lifts off on substep 0
        ref[:, j] = one.advance(gait, fsteps, frame, 0, K, feet0=feet0)
        want_t0 = np.stack([g[f"{s}_tick_t0"][j] for s in SCENARIOS])
        assert np.array_equal(one.t0, want_t0, equal_nan=True) and not one.status.any()
        swing = gait[:, 0, 1:] == 0
        assert np.array_equal(one.state[:, :, 32][swing], _stack(g, "tick", "t_swing", j, K - 1)[swing])
        assert np.array_equal(one.state[:, :, 34][swing], _stack(g, "tick", "mode", j, K - 1)[swing])
        assert np.isnan(ref[:, j][~np.broadcast_to(swing[:, None, :], (B, K, 4))]).all()
        ra = two.advance(gait, fsteps, frame, 0, 7, feet0=feet0)
        ta = two.t0.copy()
        rb = two.advance(gait, fsteps, frame, 7, 13, feet0=feet0)
        assert np.array_equal(np.concatenate([ra, rb], 1), ref[:, j], equal_nan=True)
        assert np.array_equal(np.concatenate([ta, two.t0], 1), one.t0, equal_nan=True)
        assert np.array_equal(two.state, one.state)
    want = np.stack([g[f"{s}_tick_ref"] for s in SCENARIOS])
    ratios = M.error_ratios(ref, want, g["free_err"])
    print("free-running, whole tick: kernel / reference error over the reference's own (pos, vel, acc):", ratios)
    assert (ratios <= M.TOL_FACTOR).all(), ratios


def _mixed_batch(g, B, seed=21):
    """B robots with different gaits: scenario b % 5 at tick 1 + b % 23 and a random, mid-swing
    generator state."""
    rng = np.random.default_rng(seed)
    s = [SCENARIOS[b % 5] for b in range(B)]
    j = [1 + b % 23 for b in range(B)]
    gait = np.stack([g[f"{n}_tick_gait"][t] for n, t in zip(s, j)])
    fsteps = np.stack([g[f"{n}_tick_fsteps"][t] for n, t in zip(s, j)])
    frame = np.stack([g[f"{n}_tick_frame"][t, 0] for n, t in zip(s, j)])
    state = np.zeros((B, 4, M.STATE))
    state[:, :, :37] = rng.normal(0, 0.1, (B, 4, 37))
    feet0 = rng.normal(0, 0.1, (B, 4, 6))
    return gait, fsteps, frame, state, feet0


@pytest.mark.parametrize("null_feet0", [False, True])
def test_layout_each_robot_as_alone(mpcq, eng, g, null_feet0):
    """B = 1, 16, 17, 33 robots with different gaits: each robot gets the bits it gets alone."""
    gait, fsteps, frame, state, feet0 = _mixed_batch(g, 33)
    alone_ref, alone_t0, alone_state = [], [], []
    for b in range(33):
        sw = mpcq.Swing(eng, 1)
        sw.state[:] = state[b]
        alone_ref.append(sw.advance(gait[b:b + 1], fsteps[b:b + 1], frame[b:b + 1], 3, 9,
                                    feet0=None if null_feet0 else feet0[b:b + 1])[0])
        alone_t0.append(sw.t0[0])
        alone_state.append(sw.state[0].copy())
    assert np.isfinite(np.array(alone_ref)).any() and np.isnan(np.array(alone_ref)).any()
    for B in (16, 17, 33):
        sw = mpcq.Swing(eng, B)
        sw.state[:] = state[:B]
        ref = sw.advance(gait[:B], fsteps[:B], frame[:B], 3, 9, feet0=None if null_feet0 else feet0[:B])
        assert np.array_equal(ref, np.array(alone_ref[:B]), equal_nan=True), B
        assert np.array_equal(sw.t0, np.array(alone_t0[:B]), equal_nan=True)
        assert np.array_equal(sw.state, np.array(alone_state[:B]))
        assert not sw.status.any()
    # the model agrees on the rules the reference does not define (stance NaN, last xy, NULL feet0)
    ms = state.copy()
    mref, mt0, mstat = M.advance(gait, fsteps, frame, ms, 3, 9, feet0=None if null_feet0 else feet0)
    assert np.array_equal(mt0, np.array(alone_t0), equal_nan=True) and not mstat.any()
    assert np.array_equal(np.isnan(mref), np.isnan(np.array(alone_ref)))
    st = np.array(alone_state)
    assert np.array_equal(st[:, :, 32:35], ms[:, :, 32:35])
    stance = gait[:, 0, 1:] != 0
    # world coordinates of magnitude < 4 (ulp 4.4e-16): cos / sin of ocml vs libm may differ by an ulp
    assert np.abs(st[stance][:, 35:37] - ms[stance][:, 35:37]).max() <= 4e-15
    assert np.array_equal(st[stance][:, :35], state[stance][:, :35])  # stance: mgoals, coefficients untouched


def test_host_and_device_pointers_same_bits(mpcq, eng, g):
    import torch
    B = 33
    gait, fsteps, frame, state, feet0 = _mixed_batch(g, B, seed=22)
    sw = mpcq.Swing(eng, B)
    sw.state[:] = state
    ref = sw.advance(gait, fsteps, frame, 0, 20, feet0=feet0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = {k: dev(v) for k, v in dict(gait=gait, fsteps=fsteps, frame=frame, state=state, feet0=feet0).items()}
    dref = torch.zeros((B, 20, 4, 9), dtype=torch.float64, device="cuda")
    dt0 = torch.zeros((B, 20, 4), dtype=torch.float64, device="cuda")
    dst = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    sw.advance_device(d["gait"].data_ptr(), d["fsteps"].data_ptr(), d["frame"].data_ptr(), d["state"].data_ptr(),
                      dref.data_ptr(), 0, 20, feet0_ptr=d["feet0"].data_ptr(), t0_ptr=dt0.data_ptr(),
                      status_ptr=dst.data_ptr(), asynchronous=False)
    assert np.array_equal(dref.cpu().numpy(), ref, equal_nan=True)
    assert np.array_equal(dt0.cpu().numpy(), sw.t0, equal_nan=True)
    assert np.array_equal(d["state"].cpu().numpy(), sw.state)
    assert not dst.cpu().numpy().any()
    # step: host and device
    Bs, args, st = _step_batch(g, 68)
    s2 = mpcq.Swing(eng, Bs)
    s2.state[:] = st
    out = s2.step(args)
    da, ds = dev(args), dev(st)
    do = torch.zeros((Bs, 4, 11), dtype=torch.float64, device="cuda")
    s2.step_device(da.data_ptr(), ds.data_ptr(), do.data_ptr(), asynchronous=False)
    assert np.array_equal(do.cpu().numpy(), out, equal_nan=True) and np.array_equal(ds.cpu().numpy(), s2.state)


def test_bad_gait_in_the_middle(mpcq, eng, g):
    gait, fsteps, frame, state, feet0 = _mixed_batch(g, 19, seed=23)
    good = mpcq.Swing(eng, 19)
    good.state[:] = state
    want = good.advance(gait, fsteps, frame, 0, 20, feet0=feet0)
    bad = gait.copy()
    bad[9] = g["trot_tick_gait"][1]
    assert (bad[9][0, 1:] == 0).any()
    f = int(np.flatnonzero(bad[9][0, 1:] == 0)[0])
    bad[9][:, 1 + f] = 0.0  # a swing foot without a stance row: the reference raises IndexError
    bad[17] = 0.0           # the empty table
    sw = mpcq.Swing(eng, 19)
    sw.state[:] = state
    ref = sw.advance(bad, fsteps, frame, 0, 20, feet0=feet0)
    assert sw.status[9] == mpcq.STATUS_BAD_GAIT and sw.status[17] == mpcq.STATUS_BAD_GAIT
    ok = np.ones(19, bool)
    ok[[9, 17]] = False
    assert not sw.status[ok].any()
    assert np.isnan(ref[~ok]).all() and np.isnan(sw.t0[~ok]).all()
    assert np.array_equal(sw.state[~ok], state[~ok])
    assert np.array_equal(ref[ok], want[ok], equal_nan=True) and np.array_equal(sw.state[ok], good.state[ok])
    _, _, mstat = M.advance(bad, fsteps, frame, state.copy(), 0, 20, feet0=feet0)
    assert np.array_equal(mstat, sw.status)


def test_invalid_arguments(mpcq, eng):
    B = 3
    lib = mpcq.lib()
    sp = mpcq.default_swing_params()
    a = {k: np.zeros(s) for k, s in dict(gait=(B, 20, 5), fsteps=(B, 20, 13), frame=(B, 3), state=(B, 4, 40),
                                         ref=(B, 20, 4, 9)).items()}
    a["gait"][:, 0, :] = 1.0
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731

    def call(k_sub0=0, n_sub=20, **null):
        v = {k: (None if k in null else a[k]) for k in a}
        return lib.mpcq_swing_batch(eng._h, C.byref(sp), B, k_sub0, n_sub, p(v["gait"]), p(v["fsteps"]), p(v["frame"]),
                                    None, p(v["state"]), p(v["ref"]), None, None, 0)

    assert call() == 0
    assert call(k_sub0=-1) == mpcq._lib.E_INVALID
    assert call(n_sub=0) == mpcq._lib.E_INVALID
    assert call(k_sub0=1, n_sub=20) == mpcq._lib.E_INVALID
    assert call(k_sub0=19, n_sub=2) == mpcq._lib.E_INVALID
    assert call(k_sub0=19, n_sub=1) == 0
    for k in a:
        assert call(**{k: True}) == mpcq._lib.E_INVALID, k
        assert len(lib.mpcq_last_error()) > 0
    assert lib.mpcq_swing_batch(None, C.byref(sp), B, 0, 20, p(a["gait"]), p(a["fsteps"]), p(a["frame"]), None,
                                p(a["state"]), p(a["ref"]), None, None, 0) == mpcq._lib.E_INVALID
    sin, sout = np.zeros((B, 4, 10)), np.zeros((B, 4, 11))
    assert lib.mpcq_swing_step_batch(eng._h, None, B, p(sin), p(a["state"]), p(sout), 0) == 0  # sp NULL = defaults
    for bad in ((None, a["state"], sout), (sin, None, sout), (sin, a["state"], None)):
        assert lib.mpcq_swing_step_batch(eng._h, C.byref(sp), B, p(bad[0]), p(bad[1]), p(bad[2]), 0) == mpcq._lib.E_INVALID
    with pytest.raises(mpcq.MpcqError):
        mpcq.Swing(eng, B).advance(a["gait"], a["fsteps"], a["frame"], k_sub0=5, n_sub=16)


def test_session_swing(mpcq):
    """1024 robots, N = 16, 24 ticks of the virtual robot with swing enabled: SV_SWING_REF is
    mpcq_swing_batch on the session's own gait / fsteps / frame (bit for bit), and the
    solve is untouched (a second session without swing gives the same bits)."""
    N, B, T = 16, 1024, 24
    rng = np.random.default_rng(31)
    v_ref = np.zeros((B, 6))
    v_ref[:, 0] = rng.uniform(-0.3, 0.8, B)
    v_ref[:, 1] = rng.uniform(-0.2, 0.2, B)
    v_ref[:, 5] = rng.uniform(-0.4, 0.4, B)
    with mpcq.Engine(N) as e1, mpcq.Engine(N) as e2, mpcq.Session(e1, B) as s1, mpcq.Session(e2, B) as s2:
        for what in (mpcq.SV_SWING_REF, mpcq.SV_SWING_STATE, mpcq.SV_FRAME):
            out = np.zeros(8)
            assert mpcq.lib().mpcq_session_read(s2._h, what, C.c_void_p(out.ctypes.data), 0) == mpcq._lib.E_INVALID
            ptr = C.c_void_p()
            assert mpcq.lib().mpcq_session_device_ptr(s2._h, what, C.byref(ptr)) == mpcq._lib.E_INVALID
            with pytest.raises(mpcq.MpcqError):
                s2.read(what)
        s1.enable_swing()
        assert not s1.read(mpcq.SV_SWING_STATE).any()
        sw = mpcq.Swing(e1, B)
        seen = 0
        for k in range(T):
            qw = s1.read(mpcq.SV_Q_W)
            s1.tick(v_ref)
            s2.tick(v_ref)
            frame = s1.read(mpcq.SV_FRAME)
            assert np.array_equal(frame, qw[:, [0, 1, 5]])  # q_w as it stood before this tick's update
            want = sw.advance(s1.read(mpcq.SV_GAIT), s1.read(mpcq.SV_FSTEPS), frame, 0, 20, feet0=None)
            got = s1.read(mpcq.SV_SWING_REF)
            assert got.shape == (B, 20, 4, 9)
            assert np.array_equal(got, want, equal_nan=True), k
            assert np.array_equal(s1.read(mpcq.SV_SWING_STATE), sw.state)
            seen += int(np.isfinite(got).sum())
            for what in (mpcq.SV_F0, mpcq.SV_X, mpcq.SV_ITERS, mpcq.SV_STATUS):
                assert np.array_equal(s1.read(what), s2.read(what)), (k, what)
        assert seen > B * 20 * 9  # the feet did swing
        # the references are read-only; the generators' state can be reset
        for what in (mpcq.SV_SWING_REF, mpcq.SV_FRAME):
            with pytest.raises(mpcq.MpcqError):
                s1.write(what, 0.0)
        s1.write(mpcq.SV_SWING_STATE, 0.0)
        assert not s1.read(mpcq.SV_SWING_STATE).any()


def test_drop_in_generator(mpcq, g):
    """mpc-tsid_amd/FootTrajectoryGenerator.py reproduces the step cases."""
    import FootTrajectoryGenerator as ftg
    n = g["step_in"].shape[0]
    gen = ftg.Foot_trajectory_generator(0.05, 0.05)
    assert gen.lastCoeffs == [0.0] * 24 and (gen.x1, gen.y1) == (0.0, 0.0)
    out, post = np.empty((n, 11)), np.empty((n, 26))
    for i in range(n):
        gen.lastCoeffs = list(g["step_pre"][i, :24])
        gen.x1, gen.y1 = g["step_pre"][i, 24], g["step_pre"][i, 25]
        out[i] = gen.get_next_foot(*g["step_in"][i], 0.001)
        post[i] = gen.lastCoeffs + [gen.x1, gen.y1]
    assert np.array_equal(out[:, 9:11], g["step_out"][:, 9:11]) and np.array_equal(post[:, 24:], g["step_post"][:, 24:])
    r = M.step_ratios(out, post[:, :24], g)
    print("drop-in generator / reference error over the reference's own (pos, vel, acc, coeffs):", r)
    assert (r <= M.TOL_FACTOR).all(), r
