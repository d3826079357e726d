"""GPU: the swing kernels (mpcq_swing_step_batch, mpcq_swing_batch, Session.enable_swing;
mpcq_swing.hip) under non-default mpcq_swing_params, against the unmodified reference captured
under the same parameters (tests/golden/swing_params_golden.npz, the cases of
tests/swing_param_cases.py) and the host model (tests/swing_model.py).

Tolerance rule (swing_model.TOL_FACTOR = 16): per class of quantity the bound is 16 x the
reference's own float64 - longdouble error on the fixtures of the *same case* (``<case>_step_err``
/ ``<case>_free_err``); t0, t_swing, the mode, gx / gy, NaN patterns, shapes and statuses are
exact.  test_swing_params_model.py shows on the CPU that a computation which ignores any moved
field misses these fixtures by more than 100 x that bound (or in an exact quantity).  Every test
prints its measured ratios before asserting."""
import ctypes as C

import numpy as np
import pytest

import swing_model as M
import swing_param_cases as SC

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


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
    return SC.load_golden()


def _fill_feet0(f0, rng):
    f0 = f0.copy()
    m = np.isnan(f0)
    f0[m] = rng.normal(0, 1, int(m.sum()))  # read at lift-off only: anything elsewhere
    return f0


# ----------------------------------------------------------------------------- step cases
def _step_batch(v):
    """All step cases of a case as feet of n // 4 + 1 robots: the tail (at least one foot) is
    padded by t0 = NaN and must stay as it is."""
    n = v["step_in"].shape[0]
    B = n // 4 + 1
    args = np.full((B * 4, 10), np.nan)
    state = np.zeros((B * 4, M.STATE))
    args[:n] = v["step_in"]
    state[:n, :26] = v["step_pre"]
    state[n:, :37] = 5.0
    return n, B, args.reshape(B, 4, 10), state.reshape(B, 4, M.STATE)


@pytest.mark.parametrize("case", SC.NAMES)
def test_step_cases_under_params(mpcq, eng, g, case):
    v = SC.case_view(g, case)
    n, B, args, state = _step_batch(v)
    sw = mpcq.Swing(eng, B, mpcq.default_swing_params(**SC.CASES[case]))
    sw.state[:] = state
    out = sw.step(args).reshape(B * 4, 11)
    post, pre = sw.state.reshape(B * 4, M.STATE), state.reshape(B * 4, M.STATE)
    assert np.isnan(out[n:]).all() and np.array_equal(post[n:], pre[n:])  # the padded feet
    assert np.array_equal(out[:n, 9:11], v["step_out"][:, 9:11])  # gx, gy
    assert np.array_equal(post[:n, 24:26], v["step_post"][:, 24:26])  # x1, y1
    assert np.array_equal(post[:n, 34] == 1.0, v["step_mode"])
    assert np.array_equal(post[:n, 26:34], pre[:n, 26:34]) and np.array_equal(post[:n, 35:], pre[:n, 35:])
    lock = ~v["step_mode"]
    assert lock.any() and np.array_equal(post[:n, :26][lock], v["step_pre"][lock])  # locked: slots 0..25 untouched
    r = M.step_ratios(out[:n], post[:n, :24], v)
    print(f"{case} step B={B}: kernel / reference error over the reference's own (pos, vel, acc, coeffs): {r}")
    assert (r <= M.TOL_FACTOR).all(), r


# ----------------------------------------------------------------------------- free running
@pytest.mark.parametrize("case", SC.NAMES)
def test_free_running_under_params(mpcq, eng, g, case):
    v, K = SC.case_view(g, case), SC.full(case)["k_mpc"]
    sp = mpcq.default_swing_params(**SC.CASES[case])
    T = SC.TICKS
    rng = np.random.default_rng(13)
    # trot, the frame moving every substep: n_sub = 1 calls with the recorded frames
    k = lambda f: v[f"trot_sub_{f}"]  # noqa: E731
    sw = mpcq.Swing(eng, 1, sp)
    ref = np.empty((T, K, 4, 9))
    for j in range(T):
        swing = k("gait")[j][0, 1:] == 0
        for ks in range(K):
            r = sw.advance(k("gait")[j][None], k("fsteps")[j][None], k("frame")[j, ks][None], ks, 1,
                           feet0=_fill_feet0(k("feet0")[j, ks], rng)[None])
            assert r.shape == (1, 1, 4, 9) and not sw.status.any()
            assert np.array_equal(sw.t0[0, 0], k("t0")[j, ks], equal_nan=True)
            assert np.array_equal(np.isnan(sw.t0[0, 0]), ~swing)
            assert np.array_equal(sw.state[0, swing, 32], k("t_swing")[j, ks][swing])
            assert np.array_equal(sw.state[0, swing, 34], k("mode")[j, ks][swing])
            assert np.array_equal(sw.state[0, swing, 33], k("t0")[j, ks][swing])
            assert np.isnan(r[0, 0][~swing]).all()
            ref[j, ks] = r[0, 0]
    ratios = M.error_ratios(ref, k("ref"), v["free_err"])
    print(f"{case} trot, per substep: kernel / reference error over the reference's own (pos, vel, acc): {ratios}")
    assert (ratios <= M.TOL_FACTOR).all(), ratios

    # trot and bound in one batch, the frame held per tick: one n_sub = k_mpc call per tick;
    # substeps 0..2 then 3..k_mpc-1 (a split inside an output chunk) give the single call's bits
    names = ("trot", "bound")
    st = lambda f, j: np.ascontiguousarray(np.stack([v[f"{s}_tick_{f}"][j] for s in names]))  # noqa: E731
    one, two = mpcq.Swing(eng, 2, sp), mpcq.Swing(eng, 2, sp)
    ref = np.empty((2, T, K, 4, 9))
    for j in range(T):
        gait, fsteps, frame = st("gait", j), st("fsteps", j), st("frame", j)[:, 0]
        feet0 = _fill_feet0(st("feet0", j)[:, 0], rng)  # a swing lifts off on substep 0
        ref[:, j] = one.advance(gait, fsteps, frame, feet0=feet0)  # n_sub None: up to k_mpc
        assert one.t0.shape == (2, K, 4) and not one.status.any()
        assert np.array_equal(one.t0, st("t0", j), equal_nan=True)
        swing = gait[:, 0, 1:] == 0
        assert np.array_equal(one.state[:, :, 32][swing], st("t_swing", j)[:, K - 1][swing])
        assert np.array_equal(one.state[:, :, 34][swing], st("mode", j)[:, K - 1][swing])
        assert np.array_equal(one.state[:, :, 33][swing], st("t0", j)[:, K - 1][swing])
        assert np.isnan(ref[:, j][~np.broadcast_to(swing[:, None, :], (2, K, 4))]).all()
        ra = two.advance(gait, fsteps, frame, 0, 3, feet0=feet0)
        ta = two.t0.copy()
        rb = two.advance(gait, fsteps, frame, 3, K - 3, feet0=feet0)
        assert np.array_equal(np.concatenate([ra, rb], 1), ref[:, j], equal_nan=True)
        assert np.array_equal(np.concatenate([ta, two.t0], 1), one.t0, equal_nan=True)
        assert np.array_equal(two.state, one.state)
    want = np.stack([v[f"{s}_tick_ref"] for s in names])
    ratios = M.error_ratios(ref, want, v["free_err"])
    print(f"{case} trot + bound, a tick per call: kernel / reference error over the reference's own (pos, vel, acc): {ratios}")
    assert (ratios <= M.TOL_FACTOR).all(), ratios


# ----------------------------------------------------------------------------- layout
def _mixed_batch(v, B, seed):
    """B robots from the case's tick tables (trot and bound alternating, ticks 1, 2, ...) with a
    random, mid-swing generator state."""
    rng = np.random.default_rng(seed)
    s = [("trot", "bound")[b % 2] for b in range(B)]
    j = [1 + b % (SC.TICKS - 1) for b in range(B)]
    gait = np.stack([v[f"{n}_tick_gait"][t] for n, t in zip(s, j)])
    fsteps = np.stack([v[f"{n}_tick_fsteps"][t] for n, t in zip(s, j)])
    frame = np.stack([v[f"{n}_tick_frame"][t, 0] for n, t in zip(s, j)])
    state = np.zeros((B, 4, M.STATE))
    state[:, :, :37] = rng.normal(0, 0.1, (B, 4, 37))
    feet0 = rng.normal(0, 0.1, (B, 4, 6))
    return gait, fsteps, frame, state, feet0


@pytest.mark.parametrize("case", ["k30", "all"])
def test_layout_under_params(mpcq, eng, g, case):
    """17 robots (a full workgroup and a one-robot one) with k_mpc != 20: each robot gets the
    bits it gets alone, host and device pointers the same bits, ref is [B][k_mpc][4][9], and a
    call of n_sub < k_mpc substeps writes B * n_sub rows and nothing beyond them."""
    import torch
    v, K, B = SC.case_view(g, case), SC.full(case)["k_mpc"], 17
    sp = mpcq.default_swing_params(**SC.CASES[case])
    gait, fsteps, frame, state, feet0 = _mixed_batch(v, B, seed=51)
    assert len({gait[b].tobytes() for b in range(B)}) > 4  # the robots differ
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d = {k: dev(a) for k, a in dict(gait=gait, fsteps=fsteps, frame=frame, feet0=feet0).items()}
    for null_feet0 in (False, True):
        f0 = lambda s: None if null_feet0 else feet0[s]  # noqa: E731
        alone_ref, alone_t0, alone_state = [], [], []
        for b in range(B):
            sw = mpcq.Swing(eng, 1, sp)
            sw.state[:] = state[b]
            alone_ref.append(sw.advance(gait[b:b + 1], fsteps[b:b + 1], frame[b:b + 1], feet0=f0(slice(b, b + 1)))[0])
            alone_t0.append(sw.t0[0])
            alone_state.append(sw.state[0].copy())
            assert not sw.status.any()
        alone_ref, alone_t0, alone_state = np.array(alone_ref), np.array(alone_t0), np.array(alone_state)
        assert np.isfinite(alone_ref).any() and np.isnan(alone_ref).any()
        sw = mpcq.Swing(eng, B, sp)
        sw.state[:] = state
        ref = sw.advance(gait, fsteps, frame, feet0=f0(slice(None)))
        assert ref.shape == (B, K, 4, 9) and sw.t0.shape == (B, K, 4)
        assert np.array_equal(ref, alone_ref, equal_nan=True)
        assert np.array_equal(sw.t0, alone_t0, equal_nan=True)
        assert np.array_equal(sw.state, alone_state) and not sw.status.any()
        # the model agrees on t0, the stance NaNs and the timing slots of the state
        ms = state.copy()
        mref, mt0, mstat = M.advance(gait, fsteps, frame, ms, feet0=f0(slice(None)), params=SC.CASES[case])
        assert mref.shape == ref.shape and not mstat.any()
        assert np.array_equal(mt0, sw.t0, equal_nan=True) and np.array_equal(np.isnan(mref), np.isnan(ref))
        assert np.array_equal(sw.state[:, :, 32:35], ms[:, :, 32:35])
        # device pointers: the same bits
        dstate = dev(state)
        dref = torch.full((B, K, 4, 9), SENTINEL, dtype=torch.float64, device="cuda")
        dt0 = torch.full((B, K, 4), SENTINEL, dtype=torch.float64, device="cuda")
        dst = torch.full((B,), 7, dtype=torch.int32, device="cuda")
        sw.advance_device(d["gait"].data_ptr(), d["fsteps"].data_ptr(), d["frame"].data_ptr(), dstate.data_ptr(),
                          dref.data_ptr(), feet0_ptr=0 if null_feet0 else d["feet0"].data_ptr(), t0_ptr=dt0.data_ptr(),
                          status_ptr=dst.data_ptr(), asynchronous=False)
        assert np.array_equal(dref.cpu().numpy(), ref, equal_nan=True)
        assert np.array_equal(dt0.cpu().numpy(), sw.t0, equal_nan=True)
        assert np.array_equal(dstate.cpu().numpy(), sw.state) and not dst.cpu().numpy().any()
        # n_sub < k_mpc into poisoned arrays of the full size: rows are [B][n_sub], written exactly
        k0, n = 1, K - 2
        part = mpcq.Swing(eng, B, sp)
        part.state[:] = state
        want = part.advance(gait, fsteps, frame, k0, n, feet0=f0(slice(None)))
        assert want.shape == (B, n, 4, 9)
        dstate = dev(state)
        dref.fill_(SENTINEL)
        dt0.fill_(SENTINEL)
        sw.advance_device(d["gait"].data_ptr(), d["fsteps"].data_ptr(), d["frame"].data_ptr(), dstate.data_ptr(),
                          dref.data_ptr(), k0, n, feet0_ptr=0 if null_feet0 else d["feet0"].data_ptr(),
                          t0_ptr=dt0.data_ptr(), asynchronous=False)
        flat, flat0 = dref.cpu().numpy().ravel(), dt0.cpu().numpy().ravel()
        assert np.array_equal(flat[:B * n * 36].reshape(B, n, 4, 9), want, equal_nan=True)
        assert np.array_equal(flat0[:B * n * 4].reshape(B, n, 4), part.t0, equal_nan=True)
        assert (flat[B * n * 36:] == SENTINEL).all() and (flat0[B * n * 4:] == SENTINEL).all()
        assert not (flat[:B * n * 36] == SENTINEL).any() and not (flat0[:B * n * 4] == SENTINEL).any()
        assert np.array_equal(dstate.cpu().numpy(), part.state)


# ----------------------------------------------------------------------------- arguments
def test_argument_bounds_follow_k_mpc(mpcq, eng):
    B = 3
    lib, E = mpcq.lib(), mpcq._lib.E_INVALID
    a = {k: np.zeros(s) for k, s in dict(gait=(B, 20, 5), fsteps=(B, 20, 13), frame=(B, 3), state=(B, 4, 40),
                                         ref=(B, 40, 4, 9), sin=(B, 4, 10), sout=(B, 4, 11)).items()}
    a["gait"][:, 0, :] = 1.0
    p = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731

    def batch(sp, k_sub0, n_sub):
        return lib.mpcq_swing_batch(eng._h, C.byref(sp), B, k_sub0, n_sub, p(a["gait"]), p(a["fsteps"]), p(a["frame"]),
                                    None, p(a["state"]), p(a["ref"]), None, None, 0)

    def step(sp):
        return lib.mpcq_swing_step_batch(eng._h, C.byref(sp), B, p(a["sin"]), p(a["state"]), p(a["sout"]), 0)

    sp7, sp30 = mpcq.default_swing_params(**SC.CASES["all"]), mpcq.default_swing_params(**SC.CASES["k30"])
    assert sp7.k_mpc == 7 and sp30.k_mpc == 30
    assert batch(sp7, 0, 8) == E and batch(sp7, 1, 7) == E and batch(sp7, 7, 1) == E and batch(sp7, 5, 3) == E
    assert "k_mpc (7)" in lib.mpcq_last_error().decode()
    assert batch(sp7, 0, 7) == 0 and batch(sp7, 1, 6) == 0 and batch(sp7, 6, 1) == 0 and batch(sp7, 4, 3) == 0
    assert batch(sp30, 0, 30) == 0 and batch(sp30, 29, 1) == 0 and batch(sp30, 20, 10) == 0
    assert batch(sp30, 0, 31) == E and batch(sp30, 30, 1) == E
    with pytest.raises(mpcq.MpcqError):
        mpcq.Swing(eng, B, sp7).advance(a["gait"], a["fsteps"], a["frame"], k_sub0=0, n_sub=8)
    with pytest.raises(mpcq.MpcqError):
        mpcq.Swing(eng, B, sp7).advance(a["gait"], a["fsteps"], a["frame"], k_sub0=7)  # n_sub = 0

    # parameters no entry point accepts; nothing is launched: the poisoned arrays stay as they are
    bad = [dict(dt=0.0), dict(dt=float("nan")), dict(dt=-0.001), dict(k_mpc=0), dict(k_mpc=-3), dict(t_lock=-1.0),
           dict(t_lock=float("nan"))]
    with mpcq.Engine(16) as e2, mpcq.Session(e2, B) as sess:
        for ov in bad:
            sp = mpcq.default_swing_params(**ov)
            for k in ("state", "ref", "sout"):
                a[k][:] = SENTINEL
            keep = {k: x.copy() for k, x in a.items()}
            for entry in ("step", "batch", "session"):
                assert batch(sp7, 0, 8) == E and b"swing needs" not in lib.mpcq_last_error()  # another message first
                rc = (step(sp) if entry == "step" else batch(sp, 0, 1) if entry == "batch"
                      else lib.mpcq_session_enable_swing(sess._h, C.byref(sp)))
                assert rc == E, (ov, entry)
                assert b"swing needs" in lib.mpcq_last_error(), (ov, entry)
            assert all(np.array_equal(a[k], keep[k]) for k in a), ov
            with pytest.raises(mpcq.MpcqError):
                sess.enable_swing(sp)
            assert sess.swing_params is None
            with pytest.raises(mpcq.MpcqError):  # swing is still off: no arrays
                sess.read(mpcq.SV_SWING_REF)
            ptr = C.c_void_p()
            assert lib.mpcq_session_device_ptr(sess._h, mpcq.SV_SWING_REF, C.byref(ptr)) == E
        for k in ("state", "ref", "sout"):
            a[k][:] = 0.0
        # the session is as good as new: valid parameters enable it
        sess.enable_swing(sp7)
        sess.tick(np.tile([0.3, 0, 0, 0, 0, 0], (B, 1)))
        assert sess.read(mpcq.SV_SWING_REF).shape == (B, 7, 4, 9)
        assert (sess.read(mpcq.SV_STATUS) == mpcq.STATUS_SOLVED).all()


# ----------------------------------------------------------------------------- sessions
@pytest.mark.parametrize("name", list(SC.SESSIONS))
def test_session_swing_under_params(mpcq, g, name):
    """17 virtual robots in mixed trot / bound / pace, 6 ticks, swing enabled with k_mpc != 20:
    n16 is N = 16 with case ``all`` (k_mpc = 7), n8 the reference's other time base (Engine(8,
    dt=0.04), planner dt 0.04, swing dt 0.001, k_mpc 40, max_height 0.08, t_lock 0.03, feet_z
    0.017).  Per tick SV_SWING_REF is [B][k_mpc][4][9], equals Swing.advance on the session's own
    gait / fsteps / frame bit for bit, and agrees with the host model on the same arrays: t0,
    t_swing, the mode and NaN patterns exactly, the polynomials within TOL_FACTOR x the yardstick.
    The yardstick of n16 is case ``all``'s free_err (the reference's own rounding error).  n8 has
    no fixture of the reference; its yardstick is the model's own float64 - longdouble error on
    this session's inputs as the oracle's closed loop produces them on the CPU, 1.2e-11 m,
    4.0e-10 m/s, 4.6e-8 m/s^2 (swing_param_cases.SESSION_N8_YARD, recomputed by
    test_swing_params_model.py::test_session_inputs_and_their_yardstick).  The solve is untouched
    (a twin session without swing gives the same f0, x, iterations, status); robot 9's table has
    no terminator (BAD_GAIT) and its neighbours' references equal those of a session without it."""
    c = SC.SESSIONS[name]
    N, B, T, bad = c["N"], SC.SESSION_B, SC.SESSION_TICKS, SC.SESSION_BAD
    ov = c["swing"]
    K = ov["k_mpc"]
    yard = g["all_free_err"] if name == "n16" else SC.SESSION_N8_YARD
    sp = mpcq.default_swing_params(**ov)
    good = SC.session_gaits(N)
    gaits = good.copy()
    gaits[bad, :, 0] = 1.0  # no terminator: the planner reports BAD_GAIT
    v_ref = SC.session_v_ref()
    ok = np.arange(B) != bad
    pp = lambda: mpcq.default_planner_params(dt=c["dt"])  # noqa: E731
    with mpcq.Engine(N, dt=c["dt"]) as e1, mpcq.Engine(N, dt=c["dt"]) as e2, mpcq.Engine(N, dt=c["dt"]) as e3, \
            mpcq.Session(e1, B, gait0=gaits, planner_params=pp()) as s1, \
            mpcq.Session(e2, B, gait0=gaits, planner_params=pp()) as s2, \
            mpcq.Session(e3, B, gait0=good, planner_params=pp()) as s3:
        s1.enable_swing(sp)
        s3.enable_swing(sp)
        assert s1.read(mpcq.SV_SWING_REF).shape == (B, K, 4, 9) and not s1.read(mpcq.SV_SWING_STATE).any()
        sw = mpcq.Swing(e1, B, sp)
        ms = np.zeros((B, 4, M.STATE))
        modes, lifts, worst = set(), 0, np.zeros(3)

        def tick(k):
            qw = s1.read(mpcq.SV_Q_W)
            for s in (s1, s2, s3):
                s.tick(v_ref)
            frame = s1.read(mpcq.SV_FRAME)
            assert np.array_equal(frame, qw[:, [0, 1, 5]])  # q_w as it stood before this tick's update
            got = s1.read(mpcq.SV_SWING_REF)
            assert got.shape == (B, K, 4, 9)
            for what in (mpcq.SV_F0, mpcq.SV_X):  # the bad robot's are NaN in both
                assert np.array_equal(s1.read(what), s2.read(what), equal_nan=True), (k, what)
                assert np.isfinite(s1.read(what)[ok]).all(), (k, what)
            for what in (mpcq.SV_ITERS, mpcq.SV_STATUS):
                assert np.array_equal(s1.read(what), s2.read(what)), (k, what)
            status = s1.read(mpcq.SV_STATUS)
            assert status[bad] == mpcq.STATUS_BAD_GAIT and (status[ok] == mpcq.STATUS_SOLVED).all(), status
            # the neighbours of the bad robot: as in a session without it
            assert np.array_equal(got[ok], s3.read(mpcq.SV_SWING_REF)[ok], equal_nan=True), k
            assert np.array_equal(s1.read(mpcq.SV_SWING_STATE)[ok], s3.read(mpcq.SV_SWING_STATE)[ok])
            assert not np.isfinite(got[bad][..., [0, 1]]).any()  # no fsteps: it has no target to swing to
            return s1.read(mpcq.SV_GAIT), s1.read(mpcq.SV_FSTEPS), frame, got

        for k in range(T):
            gait, fsteps, frame, got = tick(k)
            want = sw.advance(gait, fsteps, frame, feet0=None)
            assert want.shape == (B, K, 4, 9) and not sw.status.any()
            assert np.array_equal(got, want, equal_nan=True), k
            assert np.array_equal(s1.read(mpcq.SV_SWING_STATE), sw.state, equal_nan=True)
            assert np.isfinite(sw.state[ok]).all()  # NaN only where the bad robot swings without a target
            mref, mt0, mstat = M.advance(gait, fsteps, frame, ms, feet0=None, params=ov)
            assert mref.shape == got.shape and not mstat.any()
            assert np.array_equal(mt0, sw.t0, equal_nan=True) and np.array_equal(np.isnan(mref), np.isnan(got))
            assert np.array_equal(sw.state[:, :, 32:35], ms[:, :, 32:35])  # t_swing, t0, the mode
            swing = gait[:, 0, 1:] == 0
            assert np.array_equal(np.isnan(got[ok][:, 0, :, 0]), ~swing[ok])
            r = M.error_ratios(got, mref, yard)
            worst = np.maximum(worst, r)
            modes |= set(sw.state[:, :, 34][swing].tolist())
            lifts += int((mt0[:, 0] == 0).sum())
        print(f"session {name} (k_mpc {K}): kernel / model error over the yardstick {yard} (pos, vel, acc): {worst}")
        assert modes == {0.0, 1.0} and lifts >= B - 1
        assert (worst <= M.TOL_FACTOR).all(), worst

        # again with the same k_mpc and another max_height: the next tick's z follows it
        h2 = 1.5 * ov["max_height"]
        sp2 = mpcq.default_swing_params(**dict(ov, max_height=h2))
        s1.enable_swing(sp2)
        s3.enable_swing(sp2)
        old = mpcq.Swing(e1, B, sp)
        old.state[:] = sw.state
        sw.params = sp2
        gait, fsteps, frame, got = tick(T)
        want = sw.advance(gait, fsteps, frame, feet0=None)
        assert np.array_equal(got, want, equal_nan=True) and np.array_equal(s1.read(mpcq.SV_SWING_STATE), sw.state, equal_nan=True)
        was = old.advance(gait, fsteps, frame, feet0=None)
        fin = np.isfinite(got[..., 2])
        assert fin.sum() >= K * 4 and np.array_equal(fin, np.isfinite(was[..., 2]))
        xy = [0, 1, 3, 4, 6, 7]
        assert np.array_equal(got[..., xy], was[..., xy], equal_nan=True)  # x and y do not read max_height
        z2, z1 = got[..., 2][fin] - ov["feet_z"], was[..., 2][fin] - ov["feet_z"]
        big = np.abs(z1) > 1e-4
        assert big.sum() >= K and np.abs(z2[big] / z1[big] - 1.5).max() < 1e-9
        # another k_mpc: refused, and the session goes on as it was
        for s in (s1, s3):
            with pytest.raises(mpcq.MpcqError) as ei:
                s.enable_swing(mpcq.default_swing_params(**dict(ov, k_mpc=K + 1)))
            assert ei.value.code == mpcq._lib.E_INVALID
            assert s.swing_params is sp2
        gait, fsteps, frame, got = tick(T + 1)
        want = sw.advance(gait, fsteps, frame, feet0=None)
        assert got.shape == (B, K, 4, 9) and np.array_equal(got, want, equal_nan=True)
        assert np.array_equal(s1.read(mpcq.SV_SWING_STATE), sw.state, equal_nan=True)


# ----------------------------------------------------------------------------- drop-in generator
@pytest.mark.parametrize("case", SC.NAMES)
def test_drop_in_generator_under_params(mpcq, g, case):
    """mpc-tsid_amd/FootTrajectoryGenerator.py constructed with the case's (max_height, t_lock) and
    stepped with its dt reproduces the case's step fixtures."""
    import FootTrajectoryGenerator as ftg
    v, p = SC.case_view(g, case), SC.full(case)
    n = v["step_in"].shape[0]
    gen = ftg.Foot_trajectory_generator(p["max_height"], p["t_lock"])
    out, post = np.empty((n, 11)), np.empty((n, 26))
    for i in range(n):
        gen.lastCoeffs = list(v["step_pre"][i, :24])
        gen.x1, gen.y1 = v["step_pre"][i, 24], v["step_pre"][i, 25]
        out[i] = gen.get_next_foot(*v["step_in"][i], p["dt"])
        post[i] = gen.lastCoeffs + [gen.x1, gen.y1]
    assert np.array_equal(out[:, 9:11], v["step_out"][:, 9:11]) and np.array_equal(post[:, 24:], v["step_post"][:, 24:])
    lock = ~v["step_mode"]
    assert np.array_equal(post[lock], v["step_pre"][lock])
    r = M.step_ratios(out, post[:, :24], v)
    print(f"{case} drop-in generator / reference error over the reference's own (pos, vel, acc, coeffs): {r}")
    assert (r <= M.TOL_FACTOR).all(), r
