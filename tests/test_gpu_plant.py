"""GPU: the rigid-body plant (mpcq_plant_step_batch, mpcq_session_enable_plant) against its
host model (tests/plant_model.py), and what a session promises around it.

Tolerance of every comparison with the model: 1e-12 absolute on states, bit equality on the
effective forces.  Kernel and model evaluate the same float64 operations in the same order
without contraction; what may differ is the device library's sin / cos against numpy's (the
planner tests hold those to 1e-15 per evaluation) and the one fma of the world pose.  Twenty
substeps of O(1) quantities stay far below 1e-12, and a formula error is 1e-6 or more.
Measured on an MI355X: 4.4e-15 at worst on the batch entry point, 6.9e-18 over the session
ticks, whose angles stay near zero.  Everything else here is bit
equality, except MPCQ_SV_ORDER, whose order inside a bucket is arbitrary by design."""
import ctypes as C
import itertools

import numpy as np
import pytest

import plant_model as PM

pytestmark = pytest.mark.gpu

TOL = 1e-12
N, SB = 16, 65  # the sessions: horizon and batch (two blocks, the second with one robot)
V_REF = np.array([0.3, 0.1, 0.0, 0.0, 0.0, 0.4])
SV = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_L_FEET", "SV_Q_W", "SV_COST",
      "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_ROT_FLAG", "SV_H_ROT", "SV_X_ROBOT", "SV_ORDER", "SV_FIRST")


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.fixture(scope="module")
def eng(mpcq):
    with mpcq.Engine(N) as e:
        yield e


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _snap(mpcq, sess, names=SV):
    return {n: sess.read(getattr(mpcq, n)).copy() for n in names}


def _gaits(B):
    from mpcq import synth
    return np.stack([synth.gait_table(("trot", "bound")[b % 2], N) for b in range(B)])


def _batch(mpcq, B, seed):
    """Random robots: roll / pitch within 0.3 rad, any yaw; swing feet (NaN in some coordinate),
    robots with no stance foot and with four; negative fz and out-of-cone tangentials."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 12))
    x[:, 0:3] = rng.uniform(-.3, .3, (B, 3)) + [0.0, 0.0, 0.2]
    x[:, 3:5] = rng.uniform(-.3, .3, (B, 2))
    x[:, 5] = rng.uniform(-np.pi, np.pi, B)
    x[:, 6:12] = rng.uniform(-1.0, 1.0, (B, 6))
    feet = np.tile(np.vstack([PM.SHOULDERS, np.zeros((1, 4))]), (B, 1, 1)) + rng.uniform(-.05, .05, (B, 3, 4))
    swing = rng.random((B, 4)) < 0.4
    swing[0] = True  # no stance foot
    swing[B // 2] = False
    for b, q in zip(*np.nonzero(swing)):
        feet[b, rng.integers(3), q] = np.nan
    f = rng.uniform(-12.0, 12.0, (B, 12))
    f[:, 2::3] = rng.uniform(-5.0, 32.0, (B, 4))
    wrench = rng.uniform(-5.0, 5.0, (B, 6))
    table = mpcq.robots(B, mass=rng.uniform(2.0, 4.0, B), mu=rng.uniform(.4, 1.0, B), fz_max=rng.uniform(15.0, 30.0, B),
                        gI=PM.GI * rng.uniform(.8, 1.3, (B, 1, 1)))
    return x, feet, f, wrench, table


COMBOS = list(itertools.product((0, 1), (False, True), (False, True), (1, 7, 20), (PM.MODEL, PM.RIGID)))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_step_batch_vs_model(mpcq, eng, B):
    x, feet, f, wrench, table = _batch(mpcq, B, 100 + B)
    worst = 0.0
    for clamp, use_w, use_r, n_sub, integ in COMBOS:
        ctx = (B, clamp, use_w, use_r, n_sub, integ)
        pl = mpcq.Plant(eng, mpcq.default_plant_params(clamp=clamp, n_sub=n_sub, integrator=integ))
        out, fe = pl.step(x, feet, f, wrench if use_w else None, table if use_r else None)
        want, wfe = PM.step(x, feet, f, wrench if use_w else None, PM.from_table(table) if use_r else None,
                            clamp=clamp, n_sub=n_sub, integrator=integ)
        assert _same(fe, wfe), ctx
        assert np.isfinite(out).all(), ctx
        d = float(np.abs(out - want).max())
        worst = max(worst, d)
        assert d <= TOL, (ctx, d)
    print(f"B={B}: max |kernel - model| = {worst:.2e}")


def test_step_alias_device_async_and_nan(mpcq, eng):
    import torch
    B = 130
    x, feet, f, wrench, table = _batch(mpcq, B, 7)
    pl = mpcq.Plant(eng)
    out, fe = pl.step(x, feet, f, wrench, table)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda")  # noqa: E731
    back = lambda t: t.cpu().numpy().view(np.float64).reshape(B, 12)  # noqa: E731
    dx, dfeet, df, dw, dt = dev(x), dev(feet), dev(f), dev(wrench), dev(table)
    dout, dfe = torch.zeros_like(dx), torch.zeros_like(df)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    eng.set_stream(stream.cuda_stream)
    try:
        # device pointers, asynchronous: bit-equal to the host path
        pl.step_device(B, dx.data_ptr(), dfeet.data_ptr(), df.data_ptr(), dout.data_ptr(), dfe.data_ptr(),
                       dw.data_ptr(), dt.data_ptr())
        # state_out aliasing state
        pl.step_device(B, dx.data_ptr(), dfeet.data_ptr(), df.data_ptr(), dx.data_ptr(), 0, dw.data_ptr(),
                       dt.data_ptr())
        stream.synchronize()
    finally:
        eng.set_stream(None)
    assert _same(back(dout), out) and _same(back(dfe), fe)
    assert _same(back(dx), out)
    # a NaN force on one robot: its neighbours are bit-identical
    f2 = f.copy()
    b = B // 2  # four stance feet
    f2[b, 4] = np.nan
    out2, fe2 = pl.step(x, feet, f2, wrench, table)
    keep = np.arange(B) != b
    assert _same(out2[keep], out[keep]) and _same(fe2[keep], fe[keep])
    assert np.isnan(out2[b]).any() and np.isnan(fe2[b, 4])
    want, wfe = PM.step(x, feet, f2, wrench, PM.from_table(table))
    assert _same(fe2, wfe) and np.array_equal(np.isnan(out2), np.isnan(want))


def test_step_invalid_arguments(mpcq, eng):
    from mpcq import _lib as L
    lib = L.lib()
    B = 3
    x, feet, f, wrench, table = _batch(mpcq, B, 1)
    out = np.empty((B, 12))
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(pl, state=x, ft=feet, ff=f, so=out, robots=None):
        return lib.mpcq_plant_step_batch(eng._h, C.byref(pl), B, None if state is None else p(state),
                                         None if ft is None else p(ft), None if ff is None else p(ff), None,
                                         None if robots is None else p(robots), None if so is None else p(so), None, 0)
    ok = mpcq.default_plant_params()
    out[:] = -7.0
    for bad in (dict(dt=0.0), dict(dt=-0.02), dict(n_sub=0), dict(integrator=2), dict(integrator=-1)):
        assert call(mpcq.default_plant_params(**bad)) == L.E_INVALID, bad
    for kw in (dict(state=None), dict(ft=None), dict(ff=None), dict(so=None)):
        assert call(ok, **kw) == L.E_INVALID, kw
    bad_table = table.copy()
    bad_table["mass"][1] = -1.0
    assert call(ok, robots=bad_table) == L.E_INVALID  # a host table is validated
    assert (out == -7.0).all()  # nothing was launched
    assert call(ok) == 0 and np.isfinite(out).all()
    with mpcq.Session(eng, 2) as sess:
        with pytest.raises(mpcq.MpcqError):
            sess.plant_read(mpcq.PV_STATE_END)  # no plant yet
        with pytest.raises(mpcq.MpcqError):
            sess.enable_plant(mpcq.default_plant_params(dt=0.01))  # not the context's dt
        with pytest.raises(mpcq.MpcqError):
            sess.enable_plant(mpcq.default_plant_params(n_sub=0))
        sess.enable_plant()
        assert not sess.plant_read(mpcq.PV_STATE_END).any()
        buf = np.empty((2, 12))
        assert lib.mpcq_session_plant_read(sess._h, 3, p(buf), 0) == L.E_INVALID
        assert lib.mpcq_session_plant_read(sess._h, 0, None, 0) == L.E_INVALID


# ------------------------------------------------------------------------------- sessions
def _run(mpcq, eng, ticks, setup=None, before=None, names=SV, plant_names=()):
    """A virtual-robot session of SB robots over `ticks` ticks; setup(sess) after create,
    before(sess, k) ahead of tick k.  Returns the snapshots after every tick."""
    out = []
    with mpcq.Session(eng, SB, gait0=_gaits(SB)) as sess:
        if setup:
            setup(sess)
        for k in range(ticks):
            if before:
                before(sess, k)
            sess.tick(V_REF)
            snap = _snap(mpcq, sess, names)
            for n in plant_names:
                snap[n] = sess.plant_read(getattr(mpcq, n))
            out.append(snap)
    return out


def test_session_model_plant_tracks_the_prediction(mpcq, eng):
    """PLANT_MODEL without clamp, tables or wrench is the MPC's own step: the plant ends every
    tick where the QP predicted, up to OSQP's residual (5e-5, tests/test_plant_model.py)."""
    pl = mpcq.default_plant_params(integrator=mpcq.PLANT_MODEL, clamp=0)
    runs = _run(mpcq, eng, 8, setup=lambda s: s.enable_plant(pl), names=("SV_STATUS", "SV_X_ROBOT"),
                plant_names=("PV_STATE_END",))
    worst = 0.0
    for k, r in enumerate(runs):
        assert (r["SV_STATUS"] == 1).all(), (k, r["SV_STATUS"])
        d = np.abs(r["PV_STATE_END"] - r["SV_X_ROBOT"][:, :, 0]).max(axis=1)
        worst = max(worst, float(d.max()))
        assert (d <= 5e-5).all(), (k, d.max(), int(d.argmax()))
    print(f"max |PV_STATE_END - x_robot[:, 0]| = {worst:.2e}")


def _plant_table(mpcq):
    mass = np.full(SB, PM.MASS)
    mass[1::2] *= 1.4  # a payload the controller does not know about
    return mpcq.robots(SB, mass=mass)


def _wrench():
    w = np.zeros((SB, 6))
    w[1] = [6.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    w[4] = [0.0, -4.0, 1.0, 0.1, 0.0, -0.2]
    w[64] = [-3.0, 2.0, 0.0, 0.0, 0.3, 0.0]
    return w


def _check_tick(mpcq, sess, q_w_prev, consts, wrench, ctx, params):
    """One ticked session against the host model fed the tick's own arrays."""
    r = PM.session_tick(sess.read(mpcq.SV_XREF)[:, :, 0], sess.read(mpcq.SV_FSTEPS), sess.read(mpcq.SV_GAIT),
                        sess.read(mpcq.SV_F0), q_w_prev, wrench, consts, **params)
    assert (sess.read(mpcq.SV_STATUS) == 1).all(), ctx
    assert _same(sess.plant_read(mpcq.PV_F_EFF), r["f_eff"]), ctx
    worst = 0.0
    for got, want in ((sess.plant_read(mpcq.PV_STATE_END), r["end"]), (sess.read(mpcq.SV_Q_W), r["q_w"]),
                      (sess.read(mpcq.SV_STATE), r["state"]), (sess.read(mpcq.SV_L_FEET), r["l_feet"])):
        d = float(np.abs(got - want).max())
        worst = max(worst, d)
        assert d <= TOL, (ctx, d)
    return worst


def test_session_rigid_plant_vs_model_and_reset(mpcq, eng):
    """PLANT_RIGID, 20 substeps, +40 % mass on the odd robots, wrenches on three robots: after
    every tick the session's arrays are the host model's; a reset mid-run keeps the wrench and
    the plant's table, and the ticks after it still are."""
    table, wrench = _plant_table(mpcq), _wrench()
    consts = PM.from_table(table)
    params = dict(integrator=PM.RIGID, n_sub=20, clamp=1)
    worst = 0.0
    with mpcq.Session(eng, SB, gait0=_gaits(SB)) as sess:
        sess.set_wrench(wrench)  # before the plant is enabled: it persists
        sess.enable_plant()
        sess.set_plant_robots(table)
        for k in range(6):
            q_w_prev = sess.read(mpcq.SV_Q_W)
            sess.tick(V_REF)
            worst = max(worst, _check_tick(mpcq, sess, q_w_prev, consts, wrench, k, params))
        # the heavier robots sag below the lighter ones: the mismatch is felt
        end = sess.plant_read(mpcq.PV_STATE_END)
        assert np.median(end[1::2, 2]) < np.median(end[0::2, 2])
        mask = np.zeros(SB, np.int32)
        mask[[1, 2]] = 1
        sess.reset(mask=mask)
        st = sess.read(mpcq.SV_STATE)
        stand = np.zeros(12)
        stand[2] = 0.2027682
        assert np.array_equal(st[1], stand) and np.array_equal(st[2], stand)
        assert not np.array_equal(st[3], stand)
        assert np.array_equal(sess.plant_read(mpcq.PV_WRENCH), wrench)
        for k in range(6, 9):
            q_w_prev = sess.read(mpcq.SV_Q_W)
            sess.tick(V_REF)
            worst = max(worst, _check_tick(mpcq, sess, q_w_prev, consts, wrench, k, params))
    print(f"max |session - model| = {worst:.2e}")


def test_session_push_is_felt_by_one_robot_only(mpcq, eng):
    names = SV + ("SV_SWING_REF",)
    pv = ("PV_STATE_END", "PV_F_EFF")
    w = np.zeros((SB, 6))
    w[1, 0] = 8.0

    def setup(push):
        def go(s):
            s.enable_swing()
            s.enable_plant()
            if push:
                s.set_wrench(w)
        return go
    A = _run(mpcq, eng, 4, setup=setup(False), names=names, plant_names=pv)
    P = _run(mpcq, eng, 4, setup=setup(True), names=names, plant_names=pv)
    others = np.arange(SB) != 1
    for k in range(4):
        for n in names + pv:
            if n != "SV_ORDER":  # (a permutation of all robots, not a per-robot row)
                assert _same(A[k][n][others], P[k][n][others]), (k, n)
    # robot 1 starts with yaw 0: world x is its local x on the first tick
    assert P[0]["PV_STATE_END"][1, 6] > A[0]["PV_STATE_END"][1, 6]
    assert P[3]["SV_Q_W"][1, 0] > A[3]["SV_Q_W"][1, 0]
    # and without the plant, tick 0's swing references are the same bits
    plain = _run(mpcq, eng, 1, setup=lambda s: s.enable_swing(), names=("SV_SWING_REF",))
    assert _same(plain[0]["SV_SWING_REF"], A[0]["SV_SWING_REF"])


def test_session_enable_then_disable_is_a_plain_session(mpcq, eng):
    def toggled(s):
        s.enable_plant()
        s.set_wrench([5.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        s.set_plant_robots(_plant_table(mpcq))
        s.disable_plant()
    A = _run(mpcq, eng, 3)
    D = _run(mpcq, eng, 3, setup=toggled)
    for k in range(3):
        for n in SV:
            if n != "SV_ORDER":
                assert _same(A[k][n], D[k][n]), (k, n)
        # SV_ORDER: the order kernel leaves the order inside a bucket of 16 iterations to its
        # LDS atomics, so two runs of one session agree in the buckets, not in the bits
        oa, od, it = A[k]["SV_ORDER"], D[k]["SV_ORDER"], A[k]["SV_ITERS"]
        assert np.array_equal(np.sort(oa), np.arange(SB)) and np.array_equal(np.sort(od), np.arange(SB))
        assert np.array_equal(it[oa] >> 4, it[od] >> 4), k
    # while an enabled plant under a mismatch does change the course
    E = _run(mpcq, eng, 3, setup=lambda s: (s.enable_plant(), s.set_plant_robots(_plant_table(mpcq))),
             names=("SV_STATE",))
    assert not _same(A[2]["SV_STATE"], E[2]["SV_STATE"])


def test_session_failed_robot_is_left_alone(mpcq, eng):
    bad = 33
    gaits = _gaits(SB)
    gaits[bad, :, 0] = 1.0  # no terminator: MPCQ_STATUS_BAD_GAIT
    good = _gaits(SB)
    pv = ("PV_STATE_END", "PV_F_EFF")

    def run(g):
        out = []
        with mpcq.Session(eng, SB, gait0=g) as sess:
            sess.enable_plant()
            sess.set_wrench([2.0, 1.0, 0.0, 0.0, 0.0, 0.1])
            for _ in range(2):
                before = (sess.read(mpcq.SV_Q_W), sess.read(mpcq.SV_STATE), sess.read(mpcq.SV_L_FEET))
                sess.tick(V_REF)
                snap = _snap(mpcq, sess, ("SV_STATUS", "SV_Q_W", "SV_STATE", "SV_L_FEET", "SV_F0"))
                snap.update({n: sess.plant_read(getattr(mpcq, n)) for n in pv})
                out.append((before, snap))
        return out
    R, G = run(gaits), run(good)
    others = np.arange(SB) != bad
    for (before, snap), (_, ref) in zip(R, G):
        assert snap["SV_STATUS"][bad] == mpcq.STATUS_BAD_GAIT and (snap["SV_STATUS"][others] == 1).all()
        for n, was in zip(("SV_Q_W", "SV_STATE", "SV_L_FEET"), before):
            assert _same(snap[n][bad], was[bad]), n  # not moved by the plant
        for n in pv:
            assert np.isnan(snap[n][bad]).all(), n
            assert np.isfinite(snap[n][others]).all(), n
        for n in ("SV_Q_W", "SV_STATE", "SV_L_FEET", "SV_F0") + pv:
            assert _same(snap[n][others], ref[n][others]), n  # its neighbours do not notice
