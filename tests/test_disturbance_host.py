"""CPU: the mpcq_disturbance / mpcq_disturb_params ABI, their Python mirrors, and the power of
tests/disturbance_cases.py.

test_gpu_disturbance.py compares the engine under a per-instance disturbance table with
per-instance references built at the QP level (oracle.formulate, the shifted bounds,
oracle.qp_solve).  That comparison only means something if the table moves every instance: the
power test below re-establishes, from the oracle alone and at every horizon of the table, that

* with a = 0 the reference path (formulate -> qp_solve) is oracle.solve_batch bit for bit;
* with the rows every instance ends SOLVED, except at N = 50 where the status set is {1, 2},
  exactly the unshifted batch's; iteration counts stay within 350..4000;
* every instance's f0 moves by at least 0.59 from its unshifted result, by at least 7.1 from its
  neighbour instance's result, and by at least 0.5 from its own result under its neighbour's row
  (table[(b + 1) % B]): a kernel that ignored the table, or read another row, would miss by
  seven decades more than the GPU tolerance.

These are conditions on the inputs, not tolerances: a recipe that fails them is replaced, not
relaxed.

The validation of a host table runs behind a context, which needs a device: what is reachable
here is the validation of the stage's parameters (checked before the context is looked at), the
refusal of NULL handles, and the checks the Python layer makes before the call
(test_gpu_disturbance.py::test_validation has the table's rules that name index and field).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import disturbance_cases as DC
import param_cases as PC
from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")
NEW = ("mpcq_set_disturbance", "mpcq_session_set_disturbance", "mpcq_session_get_disturbance",
       "mpcq_default_disturb_params", "mpcq_disturb_step_batch", "mpcq_session_enable_disturb",
       "mpcq_session_disable_disturb", "mpcq_session_disturb_read", "mpcq_session_disturb_device_ptr")


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as m
    m.build()
    return m


def test_struct_layouts(mpcq):
    L = mpcq._lib
    assert C.sizeof(L.Disturbance) == 64
    assert [(n, getattr(L.Disturbance, n).offset) for n, _ in L.Disturbance._fields_] == [("a", 0), ("reserved", 48)]
    dt = mpcq.DISTURBANCE_DTYPE
    assert dt.itemsize == 64
    assert [(n, dt.fields[n][1], dt.fields[n][0].shape) for n in dt.names] == [("a", 0, (6,)), ("reserved", 48, (2,))]
    assert C.sizeof(L.DisturbParams) == 128
    assert [(n, getattr(L.DisturbParams, n).offset) for n, _ in L.DisturbParams._fields_] == [
        ("alpha", 0), ("d_max", 48), ("f_lag", 96), ("compensate", 100), ("skip_repeats", 104), ("reserved", 108)]
    src = open(HEADER).read()
    for name, size in (("mpcq_disturbance", 64), ("mpcq_disturb_params", 128)):
        assert src.count(f"_Static_assert(sizeof({name}) == {size}") == 1
        assert src.count(f"static_assert(sizeof({name}) == {size}") == 1  # (the C++ spelling)


def test_header_and_binding(mpcq):
    src = open(HEADER).read()
    for name in NEW:
        assert re.search(rf"\b(int|void)\s+{name}\(", src), name
        assert name in mpcq._lib.EXPORTS and hasattr(mpcq.lib(), name), name
    # additive: the version and every existing count stay
    for name, val in (("MPCQ_ABI_VERSION", 3), ("MPCQ_SV_COUNT", 21), ("MPCQ_PV_COUNT", 3), ("MPCQ_MV_COUNT", 6),
                      ("MPCQ_CV_COUNT", 7), ("MPCQ_HV_COUNT", 6), ("MPCQ_EV_COUNT", 2), ("MPCQ_GV_COUNT", 1),
                      ("MPCQ_DV_COUNT", 3), ("MPCQ_DV_DIST", 0), ("MPCQ_DV_ROW", 1), ("MPCQ_DV_RESID", 2),
                      ("MPCQ_DIST_D", 0), ("MPCQ_DIST_PREV", 6), ("MPCQ_DIST_CLOCK", 18), ("MPCQ_DIST_RING", 20),
                      ("MPCQ_DIST_SLOTS", 5), ("MPCQ_DIST_ROW", 80), ("MPCQ_DISTURB_MAX_F_LAG", 4),
                      ("MPCQ_EST_ROW", 332)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", src), name
    assert mpcq.lib().mpcq_abi_version() == 3
    L = mpcq._lib
    assert (L.DV_DIST, L.DV_ROW, L.DV_RESID) == (0, 1, 2)
    assert (L.DIST_D, L.DIST_PREV, L.DIST_CLOCK, L.DIST_RING, L.DIST_SLOTS, L.DIST_ROW) == (0, 6, 18, 20, 5, 80)
    assert L.DIST_RING + L.DIST_SLOTS * 12 == L.DIST_ROW and L.DIST_ROW * 8 % 16 == 0
    assert L.DIST_SLOTS == L.DISTURB_MAX_F_LAG + 1
    assert C.sizeof(L.Robot) == 128 and C.sizeof(L.Weights) == 128
    for cls, name in ((mpcq.Engine, "set_disturbance"), (mpcq.Engine, "set_disturbance_device"),
                      (mpcq.Session, "set_disturbance"), (mpcq.Session, "get_disturbance"),
                      (mpcq.Session, "enable_disturb"), (mpcq.Session, "disable_disturb"),
                      (mpcq.Session, "disturb_read"), (mpcq.Session, "disturb_device_ptr"),
                      (mpcq.Disturb, "step"), (mpcq.Disturb, "step_device")):
        assert callable(getattr(cls, name)), name
    import disturb_model as DM
    assert (DM.D, DM.PREV, DM.CLOCK, DM.RING, DM.SLOTS, DM.ROW) == (L.DIST_D, L.DIST_PREV, L.DIST_CLOCK, L.DIST_RING,
                                                                   L.DIST_SLOTS, L.DIST_ROW)


def test_default_disturb_params(mpcq):
    import disturb_model as DM
    p, m = mpcq.default_disturb_params(), DM.params()
    assert list(p.alpha) == m.alpha == [0.2] * 6 and list(p.d_max) == m.d_max == [5.0] * 3 + [30.0] * 3
    assert (p.f_lag, p.compensate, p.skip_repeats) == (m.f_lag, m.compensate, m.skip_repeats) == (0, 1, 1)
    assert list(p.reserved) == [0] * 5
    mpcq.lib().mpcq_default_disturb_params(None)  # a NULL output is ignored, never a crash
    q = mpcq.default_disturb_params(alpha=0.5, d_max=[1, 2, 3, 4, 5, 6], f_lag=3, compensate=0)
    assert list(q.alpha) == [0.5] * 6 and list(q.d_max) == [1, 2, 3, 4, 5, 6] and (q.f_lag, q.compensate) == (3, 0)
    with pytest.raises(AttributeError):
        mpcq.default_disturb_params(lag=1)
    with pytest.raises(ValueError):
        mpcq.default_disturb_params(alpha=[0.1, 0.2])


BAD_PARAMS = [(dict(alpha=[0.2, 0.2, -0.1, 0.2, 0.2, 0.2]), "alpha[2]"), (dict(alpha=[1.5] + [0.2] * 5), "alpha[0]"),
              (dict(alpha=[0.2] * 5 + [float("nan")]), "alpha[5]"), (dict(d_max=[5, 5, 5, 30, 0.0, 30]), "d_max[4]"),
              (dict(d_max=[-1.0] + [5] * 5), "d_max[0]"), (dict(d_max=[5, float("inf"), 5, 5, 5, 5]), "d_max[1]"),
              (dict(d_max=[5, 5, float("nan"), 5, 5, 5]), "d_max[2]"), (dict(f_lag=-1), "f_lag"), (dict(f_lag=5), "f_lag"),
              (dict(reserved=[0, 0, 1, 0, 0]), "reserved")]


@pytest.mark.parametrize("over,word", BAD_PARAMS)
def test_parameter_rules_name_the_field(mpcq, over, word):
    """Checked before anything else: a NULL context behind bad parameters still reports the field."""
    lib, E = mpcq.lib(), mpcq._lib.E_INVALID
    p = mpcq.default_disturb_params(**over)
    z = np.zeros(96)
    v = C.c_void_p(z.ctypes.data)
    assert lib.mpcq_disturb_step_batch(None, C.byref(p), 1, None, 1, v, v, v, None, None, v, v, None, 0) == E
    assert word.encode() in lib.mpcq_last_error(), lib.mpcq_last_error()
    assert lib.mpcq_session_enable_disturb(None, C.byref(p)) == E and b"session is NULL" in lib.mpcq_last_error()


def test_null_handles_are_codes_not_crashes(mpcq):
    lib, E = mpcq.lib(), mpcq._lib.E_INVALID
    t = mpcq.disturbances(3)
    p = C.c_void_p(t.ctypes.data)
    assert lib.mpcq_set_disturbance(None, 3, p, 0) == E and b"ctx is NULL" in lib.mpcq_last_error()
    assert lib.mpcq_session_set_disturbance(None, p, 0) == E and b"session is NULL" in lib.mpcq_last_error()
    assert lib.mpcq_session_get_disturbance(None, p, 0) == E and b"session is NULL" in lib.mpcq_last_error()
    assert lib.mpcq_session_disable_disturb(None) == E and b"session is NULL" in lib.mpcq_last_error()
    assert lib.mpcq_session_disturb_read(None, 0, p, 0) == E
    out = C.c_void_p()
    assert lib.mpcq_session_disturb_device_ptr(None, 0, C.byref(out)) == E
    good = mpcq.default_disturb_params()
    assert lib.mpcq_disturb_step_batch(None, C.byref(good), 1, None, 1, p, p, p, None, None, p, p, None, 0) == E


def test_disturbances_broadcasting(mpcq):
    t = mpcq.disturbances(5)
    assert t.shape == (5,) and t.dtype == mpcq.DISTURBANCE_DTYPE and t.flags.c_contiguous and not t.tobytes().strip(b"\0")
    t = mpcq.disturbances(5, lin=[1.0, 2.0, 3.0])
    assert (t["a"][:, :3] == [1.0, 2.0, 3.0]).all() and not t["a"][:, 3:].any() and not t["reserved"].any()
    lin, ang = np.arange(15.0).reshape(5, 3), -np.arange(15.0).reshape(5, 3)
    t = mpcq.disturbances(5, lin=lin, ang=ang)
    assert np.array_equal(t["a"][:, :3], lin) and np.array_equal(t["a"][:, 3:], ang)
    t2 = mpcq.disturbances(5, ang=0.5)
    assert (t2["a"][:, 3:] == 0.5).all() and not t2["a"][:, :3].any()
    d = mpcq.Disturbance.from_buffer_copy(t[2].tobytes())  # the bytes of a row are a mpcq_disturbance
    assert list(d.a) == lin[2].tolist() + ang[2].tolist() and list(d.reserved) == [0.0, 0.0]
    with pytest.raises(ValueError):
        mpcq.disturbances(5, lin=np.ones((4, 3)))
    with pytest.raises(ValueError):
        mpcq.disturbances(5, ang=np.ones(2))


def test_recipe_is_the_documented_one(mpcq):
    """The first instance of N = 16 drawn by hand in the documented order."""
    rng = np.random.default_rng(1116)
    a = np.concatenate([rng.uniform(-2, 2, 2), [rng.uniform(-3, 3)], rng.uniform(-5, 5, 3)])
    t = DC.make_disturbances(16)
    assert t.shape == (16,) and t.dtype == mpcq.DISTURBANCE_DTYPE
    assert np.array_equal(t["a"][0], a) and not t["reserved"].any()
    for N in DC.HORIZONS:
        assert DC.make_disturbances(N).shape == (16 if N <= 20 else 8,)


@pytest.mark.parametrize("N", DC.HORIZONS)
def test_recipe_has_power(oracle, N):
    tab = DC.make_disturbances(N)
    B = tab.shape[0]
    s = PC.make_batch(N)
    r = DC.oracle_solve(oracle, N, tab, key="table")
    plain = DC.oracle_solve(oracle, N, None, key="unshifted")
    nb = DC.oracle_solve(oracle, N, np.roll(tab, -1))  # instance b under table[(b + 1) % B]
    sb = oracle.solve_batch(s["xref"], s["fsteps"], 0, nthreads=8, want_x=True)
    for k in ("x", "f0", "status", "iters", "rho_updates", "admm_status"):
        assert np.array_equal(plain[k], sb[k]), k  # a = 0: qp_solve(formulate) is solve_batch bit for bit
    want = {1, 2} if N == 50 else {1}
    assert set(r["status"].tolist()) == want == set(plain["status"].tolist()), r["status"]
    assert 350 <= r["iters"].min() and r["iters"].max() <= 4000, r["iters"]
    mv_p = np.abs(r["f0"] - plain["f0"]).max(axis=1)
    mv_i = np.abs(r["f0"] - np.roll(r["f0"], -1, axis=0)).max(axis=1)
    mv_n = np.abs(r["f0"] - nb["f0"]).max(axis=1)
    print(f"N={N}: B {B}, iters {r['iters'].min()}..{r['iters'].max()}, movement vs unshifted >= {mv_p.min():.3f}, "
          f"vs the neighbour instance >= {mv_i.min():.3f}, vs the neighbour's row >= {mv_n.min():.3f}")
    assert (mv_p >= 0.59).all(), mv_p
    assert (mv_i >= 7.1).all(), mv_i
    assert (mv_n >= 0.5).all(), mv_n
    # the shift is what the header says: only the dynamics rows 6..11 of every stage move, l == u there
    rows = (np.arange(12 * N) % 12) >= 6
    for k in ("l", "u"):
        assert np.array_equal(r[k][:, 12 * N:], plain[k][:, 12 * N:])  # (-inf among them)
        assert np.array_equal(r[k][:, :12 * N][:, ~rows], plain[k][:, :12 * N][:, ~rows])
        assert (np.abs(r[k][:, :12 * N][:, rows] - plain[k][:, :12 * N][:, rows]).reshape(B, N, 6).min(axis=1) > 0).all()
    assert np.array_equal(r["l"][:, :12 * N], r["u"][:, :12 * N])
    assert np.array_equal(r["Ax"], plain["Ax"])


class _Recorder:
    """Stands in for the Engine: copies what the pointers of a call hold while they are alive."""

    def __init__(self):
        self.calls = []

    def _call(self, name, h, *args):
        self.calls.append((name,) + args)


def test_python_table_checks(mpcq):
    """What the Python layer refuses before the call: another dtype, another rank, a session table
    of another length.  A ctypes array of L.Disturbance is accepted as it is."""
    from mpcq.engine import _disturbance_table
    t = mpcq.disturbances(4, lin=1.0)
    assert _disturbance_table(t, 4) is not None
    arr = (mpcq.Disturbance * 2)()
    assert _disturbance_table(arr).tobytes() == mpcq.disturbances(2).tobytes()
    for bad in (mpcq.weights(4), np.zeros((4, 8)), t.reshape(2, 2)):
        with pytest.raises(ValueError):
            _disturbance_table(bad)
    with pytest.raises(ValueError):
        _disturbance_table(t, 5)
    s = mpcq.Session.__new__(mpcq.Session)
    s.engine, s.batch, s._h = _Recorder(), 4, None
    with pytest.raises(ValueError):
        s.set_disturbance(mpcq.disturbances(3))
    assert s.engine.calls == []
    s.set_disturbance(None)
    assert s.engine.calls == [("mpcq_session_set_disturbance", None, 0)]
    with pytest.raises(ValueError):
        s.enable_disturb(mpcq.default_disturb_params(), alpha=0.1)  # params or overrides, not both
    # the stand-alone kernel's wrapper checks shapes before the call
    k = mpcq.Disturb(s.engine)
    with pytest.raises(ValueError):
        k.step(np.zeros((3, 11)), np.zeros(12), np.zeros((3, 4)))
    with pytest.raises(ValueError):
        k.step(np.zeros((3, 12)), np.zeros(12), np.zeros((3, 4)), rows=np.zeros((3, 79)))
    with pytest.raises(ValueError):
        mpcq.disturb.unpack(np.zeros((3, 79)))
    u = mpcq.disturb.unpack(mpcq.disturb.new_rows(3))
    assert u["d"].shape == (3, 6) and u["prev"].shape == (3, 12) and u["ring"].shape == (3, 5, 12)
    assert u["valid"].shape == u["tau_next"].shape == (3,)
