"""CPU: the estimator through the layers that need no device -- the header's declarations, the
ctypes binding, the defaults, every validation rule (the batch entry point checks its parameters
before anything else, so here the context is NULL and a call whose parameters pass fails on
that instead), NULL arguments of every entry point, and Session.enable_estimator with the native
call stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")
NEW = ("mpcq_default_estimator_params", "mpcq_estimator_step_batch", "mpcq_session_enable_estimator",
       "mpcq_session_disable_estimator", "mpcq_session_estimator_read", "mpcq_session_estimator_device_ptr")
CONSTS = (("MPCQ_EV_EST", 0), ("MPCQ_EV_ROW", 1), ("MPCQ_EV_COUNT", 2), ("MPCQ_ESTIMATOR_MAX_LAG", 8),
          ("MPCQ_ESTIMATOR_MAX_F_LAG", 4), ("MPCQ_EST_POST", 0), ("MPCQ_EST_PREV", 12), ("MPCQ_EST_P", 24),
          ("MPCQ_EST_CLOCK", 42), ("MPCQ_EST_RING", 44), ("MPCQ_EST_SLOTS", 12), ("MPCQ_EST_ROW", 332))
# what the issue pins as unchanged
KEPT = (("MPCQ_ABI_VERSION", 3), ("MPCQ_SV_COUNT", 21), ("MPCQ_HV_COUNT", 6), ("MPCQ_CV_COUNT", 7), ("MPCQ_MV_COUNT", 6),
        ("MPCQ_PV_COUNT", 3))


def test_header_declares_the_estimator():
    src = open(HEADER).read()
    for name in NEW:
        assert re.search(rf"\b(int|void)\s+{name}\(", src), name
    for name, val in CONSTS + KEPT:
        assert re.search(rf"#define\s+{name}\s+{val}\b", src), name
    assert len(re.findall(r"sizeof\(mpcq_estimator_params\) == 320", src)) == 2  # C and C++
    # the row: 12 + 12 + 18 + 2 + 12 slots of 24 doubles, a multiple of 16 bytes
    assert 44 + 12 * 24 == 332 and 332 * 8 % 16 == 0
    internal = open(os.path.join(REPO, "mpc-tsid_amd", "csrc", "mpcq_internal.h")).read()
    assert re.search(r"constexpr int kGatherMax = 48;", internal)  # the gather launch is untouched


def test_binding_and_defaults():
    import mpcq
    from mpcq import _lib as L
    assert C.sizeof(L.EstimatorParams) == 320
    assert (L.EstimatorParams.lag.offset, L.EstimatorParams.f_lag.offset, L.EstimatorParams.skip_repeats.offset) == (0, 4, 8)
    assert (L.EstimatorParams.reserved.offset, L.EstimatorParams.q.offset, L.EstimatorParams.r.offset,
            L.EstimatorParams.p0.offset) == (12, 32, 128, 224)
    for name in NEW:
        assert name in L.EXPORTS and hasattr(mpcq.lib(), name), name
    assert (mpcq.EV_EST, mpcq.EV_ROW) == (0, 1) and mpcq.EST_ROW == 332
    assert (mpcq.ESTIMATOR_MAX_LAG, mpcq.ESTIMATOR_MAX_F_LAG) == (8, 4)
    assert mpcq.lib().mpcq_abi_version() == 3
    junk = L.EstimatorParams()
    C.memset(C.byref(junk), 0xFF, 320)
    mpcq.lib().mpcq_default_estimator_params(C.byref(junk))
    p = mpcq.default_estimator_params()
    assert isinstance(p, mpcq.EstimatorParams) and bytes(p) == bytes(junk)
    assert (p.lag, p.f_lag, p.skip_repeats, list(p.reserved)) == (0, 0, 1, [0] * 5)
    assert list(p.q) == [1e-6] * 6 + [1e-4] * 6 and list(p.r) == [1e-4] * 12 and list(p.p0) == [1e-2] * 12
    import estimator_model as EM
    m = EM.params()
    for name, _ in L.EstimatorParams._fields_:
        v = getattr(p, name)
        assert (list(v) if hasattr(v, "__len__") else v) == getattr(m, name), name
    assert (EM.POST, EM.PREV, EM.P_OFF, EM.CLOCK, EM.RING, EM.SLOTS, EM.ROW) == (
        L.EST_POST, L.EST_PREV, L.EST_P, L.EST_CLOCK, L.EST_RING, L.EST_SLOTS, L.EST_ROW)
    q = mpcq.default_estimator_params(lag=3, f_lag=1, skip_repeats=0, r=0.5, q=[0.25] * 12)
    assert (q.lag, q.f_lag, q.skip_repeats) == (3, 1, 0) and list(q.r) == [0.5] * 12 and list(q.q) == [0.25] * 12
    with pytest.raises(AttributeError):
        mpcq.default_estimator_params(bad=1)
    with pytest.raises(ValueError):
        mpcq.default_estimator_params(p0=[0.0, 0.0])
    for name in ("enable_estimator", "disable_estimator", "estimator_read", "estimator_device_ptr"):
        assert callable(getattr(mpcq.Session, name)), name
    for name in ("step", "step_device"):
        assert callable(getattr(mpcq.Estimator, name)), name
    rows = mpcq.estimator.new_rows(3)
    parts = mpcq.estimator.unpack(rows)
    parts["valid"][1] = 1
    parts["ring"][2, 11, 23] = 7.0
    assert rows.view(np.int32)[1, 2 * L.EST_CLOCK] == 1 and rows[2, L.EST_ROW - 1] == 7.0
    assert parts["P"].shape == (3, 6, 3) and parts["post"].shape == (3, 12)


def _vec(i, v, fill):
    a = [fill] * 12
    a[i] = v
    return a


# (overrides, the field the message must name)
BAD = [(dict(lag=-1), "lag"), (dict(lag=9), "lag"), (dict(f_lag=-1), "f_lag"), (dict(f_lag=5), "f_lag"),
       (dict(r=_vec(0, 0.0, 1e-4)), "r["), (dict(r=_vec(11, -1.0, 1e-4)), "r["), (dict(r=_vec(5, np.nan, 1e-4)), "r["),
       (dict(r=_vec(7, np.inf, 1e-4)), "r["),
       (dict(q=_vec(3, -1e-9, 0.0)), "q["), (dict(q=_vec(0, np.nan, 0.0)), "q["), (dict(q=_vec(11, np.inf, 0.0)), "q["),
       (dict(p0=_vec(6, -1.0, 0.0)), "p0["), (dict(p0=_vec(0, np.nan, 0.0)), "p0["), (dict(p0=_vec(11, np.inf, 0.0)), "p0["),
       (dict(reserved=[0, 0, 0, 0, 1]), "reserved"), (dict(reserved=[-1, 0, 0, 0, 0]), "reserved")]
GOOD = [dict(), dict(lag=8, f_lag=4), dict(q=0.0, p0=0.0), dict(r=1e-300), dict(skip_repeats=0), dict(skip_repeats=-7),
        dict(q=1e300, p0=1e300, r=1e300)]


def _step(ep, ctx=None, drop=None):
    """mpcq_estimator_step_batch on sentinel arrays that must come back untouched."""
    from mpcq import _lib as L
    lib = L.lib()
    B = 2
    arrs = dict(obs=np.full((B, 12), 5.0), f_prev=np.full((B, 12), 2.0), feet_prev=np.full((B, 3, 4), 0.1),
                row=np.full((B, L.EST_ROW), -3.0), est=np.full((B, 12), -1.0))
    keep = {k: v.copy() for k, v in arrs.items()}
    p = lambda k: None if k == drop else C.c_void_p(arrs[k].ctypes.data)  # noqa: E731
    rc = lib.mpcq_estimator_step_batch(ctx, None if ep is None else C.byref(ep), B, None, 0, p("obs"), p("f_prev"),
                                       p("feet_prev"), None, None, p("row"), p("est"), 0)
    assert all(np.array_equal(arrs[k], keep[k]) for k in arrs)
    return rc, lib.mpcq_last_error().decode()


@pytest.mark.parametrize("bad,field", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b, _ in BAD])
def test_every_validation_rule(bad, field):
    import mpcq
    from mpcq import _lib as L
    rc, msg = _step(mpcq.default_estimator_params(**bad))
    assert rc == L.E_INVALID and "estimator" in msg and field in msg, (bad, msg)
    if field == "lag":  # f_lag's message must not pass for lag's
        assert "f_lag" not in msg, msg


def test_valid_parameters_pass_the_validation():
    import mpcq
    from mpcq import _lib as L
    for good in GOOD:
        rc, msg = _step(mpcq.default_estimator_params(**good))
        assert rc == L.E_INVALID and "ctx is NULL" in msg, (good, msg)  # the next check, not the parameters
    rc, msg = _step(None)  # NULL = the defaults
    assert rc == L.E_INVALID and "ctx is NULL" in msg


def test_null_arguments_without_a_device():
    """Every entry point refuses NULL with MPCQ_E_INVALID before it touches a device."""
    from mpcq import _lib as L
    lib = L.lib()
    lib.mpcq_default_estimator_params(None)  # a no-op
    out = C.c_void_p()
    buf = np.zeros(16)
    assert lib.mpcq_session_enable_estimator(None, None) == L.E_INVALID
    assert "NULL" in lib.mpcq_last_error().decode()
    assert lib.mpcq_session_disable_estimator(None) == L.E_INVALID
    assert lib.mpcq_session_estimator_read(None, 0, C.c_void_p(buf.ctypes.data), 0) == L.E_INVALID
    assert lib.mpcq_session_estimator_device_ptr(None, 0, C.byref(out)) == L.E_INVALID
    assert out.value is None
    rc, msg = _step(None)
    assert rc == L.E_INVALID and "NULL" in msg
    # a bad parameter wins over a NULL context and a NULL array: the parameters are checked first
    import mpcq
    rc, msg = _step(mpcq.default_estimator_params(lag=9), drop="obs")
    assert rc == L.E_INVALID and "lag" in msg


class _Engine:
    """Stands in for the native library: records the calls, refuses what the test tells it to."""

    def __init__(self):
        self.calls, self.refuse = [], False

    def _call(self, name, *args):
        from mpcq import _lib as L
        if self.refuse:
            raise L.MpcqError(L.E_INVALID, "the estimator needs lag in 0..8 (got 9)")
        self.calls.append((name, args))


def _session():
    import mpcq

    class Stubbed(mpcq.Session):
        def close(self):  # (the handle is not the library's)
            self._h = None

    s = object.__new__(Stubbed)
    s.engine, s._h, s.estimator_params, s.batch = _Engine(), C.c_void_p(1), None, 5
    return s


def test_session_enable_estimator_overrides_and_refusals():
    import mpcq
    from mpcq import _lib as L
    s = _session()
    s.enable_estimator(lag=3, f_lag=1, r=1e-6, skip_repeats=0)
    name, args = s.engine.calls[-1]
    assert name == "mpcq_session_enable_estimator" and args[0] is s._h
    sent = args[1]._obj
    assert isinstance(sent, L.EstimatorParams) and sent is s.estimator_params
    assert (sent.lag, sent.f_lag, sent.skip_repeats) == (3, 1, 0) and list(sent.r) == [1e-6] * 12
    assert list(sent.p0) == [1e-2] * 12
    s.enable_estimator()  # the defaults
    assert bytes(s.engine.calls[-1][1][1]._obj) == bytes(mpcq.default_estimator_params())
    mine = mpcq.default_estimator_params(lag=1)
    s.enable_estimator(mine)
    assert s.engine.calls[-1][1][1]._obj is mine and s.estimator_params is mine
    with pytest.raises(ValueError):
        s.enable_estimator(mine, lag=2)
    with pytest.raises(AttributeError):
        s.enable_estimator(lagg=2)
    # a refusal of the library reaches the caller, and the parameters in force stay
    s.engine.refuse = True
    with pytest.raises(L.MpcqError) as e:
        s.enable_estimator(lag=9)
    assert "lag" in str(e.value) and s.estimator_params is mine
    s.engine.refuse = False
    s.disable_estimator()
    assert s.engine.calls[-1][0] == "mpcq_session_disable_estimator" and s.estimator_params is None
    with pytest.raises(L.MpcqError):
        s._group_shape("estimator", 2)
    assert s._group_shape("estimator", L.EV_ROW) == ((5, 332), np.float64) and s._group_shape("estimator", L.EV_EST) == ((5, 12), np.float64)
