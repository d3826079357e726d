"""CPU: the episode monitor through the layers that need no device -- the header's
declarations, the ctypes binding, the defaults, and the broadcasting of Session.enable_monitor /
run / monitor_read (the native call stubbed, as tests/test_plant_host.py does)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")
NEW = ("mpcq_default_monitor_params", "mpcq_monitor_step_batch", "mpcq_session_enable_monitor",
       "mpcq_session_disable_monitor", "mpcq_session_monitor_read", "mpcq_session_monitor_device_ptr",
       "mpcq_session_run")


def test_header_declares_the_monitor():
    src = open(HEADER).read()
    for name in NEW:
        assert re.search(rf"\b(int|void)\s+{name}\(", src), name
    for name, val in (("MPCQ_DONE_NONFINITE", 1), ("MPCQ_DONE_TILT", 2), ("MPCQ_DONE_HEIGHT", 4),
                      ("MPCQ_DONE_SOLVER", 8), ("MPCQ_DONE_TIMEOUT", 16), ("MPCQ_TRACE", 16), ("MPCQ_MV_DONE", 0),
                      ("MPCQ_MV_EP", 1), ("MPCQ_MV_EP_TICKS", 2), ("MPCQ_MV_EPISODES", 3), ("MPCQ_MV_LAST", 4),
                      ("MPCQ_MV_TOTALS", 5), ("MPCQ_MV_COUNT", 6), ("MPCQ_ABI_VERSION", 3), ("MPCQ_SV_COUNT", 21)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", src), name
    assert re.search(r"sizeof\(mpcq_monitor_params\) == 64", src)


def test_binding_and_defaults():
    import mpcq
    from mpcq import _lib as L
    assert C.sizeof(L.MonitorParams) == 64
    assert L.ABI_VERSION == 3 and mpcq.lib().mpcq_abi_version() == 3
    for name in NEW:
        assert name in L.EXPORTS and hasattr(mpcq.lib(), name), name
    assert (mpcq.DONE_NONFINITE, mpcq.DONE_TILT, mpcq.DONE_HEIGHT, mpcq.DONE_SOLVER, mpcq.DONE_TIMEOUT) == \
        (1, 2, 4, 8, 16)
    assert (mpcq.MV_DONE, mpcq.MV_EP, mpcq.MV_EP_TICKS, mpcq.MV_EPISODES, mpcq.MV_LAST, mpcq.MV_TOTALS) == \
        (0, 1, 2, 3, 4, 5)
    assert mpcq.TRACE == 16
    p = mpcq.default_monitor_params()
    assert isinstance(p, mpcq.MonitorParams)
    assert p.max_tilt > 0 and np.isfinite(p.min_height)  # (conventions: their values are not pinned)
    assert (p.max_ticks, p.auto_reset) == (0, 0)
    assert list(p.reserved) == [0] * 10
    q = mpcq.default_monitor_params(max_tilt=0.3, min_height=-np.inf, max_ticks=200, auto_reset=1)
    assert (q.max_tilt, q.min_height, q.max_ticks, q.auto_reset) == (0.3, -np.inf, 200, 1)
    with pytest.raises(AttributeError):
        mpcq.default_monitor_params(bad=1)
    for name in ("enable_monitor", "disable_monitor", "monitor_read", "monitor_device_ptr", "run", "run_device"):
        assert callable(getattr(mpcq.Session, name)), name
    assert callable(mpcq.Monitor.step) and callable(mpcq.Monitor.step_device)


def test_model_constants_are_the_bindings():
    import monitor_model as MM
    import mpcq
    from mpcq import monitor
    assert MM.BITS == (mpcq.DONE_NONFINITE, mpcq.DONE_TILT, mpcq.DONE_HEIGHT, mpcq.DONE_SOLVER, mpcq.DONE_TIMEOUT)
    assert MM.TRACE == mpcq.TRACE
    assert set(MM.OK_STATUS) == {mpcq.STATUS_SOLVED, mpcq.STATUS_SOLVED_INACCURATE, mpcq.STATUS_MAX_ITER_REACHED}
    a, b = MM.new_state(3), monitor.new_state(3)
    assert a.keys() == b.keys()
    for k in a:
        assert MM.same(a[k], b[k]), k


class _Recorder:
    """Stands in for the Engine: copies what the pointers of a call hold while they are alive,
    and fills the outputs of the reads."""

    def __init__(self, B):
        import mpcq
        self.B = B
        self.device = 0
        self.params = mpcq.default_params()
        self.calls = []

    def _call(self, name, h, *args):
        from mpcq import _lib as L
        B = self.B

        def grab(p, dtype, shape):
            if p is None:
                return None
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer(C.string_at(p.value, n), dtype).reshape(shape).copy()
        if name == "mpcq_session_enable_monitor":
            mp = args[0]._obj  # (C.byref keeps the structure it points at)
            assert isinstance(mp, L.MonitorParams)
            args = ((mp.max_tilt, mp.min_height, mp.max_ticks, mp.auto_reset),)
        elif name == "mpcq_session_run":
            k0, n_ticks, v_ref, v_ticks, trace, flags = args
            if trace is not None:  # the rows a monitor would write: tick and robot
                rows = np.zeros((n_ticks, B, 16))
                rows[:, :, 9] = np.arange(n_ticks)[:, None]
                rows[:, :, 0] = np.arange(B)[None, :]
                C.memmove(trace.value, rows.ctypes.data, rows.nbytes)
            args = (k0, n_ticks, grab(v_ref, np.float64, (v_ticks, B, 6)), v_ticks, trace is not None, flags)
        elif name == "mpcq_session_monitor_read":
            what, dst, flags = args
            n = {L.MV_EP: 8 * 8 * B, L.MV_LAST: 16 * 8 * B, L.MV_TOTALS: 64}.get(what, 4 * B)
            C.memset(dst.value, 0, n)
            C.memset(dst.value, what + 1, 1)
            args = (what, n, flags)
        self.calls.append((name,) + tuple(args))


def _session(B):
    import mpcq
    s = mpcq.Session.__new__(mpcq.Session)  # no device: the native calls are the recorder's
    s.engine, s.batch, s._h, s.k = _Recorder(B), B, None, 4
    # no device either: "device" arrays are host arrays
    s._to_device = lambda a: (a, a.ctypes.data)

    def new_device(shape):
        a = np.full(shape, -1.0)
        return a, a.ctypes.data, lambda: a
    s._new_device = new_device
    return s


def test_session_monitor_calls_broadcast_their_arguments():
    import mpcq
    from mpcq import _lib as L
    B = 5
    s = _session(B)
    s.enable_monitor()
    s.enable_monitor(max_tilt=0.4, max_ticks=9, auto_reset=1)
    s.enable_monitor(mpcq.default_monitor_params(min_height=0.05))
    with pytest.raises(ValueError):
        s.enable_monitor(mpcq.default_monitor_params(), max_ticks=3)
    with pytest.raises(AttributeError):
        s.enable_monitor(bad=1)
    d = mpcq.default_monitor_params()
    c = s.engine.calls
    assert c[0] == ("mpcq_session_enable_monitor", (d.max_tilt, d.min_height, 0, 0))
    assert c[1] == ("mpcq_session_enable_monitor", (0.4, d.min_height, 9, 1))
    assert c[2] == ("mpcq_session_enable_monitor", (d.max_tilt, 0.05, 0, 0))
    assert len(c) == 3 and s.monitor_params.min_height == 0.05
    # run: one command for every robot and tick
    assert s.run([0.3, 0.0, 0.0, 0.0, 0.0, 0.1], 7) is None
    name, k0, n, v, vt, has_trace, flags = c[3]
    assert (name, k0, n, vt, has_trace, flags) == ("mpcq_session_run", 4, 7, 1, False, L.FLAG_DEVICE_PTRS)
    assert v.shape == (1, B, 6) and (v == [0.3, 0.0, 0.0, 0.0, 0.0, 0.1]).all()
    assert s.k == 11
    # a command per robot, with a trace
    vb = np.arange(B * 6, dtype=np.float64).reshape(B, 6)
    tr = s.run(vb, 3, trace=True)
    name, k0, n, v, vt, has_trace, flags = c[4]
    assert (k0, n, vt, has_trace) == (11, 3, 1, True) and np.array_equal(v[0], vb)
    assert tr.shape == (3, B, 16)
    assert (tr[:, :, 9] == np.arange(3)[:, None]).all() and (tr[:, :, 0] == np.arange(B)[None, :]).all()
    # a schedule, one row broadcast over the robots, and an explicit k
    sched = np.zeros((2, 1, 6))
    sched[1, 0, 0] = 0.5
    s.run(sched, 4, k=0)
    name, k0, n, v, vt, has_trace, flags = c[5]
    assert (k0, n, vt) == (0, 4, 2) and v.shape == (2, B, 6) and (v[1, :, 0] == 0.5).all() and not v[0].any()
    assert s.k == 4
    with pytest.raises(ValueError):
        s.run(np.zeros((2, B + 1, 6)), 2)
    hold = np.zeros((3, B, 6))
    s.run_device(hold.ctypes.data, 6, v_ref_ticks=3, trace_ptr=0)
    assert c[6][0] == "mpcq_session_run" and c[6][1:3] == (4, 6) and c[6][4] == 3
    assert c[6][6] == L.FLAG_DEVICE_PTRS | L.FLAG_ASYNC and s.k == 10
    # monitor_read: shapes and types
    want = {L.MV_DONE: ((B,), np.int32), L.MV_EP: ((B, 8), np.float64), L.MV_EP_TICKS: ((B,), np.int32),
            L.MV_EPISODES: ((B,), np.int32), L.MV_LAST: ((B, 16), np.float64), L.MV_TOTALS: ((8,), np.uint64)}
    for what, (shape, dt) in want.items():
        a = s.monitor_read(what)
        assert a.shape == shape and a.dtype == dt, what
        assert s.engine.calls[-1] == ("mpcq_session_monitor_read", what, a.nbytes, 0)
        assert a.view(np.uint8).reshape(-1)[0] == what + 1 and not a.view(np.uint8).reshape(-1)[1:].any()
    with pytest.raises(mpcq.MpcqError):
        s.monitor_read(6)
    s.disable_monitor()
    assert s.engine.calls[-1] == ("mpcq_session_disable_monitor",) and s.monitor_params is None
