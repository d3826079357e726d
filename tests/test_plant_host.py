"""CPU: the rigid-body plant through the layers that need no device -- the header's
declarations, the ctypes binding, and the broadcasting of Session.enable_plant / set_wrench /
set_plant_robots (the native call stubbed, as tests/test_session_reset_host.py does)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")
NEW = ("mpcq_default_plant_params", "mpcq_plant_step_batch", "mpcq_session_enable_plant",
       "mpcq_session_disable_plant", "mpcq_session_set_plant_robots", "mpcq_session_set_wrench",
       "mpcq_session_plant_read", "mpcq_session_plant_device_ptr")


def test_header_declares_the_plant():
    src = open(HEADER).read()
    for name in NEW:
        assert re.search(rf"\b(int|void)\s+{name}\(", src), name
    for name, val in (("MPCQ_PLANT_MODEL", 0), ("MPCQ_PLANT_RIGID", 1), ("MPCQ_PV_STATE_END", 0),
                      ("MPCQ_PV_F_EFF", 1), ("MPCQ_PV_WRENCH", 2), ("MPCQ_ABI_VERSION", 3), ("MPCQ_SV_COUNT", 21)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", src), name
    assert re.search(r"sizeof\(mpcq_plant_params\) == 48", src)


def test_binding():
    import mpcq
    from mpcq import _lib as L
    assert C.sizeof(L.PlantParams) == 48
    for name in NEW:
        assert name in L.EXPORTS and hasattr(mpcq.lib(), name), name
    assert (mpcq.PLANT_MODEL, mpcq.PLANT_RIGID) == (0, 1)
    assert (mpcq.PV_STATE_END, mpcq.PV_F_EFF, mpcq.PV_WRENCH) == (0, 1, 2)
    p = mpcq.default_plant_params()
    assert (p.dt, p.gravity, p.n_sub, p.integrator, p.clamp) == (0.02, 9.81, 20, mpcq.PLANT_RIGID, 1)
    assert list(p.reserved) == [0] * 5
    q = mpcq.default_plant_params(n_sub=7, integrator=mpcq.PLANT_MODEL, clamp=0)
    assert (q.n_sub, q.integrator, q.clamp) == (7, 0, 0)
    with pytest.raises(AttributeError):
        mpcq.default_plant_params(substeps=3)
    for name in ("enable_plant", "disable_plant", "set_plant_robots", "set_wrench", "set_wrench_device",
                 "plant_read"):
        assert callable(getattr(mpcq.Session, name)), name
    assert callable(mpcq.Plant.step) and callable(mpcq.Plant.step_device)


class _Recorder:
    """Stands in for the Engine: copies what the pointers of a call hold while they are alive."""

    def __init__(self, B):
        import mpcq
        self.B = B
        self.params = mpcq.default_params()
        self.calls = []

    def _call(self, name, h, *args):
        import mpcq
        from mpcq import _lib as L
        B = self.B

        def grab(p, dtype, shape):
            if p is None:
                return None
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer(C.string_at(p.value, n), dtype).reshape(shape).copy()
        if name == "mpcq_session_enable_plant":
            pl = args[0]._obj  # (C.byref keeps the structure it points at)
            assert isinstance(pl, L.PlantParams)
            args = ((pl.dt, pl.gravity, pl.n_sub, pl.integrator, pl.clamp),)
        elif name == "mpcq_session_set_wrench":
            args = (grab(args[0], np.float64, (B, 6)), args[1])
        elif name == "mpcq_session_set_plant_robots":
            args = (grab(args[0], mpcq.ROBOT_DTYPE, (B,)), args[1])
        self.calls.append((name,) + tuple(args))


def _session(B):
    import mpcq
    s = mpcq.Session.__new__(mpcq.Session)  # no device: the native calls are the recorder's
    s.engine, s.batch, s._h, s.k = _Recorder(B), B, None, 4
    return s


def test_session_plant_calls_broadcast_their_arguments():
    import mpcq
    from mpcq import _lib as L
    B = 5
    s = _session(B)
    s.engine.params.dt = 0.02
    s.enable_plant()
    s.enable_plant(mpcq.default_plant_params(n_sub=7, integrator=mpcq.PLANT_MODEL, clamp=0))
    s.set_wrench([1.0, 0.0, -2.0, 0.0, 0.5, 0.0])
    w = np.zeros((B, 6))
    w[1, 0] = 3.0
    s.set_wrench(w)
    s.set_wrench(None)
    s.set_wrench_device(0)
    s.set_plant_robots(mpcq.robots(1, mass=3.5, mu=0.6))
    table = mpcq.robots(B, mass=np.linspace(2.0, 3.0, B))
    s.set_plant_robots(table)
    s.set_plant_robots(None)
    s.disable_plant()
    c = s.engine.calls
    assert c[0] == ("mpcq_session_enable_plant", (0.02, 9.81, 20, mpcq.PLANT_RIGID, 1))
    assert c[1] == ("mpcq_session_enable_plant", (0.02, 9.81, 7, mpcq.PLANT_MODEL, 0))
    assert c[2][0] == "mpcq_session_set_wrench" and c[2][2] == 0
    assert c[2][1].shape == (B, 6) and (c[2][1] == [1.0, 0.0, -2.0, 0.0, 0.5, 0.0]).all()
    assert np.array_equal(c[3][1], w)
    assert c[4][1] is None and c[4][2] == 0  # None: zero
    assert c[5][1] is None and c[5][2] == L.FLAG_DEVICE_PTRS | L.FLAG_ASYNC
    assert c[6][0] == "mpcq_session_set_plant_robots"
    assert c[6][1].shape == (B,) and (c[6][1]["mass"] == 3.5).all() and (c[6][1]["mu"] == 0.6).all()
    assert np.array_equal(c[7][1], table)
    assert c[8][1] is None
    assert c[9] == ("mpcq_session_disable_plant",)
    with pytest.raises(ValueError):
        s.set_plant_robots(mpcq.robots(B - 1))
    assert s.plant_params is None and s.k == 4
