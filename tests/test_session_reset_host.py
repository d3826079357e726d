"""CPU: the per-robot session reset through the layers that need no device -- the header's
declaration, the ctypes binding, and Session.reset's broadcasting (the native call stubbed)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")


def test_header_declares_reset_and_sv_first():
    src = open(HEADER).read()
    assert re.search(r"int\s+mpcq_session_reset\(mpcq_session\*\s*s,\s*const int32_t\*\s*mask,\s*const double\*\s*gait0,"
                     r"\s*const double\*\s*q_w0,\s*uint32_t flags\);", src)
    assert re.search(r"#define\s+MPCQ_SV_FIRST\s+20\b", src)
    assert re.search(r"#define\s+MPCQ_SV_COUNT\s+21\b", src)
    assert re.search(r"#define\s+MPCQ_ABI_VERSION\s+3\b", src)


def test_binding_exposes_both():
    import mpcq
    from mpcq import _lib as L
    assert L.SV_FIRST == 20 and mpcq.SV_FIRST == 20
    assert "mpcq_session_reset" in L.EXPORTS
    assert callable(mpcq.Session.reset) and callable(mpcq.Session.reset_device)
    assert mpcq.session._shapes(5, 16)[L.SV_FIRST] == ((5,), np.int32)


class _Recorder:
    """Stands in for the Engine: copies what the pointers of a call hold while they are alive."""

    def __init__(self, B):
        self.B = B
        self.calls = []

    def _call(self, name, h, mask, gait0, q_w0, flags):
        def grab(p, ctype, shape):
            if p is None:
                return None
            n = int(np.prod(shape))
            return np.ctypeslib.as_array((ctype * n).from_address(p.value)).reshape(shape).copy()
        B = self.B
        self.calls.append((name, grab(mask, C.c_int32, (B,)), grab(gait0, C.c_double, (B, 20, 5)),
                           grab(q_w0, C.c_double, (B, 6)), flags))


def _session(B):
    import mpcq
    s = mpcq.Session.__new__(mpcq.Session)  # no device: the native calls are the recorder's
    s.engine, s.batch, s._h, s.k = _Recorder(B), B, None, 4
    return s


def test_reset_broadcasts_its_arguments():
    from mpcq import synth
    B = 5
    s = _session(B)
    table = synth.gait_table("bound", 16)
    s.reset(mask=1, gait0=table, q_w0=[1.0, 2.0, 0.2, 0.0, 0.0, 0.5])
    s.reset(mask=[0, 3, 0, -1, 0])
    s.reset()
    s.reset_device(mask_ptr=0, gait0_ptr=0, q_w0_ptr=0)
    (n0, m0, g0, q0, f0), (_, m1, g1, q1, _), (_, m2, g2, q2, _), (n3, m3, g3, q3, f3) = s.engine.calls
    assert n0 == n3 == "mpcq_session_reset"
    assert m0.dtype == np.int32 and m0.tolist() == [1] * B  # a scalar mask: every robot
    assert g0.shape == (B, 20, 5) and all(np.array_equal(g0[b], table) for b in range(B))
    assert q0.shape == (B, 6) and (q0 == [1.0, 2.0, 0.2, 0.0, 0.0, 0.5]).all()
    assert f0 == 0
    assert m1.tolist() == [0, 1, 0, 1, 0] and g1 is None and q1 is None  # nonzero = reset
    assert m2 is None and g2 is None and q2 is None  # NULL mask: every robot
    assert m3 is None and g3 is None and q3 is None
    from mpcq import _lib as L
    assert f3 == L.FLAG_DEVICE_PTRS | L.FLAG_ASYNC
    assert s.k == 4  # a reset does not move the session's tick counter
