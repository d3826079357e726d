"""CPU: session snapshots through the layers that need no device -- the header's declarations,
the ctypes binding, Session.restore / fork's broadcasting of the map and their bookkeeping of
Session.k (the native call stubbed), and the NULL-argument answers of every entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")

NAMES = ("mpcq_session_snapshot_create", "mpcq_session_snapshot_destroy", "mpcq_session_snapshot_save",
         "mpcq_session_snapshot_restore", "mpcq_session_fork", "mpcq_session_snapshot_bytes",
         "mpcq_session_snapshot_export", "mpcq_session_snapshot_import", "mpcq_debug_gather_rows")

SIGNATURES = (
    r"typedef struct mpcq_snapshot mpcq_snapshot;",
    r"int mpcq_session_snapshot_create\(mpcq_session\* s, mpcq_snapshot\*\* out\);",
    r"int mpcq_session_snapshot_destroy\(mpcq_snapshot\* snap\);",
    r"int mpcq_session_snapshot_save\(mpcq_session\* s, mpcq_snapshot\* snap, uint32_t flags\);",
    r"int mpcq_session_snapshot_restore\(mpcq_session\* s, const mpcq_snapshot\* snap, const int32_t\* map, "
    r"uint32_t flags\);",
    r"int mpcq_session_fork\(mpcq_session\* s, const int32_t\* map, uint32_t flags\);",
    r"int mpcq_session_snapshot_bytes\(const mpcq_snapshot\* snap, int64_t\* bytes\);",
    r"int mpcq_session_snapshot_export\(const mpcq_snapshot\* snap, void\* dst, int64_t bytes\);",
    r"int mpcq_session_snapshot_import\(mpcq_session\* s, mpcq_snapshot\* snap, const void\* src, int64_t bytes\);",
    r"int mpcq_debug_gather_rows\(mpcq_ctx\* ctx, int n, const void\* const\* src, void\* const\* dst, "
    r"const int64_t\* row_bytes, int64_t rows_src, int64_t rows_dst, const int32_t\* map, uint32_t flags\);",
)


def test_header_declares_the_snapshot_interface():
    src = re.sub(r"\s+", " ", open(HEADER).read())
    for sig in SIGNATURES:  # the typedef and the nine functions
        assert re.search(sig, src), sig
    assert re.search(r"#define MPCQ_SV_COUNT 21\b", src)
    assert re.search(r"#define MPCQ_ABI_VERSION 3\b", src)


def test_binding_exports_them():
    import mpcq
    from mpcq import _lib as L
    for n in NAMES:
        assert n in L.EXPORTS, n
    assert L.ABI_VERSION == 3
    for m in ("snapshot", "snapshot_from", "restore", "restore_device", "fork", "fork_device"):
        assert callable(getattr(mpcq.Session, m)), m
    for m in ("save", "tobytes", "close", "__enter__", "__exit__"):
        assert callable(getattr(mpcq.Snapshot, m)), m


class _Recorder:
    """Stands in for the Engine: copies what the map pointer of a call holds while it is alive."""

    def __init__(self, B):
        self.B = B
        self.calls = []

    def _call(self, name, *args):
        if name == "mpcq_session_fork":
            (h, mp, flags), snap = args, None
        else:
            h, snap, mp, flags = args
        m = None
        if mp is not None and not (flags & 1):
            m = np.ctypeslib.as_array((C.c_int32 * self.B).from_address(mp.value)).copy()
        self.calls.append((name, snap, m if m is not None else (mp.value if mp is not None else None), flags))


def _session(B, k):
    import mpcq
    s = mpcq.Session.__new__(mpcq.Session)  # no device: the native calls are the recorder's
    s.engine, s.batch, s._h, s.k = _Recorder(B), B, None, k
    return s


def _snap(k):
    import mpcq
    p = mpcq.Snapshot.__new__(mpcq.Snapshot)
    p._h, p.k = None, k
    return p


def test_restore_and_fork_broadcast_and_convert_the_map():
    from mpcq import _lib as L
    B = 5
    s, p = _session(B, 9), _snap(6)
    s.restore(p, 2)                              # a scalar: every slot from row 2
    s.restore(p, [0, -1, 3.0, -1, 1])            # converted to int32
    s.restore(p, np.arange(B, dtype=np.int64)[::-1])  # another dtype, not contiguous
    s.fork(3)
    s.fork([4, 4, -1, 0, 0])
    s.restore_device(p, 0x1000)
    s.fork_device(0x2000, asynchronous=False)
    c = s.engine.calls
    assert [x[0] for x in c] == ["mpcq_session_snapshot_restore"] * 3 + ["mpcq_session_fork"] * 2 + \
        ["mpcq_session_snapshot_restore", "mpcq_session_fork"]
    assert c[0][2].dtype == np.int32 and c[0][2].tolist() == [2] * B and c[0][3] == 0
    assert c[1][2].tolist() == [0, -1, 3, -1, 1]
    assert c[2][2].tolist() == [4, 3, 2, 1, 0]
    assert c[3][2].tolist() == [3] * B and c[4][2].tolist() == [4, 4, -1, 0, 0] and c[4][3] == 0
    assert c[5][2] == 0x1000 and c[5][3] == L.FLAG_DEVICE_PTRS | L.FLAG_ASYNC
    assert c[6][2] == 0x2000 and c[6][3] == L.FLAG_DEVICE_PTRS
    assert s.k == 9  # mapped restores and forks of a session that has ticked leave its counter alone
    with pytest.raises(ValueError):
        s.restore(p, [0, 1])  # not broadcastable to (B,)


def test_restore_keeps_session_k_right():
    s, p = _session(4, 9), _snap(6)
    s.restore(p)  # the identity: NULL map, back to the snapshot's tick index
    assert s.engine.calls[-1][2] is None and s.k == 6
    s.k = 11
    s.restore_device(p, 0)
    assert s.engine.calls[-1][2] is None and s.k == 6
    fresh = _session(4, 0)  # has not ticked: a mapped restore hands it the snapshot's robots
    fresh.restore(p, [0, 1, 0, 1])
    assert fresh.k == 6
    fresh = _session(4, 0)
    fresh.fork(0)
    assert fresh.k == 0


def test_null_arguments_are_invalid_without_a_device():
    import mpcq
    mpcq.build()
    lib = mpcq.lib()
    vp = C.c_void_p
    some = C.create_string_buffer(256)  # stands for a non-NULL handle that must not be reached
    out, n = vp(), C.c_int64()
    inval = mpcq._lib.E_INVALID
    assert lib.mpcq_session_snapshot_destroy(None) == mpcq._lib.OK
    assert lib.mpcq_session_snapshot_create(None, C.byref(out)) == inval and not out.value
    assert lib.mpcq_session_snapshot_create(None, None) == inval
    assert lib.mpcq_session_snapshot_save(None, None, 0) == inval
    assert lib.mpcq_session_snapshot_restore(None, None, None, 0) == inval
    assert lib.mpcq_session_fork(None, None, 0) == inval
    assert lib.mpcq_session_snapshot_bytes(None, C.byref(n)) == inval
    assert lib.mpcq_session_snapshot_export(None, some, 256) == inval
    assert lib.mpcq_session_snapshot_import(None, None, some, 256) == inval
    assert lib.mpcq_debug_gather_rows(None, 1, some, some, some, 1, 1, None, 0) == inval
    # a non-NULL first argument with a NULL one behind it: refused before the first is looked at
    assert lib.mpcq_session_snapshot_create(some, None) == inval
    assert lib.mpcq_session_snapshot_save(some, None, 0) == inval
    assert lib.mpcq_session_snapshot_restore(some, None, None, 0) == inval
    assert lib.mpcq_session_fork(some, None, 0) == inval
    assert lib.mpcq_session_snapshot_bytes(some, None) == inval
    assert lib.mpcq_session_snapshot_export(some, None, 256) == inval
    assert lib.mpcq_session_snapshot_import(some, None, some, 256) == inval
    assert lib.mpcq_session_snapshot_import(some, some, None, 256) == inval
    for n, src, dst, rb in ((0, some, some, some), (49, some, some, some), (1, None, some, some),
                            (1, some, None, some), (1, some, some, None)):
        assert lib.mpcq_debug_gather_rows(some, n, src, dst, rb, 1, 1, None, 0) == inval, n
    assert len(lib.mpcq_last_error()) > 0


def test_engine_close_frees_its_live_snapshots_first():
    """A Snapshot's native destroy needs its context: Engine.close closes the live ones before
    it destroys the context, and one closed after its engine makes no native call."""
    import mpcq
    calls = []

    class _Eng(mpcq.Engine):
        def __init__(self):  # no device
            import threading
            import weakref
            self._h, self.lock, self._snapshots = object(), threading.RLock(), weakref.WeakSet()

    e = _Eng()
    p = mpcq.Snapshot.__new__(mpcq.Snapshot)
    p.engine, p._h = e, None
    p.close = lambda: calls.append("snapshot")
    e._snapshots.add(p)
    lib = mpcq.lib()
    real = lib.mpcq_destroy
    try:
        lib.mpcq_destroy = lambda h: calls.append("context")
        e.close()
    finally:
        lib.mpcq_destroy = real
    assert calls == ["snapshot", "context"] and e._h is None
    late = mpcq.Snapshot.__new__(mpcq.Snapshot)
    late.engine, late._h = e, C.c_void_p(1)  # its engine is gone: forgotten, not destroyed
    late.close()
    assert late._h is None
