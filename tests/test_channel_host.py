"""CPU: the channel through the layers that need no device -- the header's declarations, the
ctypes binding, the defaults, every validation rule (the batch entry points check their
parameters before anything else, so here the context is NULL and a call whose parameters pass
fails on that instead), NULL arguments of every entry point, and Session.enable_channel with the
native call stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")
NEW = ("mpcq_default_channel_params", "mpcq_channel_observe_batch", "mpcq_channel_actuate_batch",
       "mpcq_session_enable_channel", "mpcq_session_disable_channel", "mpcq_session_channel_read",
       "mpcq_session_channel_device_ptr")
IDS = ("CLOCK", "OBS", "F_CMD", "DRAW", "S_RING", "F_RING")


def test_header_declares_the_channel():
    src = open(HEADER).read()
    for name in NEW:
        assert re.search(rf"\b(int|void)\s+{name}\(", src), name
    for val, name in enumerate(IDS):
        assert re.search(rf"#define\s+MPCQ_HV_{name}\s+{val}\b", src), name
    for name, val in (("MPCQ_HV_COUNT", 6), ("MPCQ_ABI_VERSION", 3), ("MPCQ_SV_COUNT", 21), ("MPCQ_CV_COUNT", 7)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", src), name
    assert re.search(r"sizeof\(mpcq_channel_params\) == 256", src)


def test_binding_and_defaults():
    import mpcq
    from mpcq import _lib as L
    assert C.sizeof(L.ChannelParams) == 256
    assert L.ChannelParams.hold_prob.offset == 16 and L.ChannelParams.sigma.offset == 24
    assert L.ChannelParams.bias.offset == 120 and L.ChannelParams.f_sigma.offset == 216
    assert L.ChannelParams.f_gain.offset == 240
    for name in NEW:
        assert name in L.EXPORTS and hasattr(mpcq.lib(), name), name
    assert tuple(getattr(mpcq, "HV_" + n) for n in IDS) == tuple(range(6))
    assert mpcq.lib().mpcq_abi_version() == 3
    junk = L.ChannelParams()
    C.memset(C.byref(junk), 0xFF, 256)
    mpcq.lib().mpcq_default_channel_params(C.byref(junk))
    assert bytes(junk) == bytes(256)  # everything zero: a channel that changes nothing
    p = mpcq.default_channel_params()
    assert isinstance(p, mpcq.ChannelParams) and bytes(p) == bytes(256)
    import channel_model as CM
    m = CM.params()
    for name, _ in L.ChannelParams._fields_:
        v = getattr(p, name)
        assert (list(v) if hasattr(v, "__len__") else v) == getattr(m, name), name
    q = mpcq.default_channel_params(seed=2 ** 63 + 5, delay=3, latency=2, sigma=0.5, f_sigma=[0.1, 0.2, 0.3], f_gain=0.25)
    assert q.seed == 2 ** 63 + 5 and (q.delay, q.latency) == (3, 2) and list(q.sigma) == [0.5] * 12
    assert list(q.f_sigma) == [0.1, 0.2, 0.3] and q.f_gain == 0.25
    with pytest.raises(AttributeError):
        mpcq.default_channel_params(bad=1)
    with pytest.raises(ValueError):
        mpcq.default_channel_params(bias=[0.0, 0.0])
    for name in ("enable_channel", "disable_channel", "channel_read", "channel_device_ptr"):
        assert callable(getattr(mpcq.Session, name)), name
    for name in ("observe", "actuate", "observe_device", "actuate_device"):
        assert callable(getattr(mpcq.Channel, name)), name
    for name in ("normal", "bias", "gain", "held"):
        assert callable(getattr(mpcq.channel, name)), name


def _vec(n, i, v):
    a = [0.0] * n
    a[i] = v
    return a


# (overrides, the field the message must name)
BAD = [(dict(delay=-1), "delay"), (dict(delay=9), "delay"), (dict(latency=5), "latency"), (dict(latency=-1), "latency"),
       (dict(hold_prob=-0.1), "hold_prob"), (dict(hold_prob=1.5), "hold_prob"), (dict(hold_prob=np.nan), "hold_prob"),
       (dict(sigma=_vec(12, 0, -1.0)), "sigma"), (dict(sigma=_vec(12, 11, np.nan)), "sigma"),
       (dict(sigma=_vec(12, 5, np.inf)), "sigma"),
       (dict(bias=_vec(12, 3, -0.5)), "bias"), (dict(bias=_vec(12, 0, np.nan)), "bias"),
       (dict(bias=_vec(12, 11, np.inf)), "bias"),
       (dict(f_sigma=_vec(3, 2, -1.0)), "f_sigma"), (dict(f_sigma=_vec(3, 0, np.nan)), "f_sigma"),
       (dict(f_sigma=_vec(3, 1, np.inf)), "f_sigma"),
       (dict(f_gain=1.0), "f_gain"), (dict(f_gain=-0.1), "f_gain"), (dict(f_gain=np.nan), "f_gain"),
       (dict(f_gain=np.inf), "f_gain"), (dict(reserved=[0, 1]), "reserved")]
GOOD = [dict(), dict(delay=8, latency=4), dict(hold_prob=1.0), dict(hold_prob=0.0, sigma=1e300), dict(f_gain=0.999999),
        dict(seed=2 ** 64 - 1, bias=2.0, f_sigma=[0.0, 3.0, 0.0])]


def _observe(ch, ctx=None):
    """mpcq_channel_observe_batch on sentinel arrays that must come back untouched."""
    from mpcq import _lib as L
    lib = L.lib()
    B = 2
    arrs = dict(truth=np.full((B, 12), 5.0), clock=np.full((B, 2), 7, np.int32), obs=np.full((B, 12), -1.0),
                draw=np.full((B, 16), -2.0), s_ring=np.full((B, 8, 12), -3.0), f_ring=np.full((B, 4, 12), -4.0))
    keep = {k: v.copy() for k, v in arrs.items()}
    p = lambda k: C.c_void_p(arrs[k].ctypes.data)  # noqa: E731
    rc = lib.mpcq_channel_observe_batch(ctx, None if ch is None else C.byref(ch), B, None, 0, p("truth"), p("clock"),
                                        p("obs"), p("draw"), p("s_ring"), p("f_ring"), 0)
    assert all(np.array_equal(arrs[k], keep[k]) for k in arrs)
    return rc, lib.mpcq_last_error().decode()


def _actuate(ch, ctx=None):
    from mpcq import _lib as L
    lib = L.lib()
    B = 2
    arrs = dict(f0=np.full((B, 12), 5.0), clock=np.full((B, 2), 7, np.int32), draw=np.full((B, 16), 2.0),
                f_ring=np.full((B, 4, 12), -4.0), f_cmd=np.full((B, 12), -1.0))
    keep = {k: v.copy() for k, v in arrs.items()}
    p = lambda k: C.c_void_p(arrs[k].ctypes.data)  # noqa: E731
    rc = lib.mpcq_channel_actuate_batch(ctx, None if ch is None else C.byref(ch), B, p("f0"), p("clock"), p("draw"),
                                        p("f_ring"), p("f_cmd"), 0)
    assert all(np.array_equal(arrs[k], keep[k]) for k in arrs)
    return rc, lib.mpcq_last_error().decode()


@pytest.mark.parametrize("bad,field", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b, _ in BAD])
def test_every_validation_rule(bad, field):
    import mpcq
    from mpcq import _lib as L
    for call in (_observe, _actuate):
        rc, msg = call(mpcq.default_channel_params(**bad))
        assert rc == L.E_INVALID and "channel" in msg and field in msg, (bad, msg)
        # f_sigma's message must not pass for sigma's
        if field == "sigma":
            assert "f_sigma" not in msg, msg


def test_valid_parameters_pass_the_validation():
    import mpcq
    from mpcq import _lib as L
    for good in GOOD:
        for call in (_observe, _actuate):
            rc, msg = call(mpcq.default_channel_params(**good))
            assert rc == L.E_INVALID and "ctx is NULL" in msg, (good, msg)  # the next check, not the parameters
    rc, msg = _observe(None)  # NULL = the defaults
    assert rc == L.E_INVALID and "ctx is NULL" in msg


def test_null_arguments_without_a_device():
    """Every entry point refuses NULL with MPCQ_E_INVALID before it touches a device."""
    from mpcq import _lib as L
    lib = L.lib()
    lib.mpcq_default_channel_params(None)  # a no-op
    out = C.c_void_p()
    buf = np.zeros(16)
    assert lib.mpcq_session_enable_channel(None, None) == L.E_INVALID
    assert "NULL" in lib.mpcq_last_error().decode()
    assert lib.mpcq_session_disable_channel(None) == L.E_INVALID
    assert lib.mpcq_session_channel_read(None, 0, C.c_void_p(buf.ctypes.data), 0) == L.E_INVALID
    assert lib.mpcq_session_channel_device_ptr(None, 0, C.byref(out)) == L.E_INVALID
    assert out.value is None
    rc, msg = _observe(None)
    assert rc == L.E_INVALID and "NULL" in msg
    rc, msg = _actuate(None)
    assert rc == L.E_INVALID and "NULL" in msg


class _Engine:
    """Stands in for the native library: records the calls, refuses what the test tells it to."""

    def __init__(self):
        self.calls, self.refuse = [], False

    def _call(self, name, *args):
        from mpcq import _lib as L
        if self.refuse:
            raise L.MpcqError(L.E_INVALID, "the channel needs delay in 0..8 (got 9)")
        self.calls.append((name, args))


def _session():
    import mpcq

    class Stubbed(mpcq.Session):
        def close(self):  # (the handle is not the library's)
            self._h = None

    s = object.__new__(Stubbed)
    s.engine, s._h, s.channel_params, s.batch = _Engine(), C.c_void_p(1), None, 5
    return s


def test_session_enable_channel_overrides_and_refusals():
    import mpcq
    from mpcq import _lib as L
    s = _session()
    s.enable_channel(delay=3, latency=2, hold_prob=0.2, sigma=0.01, f_gain=0.1, seed=9)
    name, args = s.engine.calls[-1]
    assert name == "mpcq_session_enable_channel" and args[0] is s._h
    sent = args[1]._obj
    assert isinstance(sent, L.ChannelParams) and sent is s.channel_params
    assert (sent.seed, sent.delay, sent.latency, sent.hold_prob, sent.f_gain) == (9, 3, 2, 0.2, 0.1)
    assert list(sent.sigma) == [0.01] * 12 and list(sent.bias) == [0.0] * 12
    s.enable_channel()  # the defaults: all zero
    assert bytes(s.engine.calls[-1][1][1]._obj) == bytes(256)
    mine = mpcq.default_channel_params(delay=1)
    s.enable_channel(mine)
    assert s.engine.calls[-1][1][1]._obj is mine and s.channel_params is mine
    with pytest.raises(ValueError):
        s.enable_channel(mine, delay=2)
    with pytest.raises(AttributeError):
        s.enable_channel(dely=2)
    # a refusal of the library reaches the caller, and the parameters in force stay
    s.engine.refuse = True
    with pytest.raises(L.MpcqError) as e:
        s.enable_channel(delay=9)
    assert "delay" in str(e.value) and s.channel_params is mine
    s.engine.refuse = False
    s.disable_channel()
    assert s.engine.calls[-1][0] == "mpcq_session_disable_channel" and s.channel_params is None
    with pytest.raises(L.MpcqError):
        s._group_shape("channel", 6)
    assert s._group_shape("channel", L.HV_S_RING) == ((5, 8, 12), np.float64) and s._group_shape("channel", L.HV_CLOCK) == ((5, 2), np.int32)
