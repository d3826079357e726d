"""CPU: the gait stage through the layers that need no device -- the header's declarations, the
ctypes binding, the defaults, every validation rule of parameters and cycles (the batch entry
point checks them before anything else, so here the context is NULL and a call whose parameters
pass fails on that instead), NULL arguments of every entry point, and Session.enable_gait /
set_gait with the native call stubbed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import REPO

import gait_cases as GC
import gait_model as GM

HEADER = os.path.join(REPO, "include", "mpcq.h")
NEW = ("mpcq_default_gait_params", "mpcq_gait_roll_batch", "mpcq_session_enable_gait", "mpcq_session_disable_gait",
       "mpcq_session_set_gait", "mpcq_session_gait_read", "mpcq_session_gait_device_ptr")
CONSTS = (("MPCQ_GAIT_MAX", 8), ("MPCQ_GAIT_MANUAL", 0), ("MPCQ_GAIT_BY_SPEED", 1), ("MPCQ_GV_STATE", 0),
          ("MPCQ_GV_COUNT", 1))
# what the issue pins as unchanged
KEPT = (("MPCQ_ABI_VERSION", 3), ("MPCQ_SV_COUNT", 21), ("MPCQ_EV_COUNT", 2), ("MPCQ_HV_COUNT", 6), ("MPCQ_CV_COUNT", 7),
        ("MPCQ_MV_COUNT", 6), ("MPCQ_PV_COUNT", 3))


def test_header_declares_the_gait_stage():
    src = open(HEADER).read()
    for name in NEW:
        assert re.search(rf"\b(int|void)\s+{name}\(", src), name
    for name, val in CONSTS + KEPT:
        assert re.search(rf"#define\s+{name}\s+{val}\b", src), name
    assert len(re.findall(r"sizeof\(mpcq_gait_params\) == 128", src)) == 2  # C and C++
    assert "mpcq_gait_roll_batch" in src.split("#define MPCQ_ABI_VERSION")[0]  # the changelog line
    internal = open(os.path.join(REPO, "mpc-tsid_amd", "csrc", "mpcq_internal.h")).read()
    assert re.search(r"constexpr int kGatherMax = 48;", internal)  # the gather launch is untouched
    mk = open(os.path.join(REPO, "mpc-tsid_amd", "csrc", "Makefile")).read()
    assert "$(B)/mpcq_gait.o" in mk
    assert os.path.exists(os.path.join(REPO, "mpc-tsid_amd", "csrc", "mpcq_gait.hip"))


def test_binding_and_defaults():
    import mpcq
    from mpcq import _lib as L
    G = L.GaitParams
    assert C.sizeof(G) == 128
    assert (G.n_gaits.offset, G.select.offset, G.align.offset, G.reserved0.offset) == (0, 4, 8, 12)
    assert (G.thresholds.offset, G.hysteresis.offset, G.yaw_weight.offset, G.reserved.offset) == (16, 72, 80, 88)
    for name in NEW:
        assert name in L.EXPORTS and hasattr(mpcq.lib(), name), name
    assert (mpcq.GV_STATE, mpcq.GAIT_MAX, mpcq.GAIT_MANUAL, mpcq.GAIT_BY_SPEED) == (0, 8, 0, 1)
    assert (GM.GAIT_MAX, GM.MANUAL, GM.BY_SPEED) == (L.GAIT_MAX, L.GAIT_MANUAL, L.GAIT_BY_SPEED)
    assert mpcq.lib().mpcq_abi_version() == 3
    junk = G()
    C.memset(C.byref(junk), 0xFF, 128)
    mpcq.lib().mpcq_default_gait_params(C.byref(junk))
    p = mpcq.default_gait_params()
    assert isinstance(p, mpcq.GaitParams) and bytes(p) == bytes(junk)
    m = GM.params()
    for name, _ in G._fields_:
        v = getattr(p, name)
        assert (list(v) if hasattr(v, "__len__") else v) == getattr(m, name), name
    assert (p.n_gaits, p.select, p.align) == (0, 0, 1) and list(p.thresholds) == [math.inf] * 7
    assert p.yaw_weight == math.sqrt(0.19 ** 2 + 0.15005 ** 2) == GM.YAW_WEIGHT
    q = mpcq.default_gait_params(n_gaits=3, select=1, thresholds=[0.1, 0.5], hysteresis=0.05, align=0)
    assert (q.n_gaits, q.select, q.align, q.hysteresis) == (3, 1, 0, 0.05)
    assert list(q.thresholds) == [0.1, 0.5] + [math.inf] * 5
    with pytest.raises(AttributeError):
        mpcq.default_gait_params(bad=1)
    with pytest.raises(ValueError):
        mpcq.default_gait_params(thresholds=[0.0] * 8)
    for name in ("enable_gait", "disable_gait", "set_gait", "set_gait_device", "gait_state"):
        assert callable(getattr(mpcq.Session, name)), name
    for name in ("roll", "roll_device"):
        assert callable(getattr(mpcq.Gait, name)), name
    assert np.array_equal(mpcq.gait.new_state(3), GM.new_state(3))


def test_cycle_builder_matches_the_cases_and_the_planner_tables():
    import mpcq
    from mpcq import synth
    for name in ("trot", "bound", "pace", "stand"):
        assert np.array_equal(mpcq.gait.cycle(name), GC.cycle(name)), name
        assert GM.check_cycle(mpcq.gait.cycle(name)) is None
    assert np.array_equal(mpcq.gait.cycle("side"), mpcq.gait.cycle("pace"))
    for name in ("trot", "bound", "pace"):  # one period of the table a planner runs
        assert np.array_equal(mpcq.gait.cycle(name), synth.gait_table(name, 16))
        assert np.array_equal(mpcq.gait.cycle(name, dt=0.02, T_gait=0.24)[:4, 0], (1, 5, 1, 5))
    assert GM.period(mpcq.gait.cycle("stand")) == 1 and GM.period(mpcq.gait.cycle("trot")) == 16
    with pytest.raises(ValueError):
        mpcq.gait.cycle("gallop")
    with pytest.raises(ValueError):
        mpcq.gait.library([])
    with pytest.raises(ValueError):
        mpcq.gait.library(["trot"] * 9)
    assert mpcq.gait.library(["stand", GC.cycle("trot")]).shape == (2, 20, 5)


def _roll(gp, cycles, ctx=None, drop=None, select_vref=True):
    """mpcq_gait_roll_batch on sentinel arrays that must come back untouched."""
    from mpcq import _lib as L
    lib = L.lib()
    B = 2
    arrs = dict(v_ref=np.full((B, 6), 0.5), gait=np.full((B, 20, 5), 3.0), gstate=np.full((B, 4), 7, np.int32))
    keep = {k: v.copy() for k, v in arrs.items()}
    p = lambda k: None if k == drop else C.c_void_p(arrs[k].ctypes.data)  # noqa: E731
    cy = None if cycles is None else np.ascontiguousarray(cycles, np.float64)
    rc = lib.mpcq_gait_roll_batch(ctx, None if gp is None else C.byref(gp), None if cy is None else C.c_void_p(cy.ctypes.data),
                                  B, p("v_ref"), p("gait"), p("gstate"), 0)
    assert all(np.array_equal(arrs[k], keep[k]) for k in arrs)
    return rc, lib.mpcq_last_error().decode()


# (overrides, the field the message must name)
BAD = [(dict(n_gaits=0), "n_gaits"), (dict(n_gaits=9), "n_gaits"), (dict(n_gaits=-1), "n_gaits"),
       (dict(select=2), "select"), (dict(select=-1), "select"), (dict(align=2), "align"), (dict(align=-1), "align"),
       (dict(thresholds=[math.nan, 1.0]), "thresholds[0]"), (dict(thresholds=[0.5, math.nan]), "thresholds[1]"),
       (dict(thresholds=[0.5, 0.25]), "thresholds[1]"), (dict(thresholds=[math.inf, 1.0]), "thresholds[1]"),
       (dict(hysteresis=-1e-9), "hysteresis"), (dict(hysteresis=math.nan), "hysteresis"), (dict(hysteresis=math.inf), "hysteresis"),
       (dict(yaw_weight=-1.0), "yaw_weight"), (dict(yaw_weight=math.nan), "yaw_weight"), (dict(yaw_weight=math.inf), "yaw_weight"),
       (dict(reserved0=1), "reserved"), (dict(reserved=[0, 0, 0, 0, 1e-300]), "reserved"), (dict(reserved=[-0.0, 0, 0, 0, 0]), None)]
GOOD = [dict(), dict(select=1), dict(align=0), dict(thresholds=[0.25, 0.25]), dict(thresholds=[-math.inf, math.inf]),
        dict(thresholds=[0.1, 0.2, math.nan]),  # beyond the first n_gaits - 1: not read
        dict(hysteresis=1e300, yaw_weight=0.0), dict(n_gaits=1, thresholds=[math.nan] * 7)]


@pytest.mark.parametrize("bad,field", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b, _ in BAD])
def test_every_parameter_rule(bad, field):
    import mpcq
    from mpcq import _lib as L
    kw = dict(n_gaits=3)
    kw.update(bad)
    rc, msg = _roll(mpcq.default_gait_params(**kw), GC.LIB[:3])
    if field is None:  # -0.0 compares equal to zero: passes the parameter rules
        assert rc == L.E_INVALID and "ctx is NULL" in msg
        return
    assert rc == L.E_INVALID and "gait" in msg and field in msg, (bad, msg)


def _broken(g, r, c, v, lib=None):
    cy = (GC.LIB[:3] if lib is None else lib).copy()
    cy[g, r, c] = v
    return cy


BAD_CYCLES = [(_broken(0, 0, 0, 0.0), 0, 0, "count"), (_broken(1, 1, 0, 65.0), 1, 1, "count"), (_broken(1, 1, 0, 1.5), 1, 1, "count"),
              (_broken(2, 0, 0, -1.0), 2, 0, "count"), (_broken(0, 2, 0, math.nan), 0, 2, "count"),
              (_broken(0, 1, 2, 0.5), 0, 1, "contact"), (_broken(1, 3, 4, 2.0), 1, 3, "contact"),
              (_broken(1, 0, 1, math.nan), 1, 0, "contact"), (_broken(2, 0, 3, -1.0), 2, 0, "contact"),
              (_broken(0, 4, 1, 1.0), 0, 4, "contact"),     # the terminator row's contacts
              (_broken(0, 7, 0, 2.0), 0, 7, "count"),       # behind the terminator
              (_broken(2, 19, 4, 1.0), 2, 19, "contact"), (_broken(1, 4, 0, -0.0), 1, 4, "count"),
              (np.stack([np.tile([1.0, 1, 1, 1, 1], (20, 1))] * 3), 0, 19, "count")]  # 20 rows: no terminator


@pytest.mark.parametrize("i", range(len(BAD_CYCLES)))
def test_every_cycle_rule(i):
    import mpcq
    from mpcq import _lib as L
    cy, g, r, field = BAD_CYCLES[i]
    assert GM.check_cycle(cy[g]) == (r, field)  # the model names the same row and field
    assert all(GM.check_cycle(cy[h]) is None for h in range(g))
    rc, msg = _roll(mpcq.default_gait_params(n_gaits=3), cy)
    assert rc == L.E_INVALID and f"gait {g}, row {r}:" in msg and field in msg, msg
    # an entry past n_gaits is not read
    if g > 0:
        rc, msg = _roll(mpcq.default_gait_params(n_gaits=g), cy)
        assert rc == L.E_INVALID and "ctx is NULL" in msg, msg


def test_valid_parameters_pass_the_validation():
    import mpcq
    from mpcq import _lib as L
    for good in GOOD:
        kw = dict(n_gaits=3)
        kw.update(good)
        rc, msg = _roll(mpcq.default_gait_params(**kw), GC.LIB[:3])
        assert rc == L.E_INVALID and "ctx is NULL" in msg, (good, msg)  # the next check, not the parameters
    full = np.stack([GC.cycle("trot")] * 8)
    full[7, :19, 0] = 64.0  # 19 rows of 64 steps: the longest cycle
    full[7, :19, 1:] = 1.0
    full[7, 19] = 0.0
    assert GM.check_cycle(full[7]) is None
    rc, msg = _roll(mpcq.default_gait_params(n_gaits=8), full)
    assert rc == L.E_INVALID and "ctx is NULL" in msg, msg


def test_null_arguments_without_a_device():
    """Every entry point refuses NULL with MPCQ_E_INVALID before it touches a device."""
    import mpcq
    from mpcq import _lib as L
    lib = L.lib()
    lib.mpcq_default_gait_params(None)  # a no-op
    out = C.c_void_p()
    buf = np.zeros(16, np.int32)
    gp = mpcq.default_gait_params(n_gaits=3)
    cy = np.ascontiguousarray(GC.LIB[:3])
    assert lib.mpcq_session_enable_gait(None, C.byref(gp), C.c_void_p(cy.ctypes.data)) == L.E_INVALID
    assert "NULL" in lib.mpcq_last_error().decode()
    assert lib.mpcq_session_disable_gait(None) == L.E_INVALID
    assert lib.mpcq_session_set_gait(None, C.c_void_p(buf.ctypes.data), 0) == L.E_INVALID
    assert lib.mpcq_session_gait_read(None, 0, C.c_void_p(buf.ctypes.data), 0) == L.E_INVALID
    assert lib.mpcq_session_gait_device_ptr(None, 0, C.byref(out)) == L.E_INVALID
    assert out.value is None
    for gpp, cyy, word in ((None, cy, "parameters"), (gp, None, "cycles")):
        rc, msg = _roll(gpp, cyy)
        assert rc == L.E_INVALID and "NULL" in msg and word in msg
    # a bad parameter wins over a NULL context and a NULL array: the parameters are checked first
    rc, msg = _roll(mpcq.default_gait_params(n_gaits=9), cy, drop="gait")
    assert rc == L.E_INVALID and "n_gaits" in msg


class _Engine:
    """Stands in for the native library: records the calls, refuses what the test tells it to."""

    def __init__(self):
        self.calls, self.refuse = [], False

    def _call(self, name, *args):
        from mpcq import _lib as L
        if self.refuse:
            raise L.MpcqError(L.E_INVALID, "the gait library needs n_gaits in 1..8 (got 9)")
        self.calls.append((name, args))


def _session():
    import mpcq

    class Stubbed(mpcq.Session):
        def close(self):  # (the handle is not the library's)
            self._h = None

    s = object.__new__(Stubbed)
    s.engine, s._h, s.gait_params, s.gait_cycles, s.batch = _Engine(), C.c_void_p(1), None, None, 5
    return s


def test_session_enable_gait_and_set_gait():
    import mpcq
    from mpcq import _lib as L
    s = _session()
    s.enable_gait(["stand", "trot", GC.cycle("bound")], select=mpcq.GAIT_BY_SPEED, thresholds=[0.1, 0.6], hysteresis=0.05)
    name, args = s.engine.calls[-1]
    assert name == "mpcq_session_enable_gait" and args[0] is s._h
    sent = args[1]._obj
    assert isinstance(sent, L.GaitParams) and sent is s.gait_params
    assert (sent.n_gaits, sent.select, sent.align, sent.hysteresis) == (3, 1, 1, 0.05)
    assert list(sent.thresholds)[:3] == [0.1, 0.6, math.inf]
    assert args[2].value == s.gait_cycles.ctypes.data and s.gait_cycles.shape == (3, 20, 5)
    assert np.array_equal(s.gait_cycles, np.stack([GC.cycle("stand"), GC.cycle("trot"), GC.cycle("bound")]))
    mine = mpcq.default_gait_params(n_gaits=1, align=0)
    s.enable_gait(["trot"], mine)
    assert s.engine.calls[-1][1][1]._obj is mine and s.gait_params is mine
    with pytest.raises(ValueError):
        s.enable_gait(["trot"], mine, align=1)
    with pytest.raises(AttributeError):
        s.enable_gait(["trot"], alignn=1)
    # a refusal of the library reaches the caller, and the settings in force stay
    s.engine.refuse = True
    with pytest.raises(L.MpcqError) as e:
        s.enable_gait(["trot"], n_gaits=9)
    assert "n_gaits" in str(e.value) and s.gait_params is mine and s.gait_cycles.shape == (1, 20, 5)
    s.engine.refuse = False
    s.set_gait(2)  # a scalar broadcasts
    name, args = s.engine.calls[-1]
    assert name == "mpcq_session_set_gait" and args[2] == 0
    got = np.ctypeslib.as_array(C.cast(args[1], C.POINTER(C.c_int32)), (5,))
    assert got.tolist() == [2] * 5
    s.set_gait([0, 1, -1, 2, 0])
    got = np.ctypeslib.as_array(C.cast(s.engine.calls[-1][1][1], C.POINTER(C.c_int32)), (5,))
    assert got.tolist() == [0, 1, -1, 2, 0]
    with pytest.raises(ValueError):
        s.set_gait([0, 1])
    s.set_gait_device(4096, asynchronous=True)
    name, args = s.engine.calls[-1]
    assert name == "mpcq_session_set_gait" and args[1].value == 4096 and args[2] == L.FLAG_DEVICE_PTRS | L.FLAG_ASYNC
    s.disable_gait()
    assert s.engine.calls[-1][0] == "mpcq_session_disable_gait" and s.gait_params is None
