"""CPU: the scenario stage through the layers that need no device -- the header's declarations,
the ctypes binding, the defaults, and every validation rule of mpcq_scenario_step_batch, which
checks its parameters before it looks at anything else (so before any device work: here the
context is NULL, and a call whose parameters pass fails on that instead)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")
NEW = ("mpcq_default_scenario_params", "mpcq_scenario_step_batch", "mpcq_session_enable_scenario",
       "mpcq_session_disable_scenario", "mpcq_session_scenario_read", "mpcq_session_scenario_device_ptr")


def test_header_declares_the_scenario():
    src = open(HEADER).read()
    for name in NEW:
        assert re.search(rf"\b(int|void)\s+{name}\(", src), name
    for name, val in (("MPCQ_CV_EPOCH", 0), ("MPCQ_CV_TICK", 1), ("MPCQ_CV_V_REF", 2), ("MPCQ_CV_PUSH", 3),
                      ("MPCQ_CV_WRENCH", 4), ("MPCQ_CV_ROBOTS", 5), ("MPCQ_CV_DRAW", 6), ("MPCQ_CV_COUNT", 7),
                      ("MPCQ_ABI_VERSION", 3), ("MPCQ_SV_COUNT", 21), ("MPCQ_PV_COUNT", 3), ("MPCQ_MV_COUNT", 6)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", src), name
    assert re.search(r"sizeof\(mpcq_scenario_params\) == 256", src)


def test_binding_and_defaults():
    import mpcq
    from mpcq import _lib as L
    assert C.sizeof(L.ScenarioParams) == 256
    for name in NEW:
        assert name in L.EXPORTS and hasattr(mpcq.lib(), name), name
    assert (mpcq.CV_EPOCH, mpcq.CV_TICK, mpcq.CV_V_REF, mpcq.CV_PUSH, mpcq.CV_WRENCH, mpcq.CV_ROBOTS, mpcq.CV_DRAW) == \
        tuple(range(7))
    p = mpcq.default_scenario_params()
    assert isinstance(p, mpcq.ScenarioParams)
    assert p.seed == 0 and p.commands == 1 and list(p.v_lo) == [1.0, 0.0, 0.0] and list(p.v_hi) == [1.0, 0.0, 0.0]
    assert (p.cmd_start, p.cmd_ramp, p.cmd_period) == (48, 175, 0)
    assert (p.pushes, p.push_first, p.push_period, p.push_jitter, p.push_ticks, p.push_flip) == (0, 0, 0, 0, 10, 0)
    assert p.push_prob == 1.0 and list(p.wrench_lo) == [0.0] * 6 and list(p.wrench_hi) == [0.0] * 6
    assert (p.mass_scale_lo, p.mass_scale_hi, p.mu_lo, p.mu_hi) == (1.0, 1.0, 0.9, 0.9)
    assert p.robots == 0 and list(p.reserved) == [0] * 5
    # the model's defaults are the library's
    import scenario_model as SM
    m = SM.params()
    for name, _ in L.ScenarioParams._fields_:
        v = getattr(p, name)
        assert (list(v) if hasattr(v, "__len__") else v) == getattr(m, name), name
    q = mpcq.default_scenario_params(seed=2 ** 63 + 5, v_lo=[0.1, 0.2, 0.3], push_flip=63, robots=3)
    assert q.seed == 2 ** 63 + 5 and list(q.v_lo) == [0.1, 0.2, 0.3] and (q.push_flip, q.robots) == (63, 3)
    with pytest.raises(AttributeError):
        mpcq.default_scenario_params(bad=1)
    with pytest.raises(ValueError):
        mpcq.default_scenario_params(v_lo=[0.0, 0.0])
    for name in ("enable_scenario", "disable_scenario", "scenario_read", "scenario_device_ptr"):
        assert callable(getattr(mpcq.Session, name)), name
    assert callable(mpcq.Scenario.step) and callable(mpcq.Scenario.step_device)
    assert callable(mpcq.scenario.constants) and callable(mpcq.scenario.command) and callable(mpcq.scenario.push)


BAD = [dict(v_lo=[np.nan, 0.0, 0.0]), dict(v_hi=[1.0, np.inf, 0.0]), dict(v_lo=[1.5, 0.0, 0.0]),
       dict(v_lo=[1.0, 0.0, 0.1]), dict(wrench_lo=[0.0, 0.0, 0.0, 0.0, 0.0, 1.0]),
       dict(wrench_hi=[0.0, -np.inf, 0.0, 0.0, 0.0, 0.0]), dict(wrench_lo=[np.nan] + [0.0] * 5),
       dict(mass_scale_lo=np.nan), dict(mass_scale_lo=1.5), dict(mass_scale_hi=np.inf), dict(mu_lo=0.95),
       dict(mu_hi=np.nan),
       dict(robots=1, mass_scale_lo=0.0), dict(robots=1, mass_scale_lo=-0.5), dict(robots=3, mass_scale_lo=0.0),
       dict(robots=2, mu_lo=0.0), dict(robots=2, mu_lo=-0.1), dict(robots=3, mu_lo=0.0),
       dict(push_prob=-0.1), dict(push_prob=1.5), dict(push_prob=np.nan),
       dict(commands=-1), dict(cmd_start=-1), dict(cmd_ramp=-1), dict(cmd_period=-1), dict(pushes=-1),
       dict(push_first=-1), dict(push_period=-1), dict(push_jitter=-1), dict(push_ticks=-1), dict(push_flip=-1),
       dict(robots=-1),
       dict(pushes=1, push_ticks=0),
       dict(cmd_period=222), dict(cmd_start=4, cmd_ramp=3, cmd_period=6),
       dict(pushes=1, push_period=5, push_jitter=3, push_ticks=3), dict(push_period=9),
       dict(robots=4), dict(robots=7), dict(push_flip=64),
       dict(reserved=[1, 0, 0, 0, 0]), dict(reserved=[0, 0, 0, 0, -1])]
GOOD = [dict(), dict(cmd_period=223), dict(cmd_start=4, cmd_ramp=3, cmd_period=7),
        dict(pushes=1, push_period=5, push_jitter=3, push_ticks=2), dict(push_ticks=0), dict(push_period=10),
        dict(mass_scale_lo=0.0, mass_scale_hi=0.0), dict(mu_lo=-1.0, mu_hi=0.5), dict(robots=3, push_flip=63),
        dict(push_prob=0.0), dict(seed=2 ** 64 - 1)]


def _call(sc, ctx=None):
    from mpcq import _lib as L
    lib = L.lib()
    B = 2
    epoch, tick = np.full(B, 7, np.int32), np.full(B, 9, np.int32)
    out = [np.full((B, 6), -1.0) for _ in range(3)]
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = lib.mpcq_scenario_step_batch(ctx, None if sc is None else C.byref(sc), B, None, 0, p(epoch), p(tick), None,
                                      None, p(out[0]), p(out[1]), p(out[2]), None, None, 0)
    assert epoch.tolist() == [7, 7] and tick.tolist() == [9, 9] and all((o == -1.0).all() for o in out)
    return rc, lib.mpcq_last_error().decode()


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(d))
def test_every_validation_rule(bad):
    import mpcq
    from mpcq import _lib as L
    rc, msg = _call(mpcq.default_scenario_params(**bad))
    assert rc == L.E_INVALID and "scenario" in msg, (bad, msg)


def test_valid_parameters_pass_the_validation():
    import mpcq
    from mpcq import _lib as L
    for good in GOOD:
        rc, msg = _call(mpcq.default_scenario_params(**good))
        assert rc == L.E_INVALID and "ctx is NULL" in msg, (good, msg)  # the next check, not the parameters
    rc, msg = _call(None)  # NULL = the defaults
    assert rc == L.E_INVALID and "ctx is NULL" in msg
