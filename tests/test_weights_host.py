"""CPU: the mpcq_weights ABI, its Python mirrors, and the power of tests/weight_cases.py.

test_gpu_weights.py compares the engine under a per-instance weights table with per-instance
oracle solves.  That comparison only means something if the table moves every instance: the power
test below re-establishes, from the oracle alone and at every horizon of the table, that

* every instance is SOLVED;
* the oracle's checker build and its -O3 -march=native build agree on status and iteration
  count on every instance (no instance on a rounding knife-edge);
* every instance's f0 moves by more than 1e-5 (200x the GPU tolerance) from the default weights'
  result and from the result under its neighbour's row (weights[(b + 1) % B]): a kernel that
  ignored the table, or read another row, would miss.

These are conditions on the inputs, not tolerances: a recipe that fails them is replaced, not
relaxed.

The validation of a host table runs behind a context, which needs a device: what is reachable
here is the refusal of NULL handles and the checks the Python layer makes before the call
(test_gpu_weights.py::test_validation has the rules that name index and field).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import weight_cases as WC
from conftest import REPO

HEADER = os.path.join(REPO, "include", "mpcq.h")
NEW = ("mpcq_default_weights", "mpcq_set_weights", "mpcq_session_set_weights", "mpcq_session_get_weights")


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as m
    m.build()
    return m


def test_weights_struct_layout(mpcq):
    L = mpcq._lib
    assert C.sizeof(L.Weights) == 128
    assert [(n, getattr(L.Weights, n).offset) for n, _ in L.Weights._fields_] == [
        ("state", 0), ("force", 96), ("reserved", 104)]
    dt = mpcq.WEIGHTS_DTYPE
    assert dt.itemsize == 128
    assert [(n, dt.fields[n][1], dt.fields[n][0].shape) for n in dt.names] == [
        ("state", 0, (12,)), ("force", 96, ()), ("reserved", 104, (3,))]
    src = open(HEADER).read()
    assert src.count("_Static_assert(sizeof(mpcq_weights) == 128") == 1
    assert src.count("static_assert(sizeof(mpcq_weights) == 128") == 1  # (the C++ spelling)


def test_header_and_binding(mpcq):
    src = open(HEADER).read()
    for name in NEW:
        assert re.search(rf"\b(int|void)\s+{name}\(", src), name
        assert name in mpcq._lib.EXPORTS and hasattr(mpcq.lib(), name), name
    # additive: the version and every existing count stay
    for name, val in (("MPCQ_ABI_VERSION", 3), ("MPCQ_SV_COUNT", 21)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", src), name
    assert mpcq.lib().mpcq_abi_version() == 3
    assert C.sizeof(mpcq._lib.Robot) == 128 and mpcq.ROBOT_DTYPE.itemsize == 128
    for cls, name in ((mpcq.Engine, "set_weights"), (mpcq.Engine, "set_weights_device"),
                      (mpcq.Session, "set_weights"), (mpcq.Session, "get_weights")):
        assert callable(getattr(cls, name)), name
    # the sentence the weights table makes wrong is gone from the header
    robot_doc = src[src.index("---- per-robot constants"):src.index("typedef struct mpcq_robot")]
    assert "weights, footholds" not in robot_doc and "mpcq_weights" in robot_doc


def test_default_weights_equals_default_params(mpcq):
    p = mpcq.default_params()
    for w in (mpcq.default_weights(), mpcq.default_weights(p)):
        assert list(w.state) == list(p.state_weights) and w.force == p.force_weight
        assert list(w.reserved) == [0.0] * 3
    sw = tuple(float(v) for v in range(1, 13))
    q = mpcq.default_params(state_weights=(C.c_double * 12)(*sw), force_weight=3e-4)
    w = mpcq.default_weights(q)
    assert (tuple(w.state), w.force) == (sw, 3e-4)
    mpcq.lib().mpcq_default_weights(None, None)  # a NULL output is ignored, never a crash
    mpcq.lib().mpcq_default_weights(C.byref(q), None)


def test_weights_broadcasting_and_defaults(mpcq):
    p = mpcq.default_params()
    sw0 = np.array(p.state_weights[:])
    t = mpcq.weights(5)
    assert t.shape == (5,) and t.dtype == mpcq.WEIGHTS_DTYPE and t.flags.c_contiguous
    assert (t["state"] == sw0).all() and (t["force"] == p.force_weight).all() and (t["reserved"] == 0).all()
    # scalar, (12,), (B,12) state and scalar, (B,) force; the rest from params
    q = mpcq.default_params(force_weight=2e-5)
    s1 = np.arange(12.0) + 1
    t = mpcq.weights(5, state=s1, params=q)
    assert (t["state"] == s1).all() and (t["force"] == 2e-5).all()
    sB = np.arange(60.0).reshape(5, 12) + 1
    fB = np.linspace(1e-6, 1e-3, 5)
    t = mpcq.weights(5, state=sB, force=fB)
    assert np.array_equal(t["state"], sB) and np.array_equal(t["force"], fB)
    t2 = mpcq.weights(5, state=0.5, force=1e-4)
    assert (t2["state"] == 0.5).all() and (t2["force"] == 1e-4).all()
    # the bytes of a row are a mpcq_weights
    w = mpcq.Weights.from_buffer_copy(t[2].tobytes())
    assert list(w.state) == sB[2].tolist() and w.force == fB[2] and list(w.reserved) == [0.0] * 3
    with pytest.raises(ValueError):
        mpcq.weights(5, state=np.ones((4, 12)))
    with pytest.raises(ValueError):
        mpcq.weights(5, state=np.ones(11))
    with pytest.raises(ValueError):
        mpcq.weights(5, force=np.ones(4))


def test_recipe_is_the_documented_one(mpcq):
    """The first instance of N = 16 drawn by hand in the documented order."""
    d = mpcq.default_params()
    rng = np.random.default_rng(916)
    fac = np.exp(rng.uniform(-np.log(4), np.log(4), 12))
    force = 1e-5 * 10 ** rng.uniform(-1, 2)
    t = WC.make_weights(16)
    assert t.shape == (16,) and t.dtype == mpcq.WEIGHTS_DTYPE
    assert np.array_equal(t["state"][0], np.array(d.state_weights[:]) * fac)
    assert t["force"][0] == force
    r = t["state"] / np.array(d.state_weights[:])
    assert (r >= 0.25).all() and (r <= 4.0).all() and (t["force"] >= 1e-6).all() and (t["force"] <= 1e-3).all()
    assert (t["reserved"] == 0).all()


@pytest.mark.parametrize("N", WC.HORIZONS)
def test_recipe_has_power(oracle, N):
    w = WC.make_weights(N)
    B = w.shape[0]
    assert B == (16 if N <= 20 else 8)
    r = WC.oracle_solve(oracle, N, w, key="table")
    nat = WC.oracle_solve(oracle, N, w, native=True)
    dflt = WC.oracle_solve(oracle, N, None)
    nb = WC.oracle_solve(oracle, N, np.roll(w, -1))  # instance b under weights[(b + 1) % B]
    assert (r["status"] == 1).all(), r["status"]
    assert np.array_equal(r["status"], nat["status"])
    assert np.array_equal(r["iters"], nat["iters"]), (r["iters"], nat["iters"])
    assert r["iters"].max() < 4000
    d_nat = float(np.abs(r["f0"] - nat["f0"]).max())
    mv_d = np.abs(r["f0"] - dflt["f0"]).max(axis=1)
    mv_n = np.abs(r["f0"] - nb["f0"]).max(axis=1)
    print(f"N={N}: iters {r['iters'].min()}..{r['iters'].max()}, builds differ by {d_nat:.1e}, "
          f"movement vs defaults >= {mv_d.min():.2e}, vs the neighbour's row >= {mv_n.min():.2e}")
    assert (mv_d > 1e-5).all(), mv_d
    assert (mv_n > 1e-5).all(), mv_n


def test_null_handles_are_codes_not_crashes(mpcq):
    lib, E = mpcq.lib(), mpcq._lib.E_INVALID
    t = mpcq.weights(3)
    p = C.c_void_p(t.ctypes.data)
    assert lib.mpcq_set_weights(None, 3, p, 0) == E and b"ctx is NULL" in lib.mpcq_last_error()
    assert lib.mpcq_session_set_weights(None, p, 0) == E and b"session is NULL" in lib.mpcq_last_error()
    assert lib.mpcq_session_get_weights(None, p, 0) == E and b"session is NULL" in lib.mpcq_last_error()


class _Recorder:
    """Stands in for the Engine: copies what the pointers of a call hold while they are alive."""

    def __init__(self):
        self.calls = []

    def _call(self, name, h, *args):
        self.calls.append((name,) + args)


def test_python_table_checks(mpcq):
    """What the Python layer refuses before the call: another dtype, another rank, a session table
    of another length.  A ctypes array of L.Weights is accepted as it is."""
    from mpcq.engine import _weights_table
    t = mpcq.weights(4, state=2.0)
    assert _weights_table(t, 4) is not None
    arr = (mpcq.Weights * 2)(mpcq.default_weights(), mpcq.default_weights())
    assert _weights_table(arr).tobytes() == mpcq.weights(2).tobytes()
    for bad in (mpcq.robots(4), np.zeros((4, 16)), t.reshape(2, 2)):
        with pytest.raises(ValueError):
            _weights_table(bad)
    with pytest.raises(ValueError):
        _weights_table(t, 5)
    s = mpcq.Session.__new__(mpcq.Session)
    s.engine, s.batch, s._h = _Recorder(), 4, None
    with pytest.raises(ValueError):
        s.set_weights(mpcq.weights(3))
    assert s.engine.calls == []
    s.set_weights(None)
    assert s.engine.calls == [("mpcq_session_set_weights", None, 0)]
