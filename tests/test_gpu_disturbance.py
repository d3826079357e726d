"""GPU: the per-instance constant disturbance acceleration in batch solves and sessions
(mpcq_set_disturbance, mpcq_session_set_disturbance) against the oracle's formulate + shifted
bounds + qp_solve, instance by instance, and against the same engine bit for bit.

The table and the inputs are tests/disturbance_cases.py's (test_disturbance_host.py shows on the
oracle that every instance's f0 moves by at least 0.59 from the unshifted result and by at least
0.5 from the result under its neighbour's row, so an engine that ignored the table or indexed it
by workgroup instead of by instance cannot pass).  Tolerances are tests/test_gpu_params.py's:
FORM_TOL = 1e-13 on l and u (relative to max(1, |value|)), F_TOL = 5e-8 on forces and x with
status, iteration count, rho updates and ADMM status equal on every instance.  The comparisons
against the same engine are bit for bit.  No instance is excluded from any comparison.
"""
import ctypes as C

import numpy as np
import pytest

import disturbance_cases as DC
import param_cases as PC
import robot_cases as RC
import weight_cases as WC
from test_gpu_params import F_TOL, FORM_TOL, _assert_equals_oracle, _rel
from test_gpu_slice import _same

pytestmark = pytest.mark.gpu

KW = dict(want_x=True, want_y=True)


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _rows(r, sel):
    return {k: v[sel] for k, v in r.items() if isinstance(v, np.ndarray)}


# ---- 1. against the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("N", DC.HORIZONS)
def test_formulation_vs_oracle_plus_shift(mpcq, oracle, N):
    """mpcq_formulate_batch honours the table: Ax bit-equal to the run without one, l and u against
    oracle.formulate plus the shift, both formulation modes."""
    s, tab = PC.make_batch(N), DC.make_disturbances(N)
    B = tab.shape[0]
    with mpcq.Engine(N) as e:
        for mode in (0, 1):
            plain = e.formulate(s["xref"], s["fsteps"], mode)
            e.set_disturbance(tab)
            r = e.formulate(s["xref"], s["fsteps"], mode)
            e.set_disturbance(None)
            assert (r["status"] == 0).all()
            assert np.array_equal(r["Ax"], plain["Ax"])
            err, moved = 0.0, np.inf
            for b in range(B):
                _, l, u = DC.oracle_formulate(oracle, s["xref"][b], s["fsteps"][b], tab["a"][b], mode=mode)
                err = max(err, _rel(r["l"][b], l), _rel(r["u"][b], u))
                moved = min(moved, float(np.abs(r["l"][b, :12 * N] - plain["l"][b, :12 * N]).max()))  # (the dynamics rows: finite)
            print(f"N={N} mode {mode}: l, u against oracle + shift {err:.2e}; l moves by >= {moved:.2e}")
            assert err <= FORM_TOL, (mode, err)
            assert moved > 1e-3


@pytest.mark.parametrize("N", DC.HORIZONS)
def test_fused_solve_vs_oracle(mpcq, oracle, N):
    """Instance b under table[b] against formulate -> shift -> qp_solve of instance b.
    Observed max |f0 - f0_oracle| (MI355X), integer outcomes equal on every instance:
    N = 12 5.5e-11, 16 1.8e-10, 20 1.3e-11, 33 5.7e-12, 49 9.7e-11, 50 6.7e-12."""
    s, tab = PC.make_batch(N), DC.make_disturbances(N)
    with mpcq.Engine(N) as e:
        e.set_disturbance(tab)
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
    ef = _assert_equals_oracle(r, DC.oracle_solve(oracle, N, tab, key="table"), f"N={N} disturbance")
    print(f"N={N}: worst |f0 - f0_oracle| under the disturbance table {ef:.2e}")


def test_all_three_tables_vs_oracle(mpcq, oracle):
    N = 16
    s, tab, w, rob = PC.make_batch(N), DC.make_disturbances(N), WC.make_weights(N), RC.make_robots(N)
    with mpcq.Engine(N) as e:
        e.set_robots(rob)
        e.set_weights(w)
        e.set_disturbance(tab)
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
    o = DC.oracle_solve(oracle, N, tab, robots=rob, weights=w, key="table+robots+weights")
    _assert_equals_oracle(r, o, "N=16 disturbance + robots + weights")


# ---- 2. zeros and the context's values change no bit -------------------------------------------

@pytest.mark.parametrize("N", [16, 20, 33])
def test_zero_table_changes_no_bit(mpcq, N):
    """A table of +0.0, alone and beside robots and weights tables of the context's values, is the
    launch without tables bit for bit (through the ROB kernels); the recipe's table moves every
    instance; clearing restores."""
    s = PC.make_batch(N)
    B = s["xref"].shape[0]
    ov = PC.CASES["form_all"]  # (the context's values are not the library defaults either)
    with mpcq.Engine(N, **ov) as e:
        ref = e.solve(s["xref"], s["fsteps"], 0, **KW)
        fref = e.formulate(s["xref"], s["fsteps"], 0)
        e.set_disturbance(mpcq.disturbances(B))
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), f"N={N} zeros")
        f1 = e.formulate(s["xref"], s["fsteps"], 0)
        assert all(f1[k].tobytes() == fref[k].tobytes() for k in ("Ax", "l", "u"))  # (the sign of a zero too)
        e.set_robots(mpcq.robots(B, params=e.params))
        e.set_weights(mpcq.weights(B, params=e.params))
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), f"N={N} zeros + context robots + context weights")
        e.set_robots(None)
        e.set_weights(None)
        e.set_disturbance(DC.make_disturbances(N))
        moved = e.solve(s["xref"], s["fsteps"], 0, **KW)
        assert (np.abs(moved["f0"] - ref["f0"]).max(axis=1) > 1e-2).all()
        e.set_disturbance(None)
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), f"N={N} cleared")


# ---- 3. indexing by instance -------------------------------------------------------------------

@pytest.mark.parametrize("N", [16, 33])
def test_instance_in_a_batch_is_itself_alone(mpcq, N):
    """Instance b of the batch == a batch of one holding instance b and row b, bit for bit."""
    s, tab = PC.make_batch(N), DC.make_disturbances(N)
    B = tab.shape[0]
    with mpcq.Engine(N) as e:
        e.set_disturbance(tab)
        got = e.solve(s["xref"], s["fsteps"], 0, **KW)
        for b in (0, 1, B // 2, B - 1):
            e.set_disturbance(tab[b:b + 1])
            one = e.solve(s["xref"][b:b + 1], s["fsteps"][b:b + 1], 0, **KW)
            _same(_rows(one, slice(0, 1)), _rows(got, slice(b, b + 1)), f"N={N} row {b}")


def test_table_is_indexed_by_instance_under_class_order(mpcq):
    N = 16
    s, tab = PC.make_batch(N), DC.make_disturbances(N)
    B = tab.shape[0]
    with mpcq.Engine(N) as e0:
        e0.set_disturbance(tab)
        ref = e0.solve(s["xref"], s["fsteps"], 0, **KW)
    with mpcq.Engine(N) as e:
        e.set_disturbance(tab)
        k = e.class_table_slots()
        cls, order = e.class_order(s["fsteps"])
        assert np.array_equal(order, np.arange(B))
        sm, cn = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        for rank, c in enumerate(dict.fromkeys(cls.tolist())):
            sm[c], cn[c] = 10 * 200 * (rank + 1), 10
        e.set_class_table(sm, cn)
        for launch in range(2):
            got = e.solve(s["xref"], s["fsteps"], 0, order_by_class=True, **KW)
            d = e.last_dispatch()
            assert d["by_class"] and sorted(d["order"].tolist()) == list(range(B))
            assert not np.array_equal(d["order"], np.arange(B)), launch
            _same(ref, got, f"class order, launch {launch}")


def test_sliced_solve_sees_the_same_rows(mpcq):
    N = 20
    s, tab = PC.make_batch(N), DC.make_disturbances(N)
    with mpcq.Engine(N) as e0:
        e0.set_disturbance(tab)
        ref = e0.solve(s["xref"], s["fsteps"], 0, **KW)
    assert ref["iters"].min() > 45  # every instance is suspended; the resumed launch re-formulates
    with mpcq.Engine(N) as e1:
        e1.set_disturbance(tab)
        e1.set_slice(45)
        got = e1.solve(s["xref"], s["fsteps"], 0, **KW)
        d = e1.last_dispatch()
        assert d["sliced"] and d["count"] == tab.shape[0]
        _same(ref, got, "N=20 slice=45 disturbance")


SESSION_OUT = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_COST", "SV_Q_W", "SV_X_ROBOT")


def _session_run(mpcq, N, table, B=6, T=4):
    """T host-fed ticks of a B-robot session (test_gpu_session.py's inputs) under ``table``: every
    tick's outputs and the dispatch order each tick from the second on was launched in."""
    from test_gpu_session import _gaits, _inputs
    gaits = _gaits(B, N)
    rng = np.random.default_rng(3 + N)
    got, orders = [], []
    with mpcq.Engine(N) as eng, mpcq.Session(eng, B, gait0=gaits) as sess:
        sess.set_disturbance(table)
        for k in range(T):
            state, l_feet, v_ref = _inputs(rng, B, k)
            if k:
                orders.append(sess.read(mpcq.SV_ORDER))
            sess.tick(v_ref, state=state, l_feet=l_feet, k=k)
            got.append({w: sess.read(getattr(mpcq, w)) for w in SESSION_OUT})
    return got, orders


def test_session_table_is_indexed_by_robot_under_the_session_order(mpcq, monkeypatch):
    N, B = 16, 6
    tab = DC.make_disturbances(N)[:B]
    ordered, orders = _session_run(mpcq, N, tab)
    for o in orders:
        assert sorted(o.tolist()) == list(range(B))
    assert any(not np.array_equal(o, np.arange(B)) for o in orders), orders
    monkeypatch.setenv("MPCQ_DISPATCH_ORDER", "0")
    indexed, _ = _session_run(mpcq, N, tab)
    for k, (x, y) in enumerate(zip(ordered, indexed)):
        for w in SESSION_OUT:
            assert np.array_equal(x[w], y[w], equal_nan=True), (k, w)


# ---- 4. device pointers, refusals, the QP entry point ------------------------------------------

def _to_device(tab):
    import torch
    t = torch.from_numpy(tab.view(np.float64).reshape(tab.shape[0], 8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def test_device_pointer_table_and_nonfinite_rows(mpcq):
    N = 16
    s, tab = PC.make_batch(N), DC.make_disturbances(N)
    B = tab.shape[0]
    with mpcq.Engine(N) as e:
        e.set_disturbance(tab)
        ref = e.solve(s["xref"], s["fsteps"], 0, **KW)
        e.set_disturbance(None)
        t = _to_device(tab)
        e.set_disturbance_device(t.data_ptr(), B)
        del t  # the engine owns a copy
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), "device table")
        # a NaN or an Inf in a device table (not validated) ends as NONFINITE on that instance only
        for b, j, val in ((5, 2, np.nan), (3, 0, np.inf), (9, 4, -np.inf)):
            bad = tab.copy()
            bad["a"][b, j] = val
            t = _to_device(bad)
            e.set_disturbance_device(t.data_ptr(), B)
            r = e.solve(s["xref"], s["fsteps"], 0, **KW)
            assert r["status"][b] == mpcq.STATUS_NONFINITE and np.isnan(r["f0"][b]).all(), (b, j, val)
            keep = np.arange(B) != b
            _same(_rows(ref, keep), _rows(r, keep), f"the other instances ({val} in row {b})")
        e.set_disturbance_device(0, 0)  # clears
        assert not e.has_disturbance
        plain = e.solve(s["xref"], s["fsteps"], 0, **KW)
        assert (np.abs(plain["f0"] - ref["f0"]).max(axis=1) > 1e-2).all()


def test_validation(mpcq):
    N = 16
    s, tab = PC.make_batch(N), DC.make_disturbances(N)
    B = tab.shape[0]
    with mpcq.Engine(N) as e:
        e.set_disturbance(tab[:B - 1])
        # batch > count: an error before anything is staged or launched; the outputs stay as they were
        f0 = np.full((B, 12), 7.0)
        st = np.full(B, 77, np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        xr, fs = np.ascontiguousarray(s["xref"]), np.ascontiguousarray(s["fsteps"])
        rc = mpcq.lib().mpcq_solve_batch(e._h, B, p(xr), p(fs), 0, None, None, None, p(f0), None, None, None, p(st),
                                         None, None, 0)
        assert rc == mpcq._lib.E_INVALID and b"disturbance table" in mpcq.lib().mpcq_last_error()
        assert (f0 == 7.0).all() and (st == 77).all()
        with pytest.raises(mpcq.MpcqError):
            e.formulate(s["xref"], s["fsteps"], 0)  # the formulation reads the table too
        ref = e.solve(s["xref"][:B - 1], s["fsteps"][:B - 1], 0, **KW)  # a batch within the table is fine
        # host tables: the first offending index and field are named; the table in force stays
        for field, idx, j, val, word in (("a", 3, 0, np.nan, "a[0]"), ("a", 5, 5, np.inf, "a[5]"),
                                         ("a", 2, 3, -np.inf, "a[3]"), ("reserved", 7, 1, 1.0, "reserved")):
            bad = tab.copy()
            bad[field][idx, j] = val
            bad["a"][idx + 2, 1] = np.nan  # (a later offender: not the one reported)
            with pytest.raises(mpcq.MpcqError) as ei:
                e.set_disturbance(bad)
            assert ei.value.code == mpcq._lib.E_INVALID
            assert f"disturbance[{idx}]" in str(ei.value) and word in str(ei.value), str(ei.value)
        _same(ref, e.solve(s["xref"][:B - 1], s["fsteps"][:B - 1], 0, **KW), "after rejected tables")


def test_qp_solve_ignores_the_table(mpcq):
    N = 16
    s, tab = PC.make_batch(N), DC.make_disturbances(N)
    with mpcq.Engine(N) as e:
        f = e.formulate(s["xref"], s["fsteps"], 0)
        ref = e.qp_solve(f["Ax"], f["l"], f["u"])
        for t in (tab, tab[:4]):  # (shorter than the batch too: the entry point does not look at it)
            e.set_disturbance(t)
            _same(ref, e.qp_solve(f["Ax"], f["l"], f["u"]), "qp_solve with a disturbance table set")
        # and the fused solve under the table is the QP entry point on the table's own l and u
        e.set_disturbance(tab)
        ft = e.formulate(s["xref"], s["fsteps"], 0)
        fused = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
        qp = e.qp_solve(ft["Ax"], ft["l"], ft["u"])
        assert np.array_equal(fused["status"], qp["status"]) and np.array_equal(fused["iters"], qp["iters"])
        assert np.abs(fused["x"] - qp["x"]).max() < F_TOL


# ---- 5. session --------------------------------------------------------------------------------

def test_session_with_a_constant_table(mpcq, oracle):
    """N = 16, B = 5, 12 ticks of the virtual robot through a reset of two robots before tick 7:
    every (robot, tick) against formulate -> shift -> qp_solve on the session's own XREF / FSTEPS,
    warm from the session's own previous tick (the oracle's retrieve shifts its x).  The table
    survives the reset; no snapshot carries it."""
    from test_gpu_session import _gaits
    N, B, T = 16, 5, 12
    gaits = _gaits(B, N)
    tab = DC.make_disturbances(N)[:B]
    tab["a"] *= 0.25  # (a payload's or a push's size: the robots keep walking)
    v_ref = np.array([[0.3 + 0.1 * b, 0.05 * (b - 2), 0, 0, 0, 0.1 * (b - 2)] for b in range(B)])
    mask = np.array([0, 1, 0, 1, 0], np.int32)
    names = ("SV_X", "SV_Y", "SV_RHO", "SV_XREF", "SV_FSTEPS", "SV_GAIT", "SV_Q_W", "SV_STATUS", "SV_ITERS", "SV_F0")
    worst = 0.0
    with mpcq.Engine(N) as eng, mpcq.Session(eng, B, gait0=gaits) as sess:
        assert sess.get_disturbance().tobytes() == mpcq.disturbances(B).tobytes()  # without a table: zeros
        sess.set_disturbance(tab)
        prev, qw0 = None, sess.read(mpcq.SV_Q_W)  # (the shifted warm start does not depend on the pose)
        for k in range(T):
            first = np.ones(B, bool) if k == 0 else np.zeros(B, bool)
            if k == 7:
                sess.reset(mask)
                first = mask != 0
            sess.tick(v_ref)
            now = {w: sess.read(getattr(mpcq, w)) for w in names}
            assert (now["SV_STATUS"] == 1).all(), (k, now["SV_STATUS"])
            for b in range(B):
                warm = {}
                if not first[b]:
                    o = oracle.retrieve(N, prev["SV_X"][b], prev["SV_XREF"][b], prev["SV_FSTEPS"][b], prev["SV_GAIT"][b],
                                        qw0[b])
                    warm = dict(warm_x=o["warm_x"], warm_y=prev["SV_Y"][b], rho=float(prev["SV_RHO"][b]))
                r = DC.oracle_solve_one(oracle, now["SV_XREF"][b], now["SV_FSTEPS"][b], tab["a"][b],
                                        mode=1 if first[b] else 0, **warm)
                assert (now["SV_STATUS"][b], now["SV_ITERS"][b]) == (r["status"], r["iters"]), (k, b)
                worst = max(worst, float(np.abs(now["SV_F0"][b] - r["f0"]).max()),
                            float(np.abs(now["SV_X"][b] - r["x"]).max()))
            prev = now
        print(f"session under a constant table: max |f0, x - reference| over {T} ticks {worst:.2e}")
        assert worst < F_TOL, worst
        assert sess.get_disturbance().tobytes() == tab.tobytes()  # (after the reset and 12 ticks)
        # snapshots do not carry the table
        with sess.snapshot() as with_table:
            blob_with = with_table.tobytes()
            sess.set_disturbance(None)
            with sess.snapshot() as without:
                assert without.tobytes() == blob_with
            sess.restore(with_table)
            assert sess.get_disturbance().tobytes() == mpcq.disturbances(B).tobytes()
            sess.set_disturbance(tab)
            sess.restore(with_table, map=np.arange(B)[::-1])
            sess.fork(0)
            assert sess.get_disturbance().tobytes() == tab.tobytes()
