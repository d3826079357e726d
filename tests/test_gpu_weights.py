"""GPU: per-instance cost weights (the diagonal of P) in batch solves and sessions
(mpcq_set_weights, mpcq_session_set_weights) against per-instance oracle solves and against the
same engine created with each row's weights.

The table and the inputs are tests/weight_cases.py's (test_weights_host.py shows on the oracle that
every instance moves by more than 1e-5 from the default weights' result and from its neighbour's
row's, so an engine that ignored the table or indexed it by workgroup instead of by instance
cannot pass).  Tolerances are tests/test_gpu_params.py's: F_TOL = 5e-8 on forces and x with
status, iteration count, rho updates and ADMM status equal on every instance.  The comparisons
against the same engine are bit for bit.  No instance is excluded from any comparison.
"""
import ctypes as C

import numpy as np
import pytest

import param_cases as PC
import robot_cases as RC
import weight_cases as WC
from test_gpu_params import F_TOL, FORM_TOL, _assert_equals_oracle  # noqa: F401
from test_gpu_slice import _same

pytestmark = pytest.mark.gpu

KW = dict(want_x=True, want_y=True)


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _row_params(row):
    """Engine overrides that make row ``row`` of a table the context's own weights."""
    return dict(state_weights=tuple(float(v) for v in row["state"]), force_weight=float(row["force"]))


# ---- 1. against the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("N", PC.HORIZONS)
def test_fused_solve_vs_oracle(mpcq, oracle, N):
    """Instance b under weights[b] against the oracle's solve of instance b with those Params.
    Observed max |f0 - f0_oracle| (MI355X), integer outcomes equal on every instance:
    N = 12 5.8e-12, 16 1.4e-11, 20 9.5e-11, 33 5.5e-11, 49 5.1e-12, 50 2.5e-9."""
    s, w = PC.make_batch(N), WC.make_weights(N)
    with mpcq.Engine(N) as e:
        e.set_weights(w)
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
    ef = _assert_equals_oracle(r, WC.oracle_solve(oracle, N, w, key="table"), f"N={N} weights")
    print(f"N={N}: worst |f0 - f0_oracle| under the weights table {ef:.2e}")


# ---- 2. against the same engine, bit for bit ---------------------------------------------------

@pytest.mark.parametrize("N,polish", [(16, False), (33, False), (16, True)])
def test_row_equals_an_engine_created_with_it(mpcq, N, polish):
    """Instance b under weights[b] == instance b of an engine whose own parameters are row b's."""
    s, w = PC.make_batch(N), WC.make_weights(N)
    ov = dict(PC.POLISH2) if polish else {}
    with mpcq.Engine(N, **ov) as e:
        e.set_weights(w)
        got = e.solve(s["xref"], s["fsteps"], 0, **KW)
    if polish:
        assert (got["polish"] != 0).any()  # (the polish ran: its KKT diagonal read the row too)
    B = w.shape[0]
    for b in (0, 1, B // 2, B - 1):
        with mpcq.Engine(N, **_row_params(w[b]), **ov) as eb:
            ref = eb.solve(s["xref"], s["fsteps"], 0, **KW)
        _same({k: v[b:b + 1] for k, v in ref.items() if isinstance(v, np.ndarray)},
              {k: v[b:b + 1] for k, v in got.items() if isinstance(v, np.ndarray)}, f"N={N} polish={polish} row {b}")


# ---- 3. a table of the context's own values ----------------------------------------------------

@pytest.mark.parametrize("N", [16, 20])
def test_table_of_context_values_changes_no_bit(mpcq, N):
    s = PC.make_batch(N)
    B = s["xref"].shape[0]
    ov = PC.CASES["form_all"]  # (the context's values are not the library defaults either)
    with mpcq.Engine(N, **ov) as e:
        ref = e.solve(s["xref"], s["fsteps"], 0, **KW)
        e.set_weights(mpcq.weights(B, params=e.params))
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), f"N={N} table = context")
        e.set_weights(WC.make_weights(N))
        moved = e.solve(s["xref"], s["fsteps"], 0, **KW)
        assert (np.abs(moved["f0"] - ref["f0"]).max(axis=1) > 1e-5).all()
        e.set_weights(None)
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), f"N={N} cleared")


# ---- 4. both tables ----------------------------------------------------------------------------

def test_both_tables_vs_oracle(mpcq, oracle):
    N = 16
    s, w, rob = PC.make_batch(N), WC.make_weights(N), RC.make_robots(N)
    with mpcq.Engine(N) as e:
        e.set_robots(rob)
        e.set_weights(w)
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
    _assert_equals_oracle(r, WC.oracle_solve(oracle, N, w, robots=rob, key="table+robots"), "N=16 weights + robots")


# ---- 5. indexing by instance -------------------------------------------------------------------

def test_table_is_indexed_by_instance_under_class_order(mpcq):
    N = 16
    s, w = PC.make_batch(N), WC.make_weights(N)
    B = w.shape[0]
    with mpcq.Engine(N) as e0:
        e0.set_weights(w)
        ref = e0.solve(s["xref"], s["fsteps"], 0, **KW)
    with mpcq.Engine(N) as e:
        e.set_weights(w)
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
    s, w = PC.make_batch(N), WC.make_weights(N)
    with mpcq.Engine(N) as e0:
        e0.set_weights(w)
        ref = e0.solve(s["xref"], s["fsteps"], 0, **KW)
    assert ref["iters"].min() > 45  # every instance is suspended and re-scaled by the resumed launch
    with mpcq.Engine(N) as e1:
        e1.set_weights(w)
        e1.set_slice(45)
        got = e1.solve(s["xref"], s["fsteps"], 0, **KW)
        d = e1.last_dispatch()
        assert d["sliced"] and d["count"] == w.shape[0]
        _same(ref, got, "N=20 slice=45 weights")


SESSION_OUT = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_COST", "SV_Q_W", "SV_X_ROBOT")


def _session_run(mpcq, N, table, B=6, T=4):
    """T host-fed ticks of a B-robot session (test_gpu_session.py's inputs) under ``table``: every
    tick's outputs and the dispatch order each tick from the second on was launched in."""
    from test_gpu_session import _gaits, _inputs
    gaits = _gaits(B, N)
    rng = np.random.default_rng(3 + N)
    got, orders = [], []
    with mpcq.Engine(N) as eng, mpcq.Session(eng, B, gait0=gaits) as sess:
        if table is not None:
            sess.set_weights(table)
        for k in range(T):
            state, l_feet, v_ref = _inputs(rng, B, k)
            if k:
                orders.append(sess.read(mpcq.SV_ORDER))
            sess.tick(v_ref, state=state, l_feet=l_feet, k=k)
            got.append({w: sess.read(getattr(mpcq, w)) for w in SESSION_OUT})
    return got, orders


def test_session_table_is_indexed_by_robot_under_the_session_order(mpcq, monkeypatch):
    N, B = 16, 6
    tab = WC.make_weights(N)[:B]
    ordered, orders = _session_run(mpcq, N, tab)
    for o in orders:
        assert sorted(o.tolist()) == list(range(B))
    assert any(not np.array_equal(o, np.arange(B)) for o in orders), orders
    monkeypatch.setenv("MPCQ_DISPATCH_ORDER", "0")
    indexed, _ = _session_run(mpcq, N, tab)
    for k, (x, y) in enumerate(zip(ordered, indexed)):
        for w in SESSION_OUT:
            assert np.array_equal(x[w], y[w], equal_nan=True), (k, w)


# ---- 6. session --------------------------------------------------------------------------------

SV5 = ("SV_F0", "SV_X_ROBOT", "SV_COST", "SV_STATUS", "SV_ITERS")


def _virtual_run(mpcq, eng, gaits, v_ref, T, table=None, reset_at=None, reset_mask=None):
    B = gaits.shape[0]
    out = []
    with mpcq.Session(eng, B, gait0=gaits) as sess:
        dflt = sess.get_weights()
        if table is not None:
            sess.set_weights(table)
        for k in range(T):
            if reset_at is not None and k == reset_at:
                sess.reset(reset_mask)
            sess.tick(v_ref)
            out.append({w: sess.read(getattr(mpcq, w)) for w in SV5})
        now = sess.get_weights()
    return out, dflt, now


def test_session_with_a_weights_table(mpcq):
    """N = 16, B = 5, 12 ticks of the virtual robot from create: the session under the table against
    five one-robot sessions, each on an engine created with its row's weights, bit for bit; a
    mid-run reset of two robots keeps the table."""
    from test_gpu_session import _gaits
    N, B, T = 16, 5, 12
    gaits = _gaits(B, N)
    tab = WC.make_weights(N)[:B]
    v_ref = np.array([[0.3 + 0.1 * b, 0.05 * (b - 2), 0, 0, 0, 0.1 * (b - 2)] for b in range(B)])
    mask = np.array([0, 1, 0, 1, 0], np.int32)
    with mpcq.Engine(N) as eng:
        got, dflt, now = _virtual_run(mpcq, eng, gaits, v_ref, T, tab, reset_at=7, reset_mask=mask)
        plain, _, still = _virtual_run(mpcq, eng, gaits, v_ref, T, None, reset_at=7, reset_mask=mask)
        assert dflt.tobytes() == mpcq.weights(B, params=eng.params).tobytes()  # without a table: the context's
        assert still.tobytes() == dflt.tobytes()
        assert now.tobytes() == tab.tobytes()  # (after the reset and 12 ticks)
    for b in range(B):
        with mpcq.Engine(N, **_row_params(tab[b])) as eb:
            one, _, _ = _virtual_run(mpcq, eb, gaits[b:b + 1], v_ref[b:b + 1], T, None,
                                     reset_at=7 if mask[b] else None, reset_mask=None)
        for k in range(T):
            for w in SV5:
                assert np.array_equal(got[k][w][b], one[k][w][0], equal_nan=True), (b, k, w)
    for k in range(T):
        differs = np.abs(got[k]["SV_COST"] - plain[k]["SV_COST"]).max(axis=1) > 0
        assert differs.all(), (k, differs)


# ---- 7. fork for a sweep -----------------------------------------------------------------------

def test_fork_then_set_weights_is_a_sweep(mpcq):
    from test_gpu_session import _gaits
    N, B = 16, 6
    gaits = _gaits(B, N)
    tab = WC.make_weights(N)[:B]
    v_ref = np.array([[0.3 + 0.1 * b, 0.0, 0, 0, 0, 0.05 * b] for b in range(B)])
    with mpcq.Engine(N) as eng, mpcq.Session(eng, B, gait0=gaits) as sess:
        for _ in range(6):
            sess.tick(v_ref)
        sess.fork(2)
        st = sess.read(mpcq.SV_STATE)
        assert (st == st[2]).all()  # one state in every slot
        sess.set_weights(tab)
        f0 = sess.tick(np.broadcast_to(v_ref[2], (B, 6)))
        for i in range(B):
            for j in range(i + 1, B):
                assert np.abs(f0[i] - f0[j]).max() > 1e-5, (i, j)
        # snapshots do not carry the table
        with sess.snapshot() as with_table:
            blob_with = with_table.tobytes()
            sess.set_weights(None)
            with sess.snapshot() as without:
                assert without.tobytes() == blob_with
            sess.restore(with_table)
            assert sess.get_weights().tobytes() == mpcq.weights(B, params=eng.params).tobytes()
            sess.set_weights(tab)
            sess.restore(with_table, map=np.arange(B)[::-1])
            sess.fork(0)
            assert sess.get_weights().tobytes() == tab.tobytes()


# ---- 8. device pointers, refusals, the formulation ---------------------------------------------

def test_device_pointer_table(mpcq):
    import torch
    N = 16
    s, w = PC.make_batch(N), WC.make_weights(N)
    B = w.shape[0]
    with mpcq.Engine(N) as e:
        e.set_weights(w)
        ref = e.solve(s["xref"], s["fsteps"], 0, **KW)
        e.set_weights(None)
        t = torch.from_numpy(w.view(np.float64).reshape(B, 16).copy()).to("cuda:0")
        torch.cuda.synchronize()
        e.set_weights_device(t.data_ptr(), B)
        del t  # the engine owns a copy
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), "device table")
        # a NaN in a device table (not validated) ends as NONFINITE on that instance only
        bad = w.copy()
        bad["state"][5, 2] = np.nan
        t = torch.from_numpy(bad.view(np.float64).reshape(B, 16).copy()).to("cuda:0")
        torch.cuda.synchronize()
        e.set_weights_device(t.data_ptr(), B)
        r = e.solve(s["xref"], s["fsteps"], 0, **KW)
        assert r["status"][5] == mpcq.STATUS_NONFINITE and np.isnan(r["f0"][5]).all()
        keep = np.arange(B) != 5
        _same({k: v[keep] for k, v in ref.items() if isinstance(v, np.ndarray)},
              {k: v[keep] for k, v in r.items() if isinstance(v, np.ndarray)}, "the other instances")
        with pytest.raises(mpcq.MpcqError):
            e.solve(np.concatenate([s["xref"], s["xref"]]), np.concatenate([s["fsteps"], s["fsteps"]]), 0)


def test_validation(mpcq):
    N = 16
    s, w = PC.make_batch(N), WC.make_weights(N)
    B = w.shape[0]
    with mpcq.Engine(N) as e:
        e.set_weights(w[:B - 1])
        # batch > count: an error before anything is staged or launched; the outputs stay as they were
        f0 = np.full((B, 12), 7.0)
        st = np.full(B, 77, np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        xr, fs = np.ascontiguousarray(s["xref"]), np.ascontiguousarray(s["fsteps"])
        rc = mpcq.lib().mpcq_solve_batch(e._h, B, p(xr), p(fs), 0, None, None, None, p(f0), None, None, None, p(st),
                                         None, None, 0)
        assert rc == mpcq._lib.E_INVALID and b"weights table" in mpcq.lib().mpcq_last_error()
        assert (f0 == 7.0).all() and (st == 77).all()
        with pytest.raises(mpcq.MpcqError) as ei:
            e.solve(s["xref"], s["fsteps"], 0)
        assert ei.value.code == mpcq._lib.E_INVALID
        ref = e.solve(s["xref"][:B - 1], s["fsteps"][:B - 1], 0, **KW)  # a batch within the table is fine
        # host tables: the first offending index and field are named; the table in force stays
        for field, idx, j, val, word in (("state", 3, 0, 0.0, "state[0]"), ("state", 5, 11, -1.0, "state[11]"),
                                         ("state", 2, 7, np.nan, "state[7]"), ("force", 6, None, np.inf, "force"),
                                         ("force", 0, None, 0.0, "force"), ("reserved", 7, 2, 1.0, "reserved")):
            bad = w.copy()
            if j is None:
                bad[field][idx] = val
            else:
                bad[field][idx, j] = val
            bad["force"][idx + 2] = -1.0  # (a later offender: not the one reported)
            with pytest.raises(mpcq.MpcqError) as ei:
                e.set_weights(bad)
            assert ei.value.code == mpcq._lib.E_INVALID
            assert f"weights[{idx}]" in str(ei.value) and word in str(ei.value), str(ei.value)
        _same(ref, e.solve(s["xref"][:B - 1], s["fsteps"][:B - 1], 0, **KW), "after rejected tables")


def test_formulation_and_qp_solve_ignore_the_table(mpcq):
    N = 16
    s, w = PC.make_batch(N), WC.make_weights(N)
    with mpcq.Engine(N) as e:
        f = e.formulate(s["xref"], s["fsteps"], 0)
        ref = e.qp_solve(f["Ax"], f["l"], f["u"])
        for tab in (w, w[:4]):  # (shorter than the batch too: neither entry point looks at it)
            e.set_weights(tab)
            f1 = e.formulate(s["xref"], s["fsteps"], 0)
            assert all(np.array_equal(f[k], f1[k]) for k in ("Ax", "l", "u"))
            _same(ref, e.qp_solve(f["Ax"], f["l"], f["u"]), "qp_solve with a weights table set")
