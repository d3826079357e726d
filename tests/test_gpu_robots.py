"""GPU: per-robot mass, inertia, friction and force limit in batch solves and sessions
(mpcq_set_robots, mpcq_session_set_robots) against per-instance oracle solves.

The table and the inputs are tests/robot_cases.py's (test_robots_host.py shows on the oracle that
every instance moves by more than 1e-5 from the default robot's result and from its neighbour's
robot's, so an engine that ignored the table or indexed it by workgroup instead of by instance
cannot pass).  Tolerances are tests/test_gpu_params.py's: F_TOL = 5e-8 on forces and x with
status, iteration count, rho updates and ADMM status equal on every instance; FORM_TOL = 1e-13
relative on the formulation.  No instance is excluded from any comparison.

Worst |f0 - f0_oracle| of the fused comparison per horizon (MI355X): see
test_fused_solve_vs_oracle's docstring.
"""
import ctypes as C

import numpy as np
import pytest

import param_cases as PC
import robot_cases as RC
from test_gpu_params import F_TOL, FORM_TOL, _assert_equals_oracle, _rel
from test_gpu_slice import _same

pytestmark = pytest.mark.gpu

KW = dict(want_x=True, want_y=True)


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


@pytest.mark.parametrize("N", PC.HORIZONS)
def test_fused_solve_vs_oracle(mpcq, oracle, N):
    """Instance b under robots[b] against the oracle's solve of instance b with those Params.
    Observed max |f0 - f0_oracle| (MI355X), integer outcomes equal on every instance:
    N = 12 3.9e-12, 16 2.8e-11, 20 5.0e-11, 33 5.6e-11, 49 7.3e-11, 50 3.3e-10."""
    s, rob = PC.make_batch(N), RC.make_robots(N)
    with mpcq.Engine(N) as e:
        e.set_robots(rob)
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
    ef = _assert_equals_oracle(r, RC.oracle_solve(oracle, N, rob, key="table"), f"N={N} robots")
    print(f"N={N}: worst |f0 - f0_oracle| under the robot table {ef:.2e}")


@pytest.mark.parametrize("N", [16, 33, 50])
def test_formulation_vs_oracle(mpcq, oracle, N):
    s, rob = PC.make_batch(N), RC.make_robots(N)
    with mpcq.Engine(N) as e:
        e.set_robots(rob)
        for mode in (0, 1):
            r = e.formulate(s["xref"], s["fsteps"], mode)
            assert (r["status"] == 0).all()
            err = 0.0
            for b in range(rob.shape[0]):
                Ax, l, u = oracle.formulate(s["xref"][b], s["fsteps"][b], mode, params=RC.oracle_params(oracle, rob[b]))
                err = max(err, _rel(r["Ax"][b], Ax), _rel(r["l"][b], l), _rel(r["u"][b], u))
            print(f"N={N} robots mode {mode}: {err:.2e}")
            assert err <= FORM_TOL, (mode, err)


@pytest.mark.parametrize("N", [16, 20])
def test_table_of_context_values_changes_no_bit(mpcq, N):
    s = PC.make_batch(N)
    B = s["xref"].shape[0]
    ov = PC.CASES["form_all"]  # (the context's values are not the library defaults either)
    with mpcq.Engine(N, **ov) as e:
        ref = e.solve(s["xref"], s["fsteps"], 0, **KW)
        fref = e.formulate(s["xref"], s["fsteps"], 0)
        e.set_robots(mpcq.robots(B, params=e.params))
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), f"N={N} table = context")
        f1 = e.formulate(s["xref"], s["fsteps"], 0)
        assert all(np.array_equal(fref[k], f1[k]) for k in ("Ax", "l", "u"))
        e.set_robots(RC.make_robots(N))
        moved = e.solve(s["xref"], s["fsteps"], 0, **KW)
        assert (np.abs(moved["f0"] - ref["f0"]).max(axis=1) > 1e-5).all()
        e.set_robots(None)
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), f"N={N} cleared")


def test_table_is_indexed_by_instance_under_class_order(mpcq):
    N = 16
    s, rob = PC.make_batch(N), RC.make_robots(N)
    B = rob.shape[0]
    with mpcq.Engine(N) as e0:
        e0.set_robots(rob)
        ref = e0.solve(s["xref"], s["fsteps"], 0, **KW)
    with mpcq.Engine(N) as e:
        e.set_robots(rob)
        k = e.class_table_slots()
        cls, order = e.class_order(s["fsteps"])
        assert np.array_equal(order, np.arange(B))
        # the three classes of the batch, the first instance's the cheapest
        sm, cn = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        for rank, c in enumerate(dict.fromkeys(cls.tolist())):
            sm[c], cn[c] = 10 * 200 * (rank + 1), 10
        assert len(set(cls.tolist())) == 3
        e.set_class_table(sm, cn)
        for launch in range(2):
            got = e.solve(s["xref"], s["fsteps"], 0, order_by_class=True, **KW)
            d = e.last_dispatch()
            assert d["by_class"] and sorted(d["order"].tolist()) == list(range(B))
            assert not np.array_equal(d["order"], np.arange(B)), launch
            _same(ref, got, f"class order, launch {launch}")


def test_sliced_solve_sees_the_same_rows(mpcq):
    N = 20
    s, rob = PC.make_batch(N), RC.make_robots(N)
    with mpcq.Engine(N) as e0:
        e0.set_robots(rob)
        ref = e0.solve(s["xref"], s["fsteps"], 0, **KW)
    assert ref["iters"].min() > 45  # every instance is suspended and re-formulated by the resumed launch
    with mpcq.Engine(N) as e1:
        e1.set_robots(rob)
        e1.set_slice(45)
        got = e1.solve(s["xref"], s["fsteps"], 0, **KW)
        d = e1.last_dispatch()
        assert d["sliced"] and d["count"] == rob.shape[0]
        _same(ref, got, "N=20 slice=45 robots")


def test_general_loop_at_16_stages(mpcq, oracle):
    """polish = 2 at N = 16: the general loop and the polish's bounds (lo_of) under the table."""
    N = 16
    s, rob = PC.make_batch(N), RC.make_robots(N)
    with mpcq.Engine(N, **PC.POLISH2) as e:
        e.set_robots(rob)
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
    _assert_equals_oracle(r, RC.oracle_solve(oracle, N, rob, key="table+polish2", **PC.POLISH2), "N=16 robots polish=2",
                          polish=True)


def test_validation(mpcq):
    N = 16
    s, rob = PC.make_batch(N), RC.make_robots(N)
    B = rob.shape[0]
    with mpcq.Engine(N) as e:
        e.set_robots(rob[:B - 1])
        # batch > count: an error before anything is staged or launched; the outputs stay as they were
        f0 = np.full((B, 12), 7.0)
        st = np.full(B, 77, np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        xr, fs = np.ascontiguousarray(s["xref"]), np.ascontiguousarray(s["fsteps"])
        rc = mpcq.lib().mpcq_solve_batch(e._h, B, p(xr), p(fs), 0, None, None, None, p(f0), None, None, None, p(st),
                                         None, None, 0)
        assert rc == mpcq._lib.E_INVALID and b"robot table" in mpcq.lib().mpcq_last_error()
        assert (f0 == 7.0).all() and (st == 77).all()
        Ax, l, u = np.full((B, 126 * N - 18), 7.0), np.full((B, 44 * N), 7.0), np.full((B, 44 * N), 7.0)
        rc = mpcq.lib().mpcq_formulate_batch(e._h, B, p(xr), p(fs), 0, p(Ax), p(l), p(u), p(st), 0)
        assert rc == mpcq._lib.E_INVALID
        assert (Ax == 7.0).all() and (l == 7.0).all() and (u == 7.0).all() and (st == 77).all()
        with pytest.raises(mpcq.MpcqError) as ei:
            e.solve(s["xref"], s["fsteps"], 0)
        assert ei.value.code == mpcq._lib.E_INVALID
        e.solve(s["xref"][:B - 1], s["fsteps"][:B - 1], 0)  # a batch within the table is fine
        # host tables: the first offending index and field are named; the table in force stays
        ref = e.solve(s["xref"][:B - 1], s["fsteps"][:B - 1], 0, **KW)
        for field, idx, val, word in (("mass", 3, 0.0, "mass"), ("mu", 5, -1.0, "mu"), ("gI", 2, np.nan, "gI"),
                                      ("reserved", 7, 1.0, "reserved"), ("fz_max", 1, np.inf, "fz_max")):
            bad = rob.copy()
            if field == "gI":
                bad["gI"][idx, 1, 2] = val
            elif field == "reserved":
                bad["reserved"][idx, 3] = val
            else:
                bad[field][idx] = val
            bad["mass"][idx + 2] = -1.0  # (a later offender: not the one reported)
            with pytest.raises(mpcq.MpcqError) as ei:
                e.set_robots(bad)
            assert ei.value.code == mpcq._lib.E_INVALID
            assert f"robots[{idx}]" in str(ei.value) and word in str(ei.value), str(ei.value)
        _same(ref, e.solve(s["xref"][:B - 1], s["fsteps"][:B - 1], 0, **KW), "after rejected tables")


def test_device_pointer_table(mpcq):
    """(The first test of the suite to initialise torch on the device pays that once, about ten
    seconds; the test itself is two N = 16 solves.)"""
    import torch
    N = 16
    s, rob = PC.make_batch(N), RC.make_robots(N)
    B = rob.shape[0]
    with mpcq.Engine(N) as e:
        e.set_robots(rob)
        ref = e.solve(s["xref"], s["fsteps"], 0, **KW)
        e.set_robots(None)
        t = torch.from_numpy(rob.view(np.float64).reshape(B, 16).copy()).to("cuda:0")
        torch.cuda.synchronize()
        e.set_robots_device(t.data_ptr(), B)
        del t  # the engine owns a copy
        _same(ref, e.solve(s["xref"], s["fsteps"], 0, **KW), "device table")
        with pytest.raises(mpcq.MpcqError):
            e.solve(np.concatenate([s["xref"], s["xref"]]), np.concatenate([s["fsteps"], s["fsteps"]]), 0)


def test_qp_solve_ignores_the_table(mpcq):
    N = 16
    s, rob = PC.make_batch(N), RC.make_robots(N)
    with mpcq.Engine(N) as e:
        f = e.formulate(s["xref"], s["fsteps"], 0)
        ref = e.qp_solve(f["Ax"], f["l"], f["u"])
        e.set_robots(rob[:4])  # (shorter than the batch too: the qp path does not look at it)
        _same(ref, e.qp_solve(f["Ax"], f["l"], f["u"]), "qp_solve with a table set")


@pytest.mark.parametrize("N", [16, 20])
def test_session_with_per_robot_tables_vs_oracle(mpcq, N):
    """Four host-fed ticks, each robot with its own constants, the table replaced between ticks 1
    and 2 on both sides; tolerances and helpers of test_gpu_session.py."""
    from oracle import oracle as O
    from test_gpu_session import _compare, _gaits, _inputs
    B, T = 6, 4
    gaits = _gaits(B, N)
    tabs = (RC.make_robots(N)[:B], RC.make_robots(N + 1, 8)[2:2 + B])
    rng = np.random.default_rng(11 + N)
    agree, worst = [], 0.0
    with mpcq.Engine(N) as eng, mpcq.Session(eng, B, gait0=gaits) as sess:
        dflt = sess.get_robots()
        assert dflt.tobytes() == mpcq.robots(B, params=eng.params).tobytes()
        ors = [O.Session(N, gaits[b]) for b in range(B)]
        eng.set_robots(tabs[1])  # the context's own table: not the session's business
        for k in range(T):
            if k in (0, 2):
                tab = tabs[k // 2]
                sess.set_robots(tab)
                assert sess.get_robots().tobytes() == tab.tobytes()
                for b, o in enumerate(ors):
                    o.p = RC.oracle_params(O, tab[b])
            state, l_feet, v_ref = _inputs(rng, B, k)
            red = (np.arange(B) % 5 == 0).astype(np.int32)
            sess.tick(v_ref, state=state, l_feet=l_feet, reduced=red, k=k)
            for b, o in enumerate(ors):
                o.tick(k, v_ref[b], state=state[b], l_feet=l_feet[b], reduced=bool(red[b]))
            d, _ = _compare(sess, ors, mpcq, k, agree)
            worst = max(worst, d)
        sess.set_robots(None)
        assert sess.get_robots().tobytes() == dflt.tobytes()
    assert len(agree) == B * T and all(agree)
    print(f"N={N}: max |f0 - f0_oracle| over {T} ticks with per-robot tables = {worst:.2e}")


SESSION_OUT = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_COST", "SV_Q_W", "SV_X_ROBOT")


def _session_run(mpcq, N, table, B=6, T=4):
    """T host-fed ticks of a B-robot session (test_gpu_session.py's inputs) with ``table`` (None:
    set_robots is never called): every tick's outputs, and the dispatch order each tick from the
    second on was launched in (MPCQ_SV_ORDER as it stood before the tick)."""
    from test_gpu_session import _gaits, _inputs
    gaits = _gaits(B, N)
    rng = np.random.default_rng(3 + N)
    got, orders = [], []
    with mpcq.Engine(N) as eng, mpcq.Session(eng, B, gait0=gaits) as sess:
        if table is not None:
            sess.set_robots(table)
        for k in range(T):
            state, l_feet, v_ref = _inputs(rng, B, k)
            if k:
                orders.append(sess.read(mpcq.SV_ORDER))
            sess.tick(v_ref, state=state, l_feet=l_feet, k=k)
            got.append({w: sess.read(getattr(mpcq, w)) for w in SESSION_OUT})
    return got, orders


def _same_ticks(a, b, tag):
    assert len(a) == len(b) == 4
    for k, (x, y) in enumerate(zip(a, b)):
        for w in SESSION_OUT:
            assert np.array_equal(x[w], y[w], equal_nan=True), (tag, k, w)


def _permuted(orders, B=6):
    for o in orders:
        assert sorted(o.tolist()) == list(range(B))
    return [not np.array_equal(o, np.arange(B)) for o in orders]


@pytest.mark.parametrize("N", [16, 20])
def test_session_without_a_table_equals_the_default_table(mpcq, N):
    """B = 6, four host-fed ticks: a session that never calls set_robots against the same session
    given the all-default table, bit for bit -- the plain kernel against the table kernel with warm
    starts, the rho carry-over and the longest-first order in play (the order of at least one of
    the warm ticks is not the identity, and equal in both runs)."""
    plain, o0 = _session_run(mpcq, N, None)
    tabled, o1 = _session_run(mpcq, N, mpcq.robots(6))
    _same_ticks(plain, tabled, f"N={N} default table")
    assert all(np.array_equal(a, b) for a, b in zip(o0, o1))
    print(f"N={N}: dispatch orders of ticks 1..3 {[o.tolist() for o in o0]}")
    assert any(_permuted(o0)), o0


@pytest.mark.parametrize("N", [16, 20])
def test_session_table_is_indexed_by_robot_under_the_session_order(mpcq, N, monkeypatch):
    """The same per-robot table with the longest-first dispatch order (not the identity: asserted
    on MPCQ_SV_ORDER) and in index order (MPCQ_DISPATCH_ORDER=0, read when the session is
    created): bit-identical, so workgroup i reads row order[i], not row i."""
    tab = RC.make_robots(N)[:6]
    ordered, orders = _session_run(mpcq, N, tab)
    assert any(_permuted(orders)), orders
    monkeypatch.setenv("MPCQ_DISPATCH_ORDER", "0")
    indexed, _ = _session_run(mpcq, N, tab)
    _same_ticks(ordered, indexed, f"N={N} session order on / off")
    moved = np.abs(ordered[3]["SV_F0"] - _session_run(mpcq, N, None)[0][3]["SV_F0"]).max(axis=1)
    assert (moved > 1e-5).all(), moved  # (and the table does move every robot of this session)


def test_wrapper_solve_batch_forwards_robots(mpcq):
    N = 16
    s, rob = PC.make_batch(N), RC.make_robots(N)
    with mpcq.Engine(N) as e:
        plain = e.solve(s["xref"], s["fsteps"], 0)
        e.set_robots(rob)
        ref = e.solve(s["xref"], s["fsteps"], 0)
    from mpcq.wrapper import MPC_Wrapper
    w = MPC_Wrapper(0.02, N, 20, 0.32, dual_warm=0)
    try:
        f0, info = w.solve_batch(s["xref"], s["fsteps"], robots=rob)
        assert np.array_equal(f0, ref["f0"]) and np.array_equal(info["iters"], ref["iters"])
        f0, info = w.solve_batch(s["xref"], s["fsteps"])  # the table was for that call only
        assert np.array_equal(f0, plain["f0"]) and np.array_equal(info["iters"], plain["iters"])
        # an engine with a table of its own: used as it is, never silently replaced
        w.mpc.engine.set_robots(rob)
        f0, info = w.solve_batch(s["xref"], s["fsteps"])
        assert np.array_equal(f0, ref["f0"])
        with pytest.raises(ValueError):
            w.solve_batch(s["xref"], s["fsteps"], robots=rob)
        assert np.array_equal(w.solve_batch(s["xref"], s["fsteps"])[0], ref["f0"])
    finally:
        w.close()
        w.mpc.engine.close()
