"""GPU: infeasible and inaccurate exits of every engine layout, against the oracle.

The rest of the GPU suite solves feasible problems under eps_prim_inf = eps_dual_inf = 1e-4, where
the infeasibility arithmetic of a termination check (the projected dy and the ineq sum with its
phantom-row guard, the DPP / permlane butterflies, the cross-wave slots, infeas_products and the
inf_need / inf_bits carry) is computed and never decides anything.  Every case of
tests/infeas_cases.py makes it decide, at one horizon per layout (7, 12, 16: exit status through
LDS, 16 in the explicit-inverse loop; 17, 20, 32, 33: re-derived after the loop, 33 in the global
workspace; 49, 50: beyond 48 stages); tests/test_oracle_infeas.py shows on the CPU that each
(case, N) has its power and that no instance flips when the tolerances move by 1e-3 relative, six
decades above the GPU's difference from the oracle.

1. every (case, N) against the oracle: status, iteration count, rho updates and ADMM status equal
   on every instance; x, y (and f0) all-NaN where the oracle ends -3, -4, 3 or 4 (osqp
   store_solution); elsewhere x within X_TOL = 1e-9 (QP entry point, test_gpu_parity.py) or
   F_TOL = 5e-8 (fused, test_gpu_horizons.py) and y within Y_RTOL = 1e-6 relative
   (test_dual_warm_vs_oracle); rho_out within RHO_RTOL; a second launch bit-identical;
2. the feasible neighbours of the hand-made instances: bit-identical to a launch without them;
3. the general loop at N = 16 (polish = 2): an infeasible exit is not polished;
4. sliced solves suspended before a detection and ending exactly on one, and the class order;
5. a per-robot table (fz_max() and mu enter chk_bounds' rebuilt bounds);
6. a NaN in xref through the fused path at N = 12, 20, 33, 50;
7. sessions under a loose eps_prim_inf: robots that fail restart cold and solve on a later tick.

Observed (MI355X), integer outcomes equal to the oracle's on every instance of every pair:
Largest differences from the oracle as max |x - x_oracle| / y relative / rho_out relative, with the
statuses reached and the iterations of the exits without a solution:
  hand_first, hand_mid, hand_last   2.1e-11 / 3.5e-11 / 1.4e-7   -3 at 125..425, neighbours 1
  epi_tight (1e-7)                  2.1e-11 / 3.5e-11 / 1.4e-7   -3 at 325..625
  epi_loose (1e-2)                  2.1e-11 / 3.5e-11 / 1.4e-7   -3 at 50..75
  pinf_inacc_checked / _unchecked   5.4e-11 / 6.8e-13 / 1.5e-10  3 at max_iter (90..160), neighbours -2
  solved_inacc                      1.7e-10 / 3.9e-11 / 2.2e-8   2 and -2 (1 where converged earlier)
  dinf                              2.1e-11 / 3.5e-11 / 1.2e-8   -4 at 200..350 next to 1 and 2
  dinf_first, dinf_inacc            no solution to compare, rho unchanged: -4 at 25, 4 at 60
  fused_epi                         2.6e-10 / 1.6e-12 / 2.2e-8   -3 at 50..825 next to 1
  fused_edi                         2.3e-10 / 9.3e-12 / 5.0e-7   -4 at 25..575 next to 1
  polish = 2, N = 16                1.6e-10 / (polished) / 5.4e-9
  robot table, N = 16 / 33          3.1e-8 / 3.6e-11 / 8.8e-7 at N = 16, 3.2e-11 / 9.2e-15 / 3.2e-10 at 33
  sessions, N = 16 / 20             forces of the solved within 7.2e-12 / 4.5e-11; every (robot, tick)
                                    equal in status and iterations; per tick
                                    2, 4, 6, 0, 6 of 6 robots end -3 at N = 16 and 4, 5, 6, 5, 6 at 20
Sliced (10 iterations, the first and the last detection) and class-ordered solves, the neighbours
of the hand-made rows and of the NaN instance, and the two dispatch orders of a session: bit-equal.
rho_out is rho sqrt(pri / dua) of residual norms that are themselves differences of nearly equal
terms, so it carries the iterate's ~1e-12 difference amplified by 1 / residual: up to 8.8e-7 here
(the robot table at N = 16, whose x difference is that rho's transient); RHO_RTOL = 9e-6 is one
decade above.  The rho update *decisions* (rho_updates) are equal everywhere.
"""
import numpy as np
import pytest

import infeas_cases as IC
import param_cases as PC
from test_gpu_slice import _same

pytestmark = pytest.mark.gpu

X_TOL = 1e-9      # tests/test_gpu_parity.py (QP entry point)
F_TOL = 5e-8      # tests/test_gpu_horizons.py, test_gpu_params.py (fused batches)
Y_RTOL = 1e-6     # tests/test_gpu_parity.py::test_dual_warm_vs_oracle
POLISH_TOL = 1e-8  # tests/test_gpu_parity.py (polished solutions)
RHO_RTOL = 9e-6   # one decade above the largest observed against the oracle, 8.9e-7 (docstring)

KW = dict(want_x=True, want_y=True)
WORST = {}        # case -> [x, y, rho] largest differences seen in this run
_ORACLE = {}      # (case, N, variant) -> the oracle's result, computed once and never modified


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _oracle(oracle, N, name, variant="", **kw):
    key = (name, N, variant)
    if key not in _ORACLE:
        _ORACLE[key] = IC.oracle_solve(oracle, N, name, **kw)
    return _ORACLE[key]


def _launch(e, oracle, N, name, sel=None, order_by_class=False):
    """One launch of the case's batch (or of its instances sel) through the case's entry point."""
    sel = slice(None) if sel is None else sel
    if IC.CASES[name]["entry"] == "qp":
        Ax, l, u, _, _ = IC.make_qp(oracle, N, name, params=oracle.default_params())
        return e.qp_solve(Ax[sel], l[sel], u[sel])
    s = IC.make_batch(N, name)
    return e.solve(s["xref"][sel], s["fsteps"][sel], 0, order_by_class=order_by_class, **KW)


def _vs_oracle(r, o, name, tag, x_tol=None, polish=False):
    """Every instance against the oracle (module docstring, 1).  Returns (x, y, rho) differences.
    polish: also the polish outcome; the duals of a polished instance are not compared (the engine
    polishes by the method of multipliers, the oracle by OSQP's refined KKT solve: the two agree on
    x, which is what the project bounds, and differ by ~4e-3 relative in y on weakly active rows)."""
    fused = IC.CASES[name]["entry"] == "fused"
    x_tol = x_tol or (F_TOL if fused else X_TOL)
    for k in ("status", "iters", "rho_updates", "admm_status") + (("polish",) if polish else ()):
        assert np.array_equal(r[k], o[k]), (tag, k, r[k].tolist(), o[k].tolist())
    nan = np.isin(o["status"], IC.NAN_STATUSES)
    for k in ("x", "y") + (("f0",) if fused else ()):
        assert np.isnan(r[k][nan]).all(), (tag, k)
        assert np.isfinite(r[k][~nan]).all(), (tag, k)
    ex = ey = 0.0
    for b in np.flatnonzero(~nan):
        ex = max(ex, float(np.abs(r["x"][b] - o["x"][b]).max()))
        if not (polish and o["polish"][b] != 0):
            ey = max(ey, float(np.abs(r["y"][b] - o["y"][b]).max() / max(1.0, np.abs(o["y"][b]).max())))
        if fused:
            ex = max(ex, float(np.abs(r["f0"][b] - o["f0"][b]).max()))
    er = float((np.abs(r["rho"] - o["rho"]) / o["rho"]).max())
    det = o["iters"][nan]
    print(f"{tag}: statuses {o['status'].tolist()}, iters {o['iters'].tolist()}; max|x - x_oracle| {ex:.2e}, "
          f"y relative {ey:.2e}, rho relative {er:.2e}" + (f"; exits without a solution at {det.min()}..{det.max()}"
                                                           if det.size else ""))
    assert ex < x_tol, (tag, ex)
    assert ey < Y_RTOL, (tag, ey)
    assert er < RHO_RTOL, (tag, er)
    return ex, ey, er


@pytest.mark.parametrize("name,N", IC.PAIRS)
def test_case_vs_oracle(mpcq, oracle, name, N):
    o = _oracle(oracle, N, name)
    with mpcq.Engine(N, **IC.CASES[name]["params"][N]) as e:
        r = _launch(e, oracle, N, name)
        again = _launch(e, oracle, N, name)
    d = _vs_oracle(r, o, name, f"{name} N={N}")
    _same(r, again, f"{name} N={N} second launch")
    WORST[name] = [max(a, b) for a, b in zip(WORST.get(name, (0.0, 0.0, 0.0)), d)]
    print(f"{name}: largest x / y / rho differences over the horizons so far "
          + " / ".join(f"{v:.2e}" for v in WORST[name]))


@pytest.mark.parametrize("name", ["hand_first", "hand_mid", "hand_last"])
@pytest.mark.parametrize("N", IC.HORIZONS)
def test_neighbours_unaffected(mpcq, oracle, N, name):
    """The feasible instances next to the hand-made ones: bit for bit what a launch of them alone gives."""
    feas = np.flatnonzero(~IC.hand_mask())
    with mpcq.Engine(N) as e:
        r = _launch(e, oracle, N, name)
    with mpcq.Engine(N) as e:
        alone = _launch(e, oracle, N, name, sel=feas)
    assert (alone["status"] == mpcq.STATUS_SOLVED).all() and (np.delete(r["status"], feas) == IC.PINF).all()
    _same(alone, {k: (v[feas] if v is not None else None) for k, v in r.items()}, f"{name} N={N} neighbours")


@pytest.mark.parametrize("name", ["hand_mid", "fused_epi"])
def test_general_loop_at_16_stages(mpcq, oracle, name):
    """polish = 2 at N = 16 iterates in the general loop, not the explicit-inverse one.  An
    infeasible exit reports polish == 0 and admm_status == status; the others are polished as the
    oracle's are (x within POLISH_TOL on the QP entry point, test_gpu_parity.py's bound for
    polished solutions; F_TOL fused, as test_gpu_params.py)."""
    N = 16
    o = _oracle(oracle, N, name, "polish2", extra=PC.POLISH2)
    with mpcq.Engine(N, **dict(IC.CASES[name]["params"][N], **PC.POLISH2)) as e:
        r = _launch(e, oracle, N, name)
    _vs_oracle(r, o, name, f"{name} N={N} polish=2", x_tol=None if name == "fused_epi" else POLISH_TOL, polish=True)
    nan = np.isin(o["status"], IC.NAN_STATUSES)
    assert nan.any() and (~nan).any()
    assert (r["polish"][nan] == 0).all() and (r["polish_rounds"][nan] == 0).all(), r["polish"].tolist()
    assert np.array_equal(r["admm_status"][nan], r["status"][nan])
    assert (r["polish"][~nan] != 0).any()


@pytest.mark.parametrize("name", ["hand_last", "fused_epi"])
@pytest.mark.parametrize("N", [20, 33, 50])
def test_sliced_solves(mpcq, oracle, N, name):
    """Slices of 10 iterations (every instance suspended before any detection) and of exactly the
    first and the last detection iteration (an instance ends -3 on the slice's last check): bit
    for bit the unsliced solve, which equals the oracle.  fused_epi also in class order."""
    o = _oracle(oracle, N, name)
    det = o["iters"][np.isin(o["status"], IC.NAN_STATUSES)]
    assert det.size and det.min() > 10
    ov = IC.CASES[name]["params"][N]
    with mpcq.Engine(N, **ov) as e0:
        ref = _launch(e0, oracle, N, name)
    _vs_oracle(ref, o, name, f"{name} N={N} unsliced")
    for q in sorted({10, int(det.min()), int(det.max())}):
        with mpcq.Engine(N, **ov) as e1:
            e1.set_slice(q)
            got = _launch(e1, oracle, N, name)
            d = e1.last_dispatch()
            assert d["sliced"] and d["count"] == (IC.B if q == 10 else int((o["iters"] > q).sum())), (q, d["count"])
            _same(ref, got, f"{name} N={N} slice={q}")
    if name == "fused_epi":
        with mpcq.Engine(N, **ov) as e2:
            e2.set_slice(int(det.min()))
            for launch in range(2):   # (the class table learns on the first)
                _same(ref, _launch(e2, oracle, N, name, order_by_class=True), f"{name} N={N} class order {launch}")


@pytest.mark.parametrize("N", [16, 33])
def test_robot_table(mpcq, oracle, N):
    """fused_epi with per-instance fz_max and mu (and mass, inertia): the fused path's rebuilt
    bounds take the row's values.  Against the oracle run per instance with that robot's Params."""
    import robot_cases as RC
    rob = RC.make_robots(N, IC.B)
    o = _oracle(oracle, N, "fused_epi", "robots", robots=rob)
    assert (o["status"] == IC.PINF).sum() >= 2 and (o["status"] == IC.SOLVED).any()
    with mpcq.Engine(N, **IC.CASES["fused_epi"]["params"][N]) as e:
        e.set_robots(rob)
        r = _launch(e, oracle, N, "fused_epi")
    _vs_oracle(r, o, "fused_epi", f"fused_epi N={N} robots")


@pytest.mark.parametrize("N", [12, 20, 33, 50])
def test_nonfinite_input_through_the_fused_path(mpcq, oracle, N):
    """One instance with a NaN in xref: MPCQ_STATUS_NONFINITE as in the oracle, no solution; the
    other instances bit for bit as in a launch without the NaN."""
    s = IC.make_batch(N, "fused_epi")
    bad = 3
    xref = s["xref"].copy()
    xref[bad, 2, N // 2] = np.nan
    o = oracle.solve_batch(xref, s["fsteps"], 0, nthreads=8, want_x=True)
    assert o["status"][bad] == mpcq.STATUS_NONFINITE and np.isin(np.delete(o["status"], bad), (1, 2)).all()
    with mpcq.Engine(N) as e:
        clean = e.solve(s["xref"], s["fsteps"], 0, **KW)
        r = e.solve(xref, s["fsteps"], 0, **KW)
    assert np.array_equal(r["status"], o["status"]), r["status"].tolist()
    assert r["admm_status"][bad] == mpcq.STATUS_NONFINITE
    assert np.isnan(r["x"][bad]).all() and np.isnan(r["f0"][bad]).all()
    keep = np.arange(IC.B) != bad
    _same({k: (v[keep] if v is not None else None) for k, v in clean.items()},
          {k: (v[keep] if v is not None else None) for k, v in r.items()}, f"N={N} neighbours of the NaN")
    assert np.abs(r["f0"][keep] - o["f0"][keep]).max() < F_TOL


SESSION_NAMES = ("SV_F0", "SV_X", "SV_Y", "SV_STATUS", "SV_ITERS", "SV_RHO", "SV_STATE", "SV_Q_W", "SV_COST",
                 "SV_X_ROBOT")


@pytest.mark.parametrize("N", sorted(IC.SESSION_EPI))
def test_session_fails_and_recovers(mpcq, oracle, monkeypatch, N):
    """Six robots, five host-fed ticks under a loose eps_prim_inf, against oracle.Session tick by
    tick (test_gpu_session.py's rules and SOLVE_TOL).  A robot whose solve ends -3 keeps its pose,
    and restarts cold (rho back at params.rho, y zero); it solves on a later tick.  With and
    without the longest-first dispatch order: identical."""
    from test_gpu_session import _compare
    B = IC.SESSION_B
    gaits = IC.session_gaits(N)
    runs, worst = {}, 0.0
    for flag in ("1", "0"):
        monkeypatch.setenv("MPCQ_DISPATCH_ORDER", flag)
        ors = IC.oracle_sessions(oracle, N)
        agree, out, st_all = [], [], []
        with mpcq.Engine(N, eps_prim_inf=IC.SESSION_EPI[N]) as eng, mpcq.Session(eng, B, gait0=gaits) as sess:
            for k, state, l_feet, v_ref, red in IC.session_inputs(N):
                q_prev = sess.read(mpcq.SV_Q_W)
                sess.tick(v_ref, state=state, l_feet=l_feet, reduced=red, k=k)
                for b, o in enumerate(ors):
                    o.tick(k, v_ref[b], state=state[b], l_feet=l_feet[b], reduced=bool(red[b]))
                _compare(sess, ors, mpcq, k, agree)
                st = np.array([o.status for o in ors])
                failed = np.isin(st, IC.NAN_STATUSES)
                if (~failed).any():
                    f0 = sess.read(mpcq.SV_F0)
                    worst = max(worst, max(float(np.abs(f0[b] - ors[b].f0).max()) for b in np.flatnonzero(~failed)))
                qw, rho, y = sess.read(mpcq.SV_Q_W), sess.read(mpcq.SV_RHO), sess.read(mpcq.SV_Y)
                assert np.array_equal(qw[failed], q_prev[failed]), k
                assert (rho[failed] == eng.params.rho).all() and not y[failed].any(), k
                assert np.isnan(sess.read(mpcq.SV_F0)[failed]).all(), k
                if (~failed).any():
                    assert (np.abs(qw[~failed] - q_prev[~failed]).max(axis=1) > 0).all(), k
                st_all.append(st)
                out.append({n: sess.read(getattr(mpcq, n)).copy() for n in SESSION_NAMES})
        assert len(agree) == B * IC.SESSION_T and all(agree)
        IC.expect_session(np.array(st_all))
        runs[flag] = out
    print(f"session N={N}: statuses per tick {np.array(st_all).tolist()}, max |f0 - f0_oracle| of the solved {worst:.2e}")
    for k in range(IC.SESSION_T):
        for n in SESSION_NAMES:
            assert np.array_equal(runs["0"][k][n], runs["1"][k][n], equal_nan=True), (k, n)
