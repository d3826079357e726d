"""GPU: every field of mpcq_params away from its default, against the oracle.

The rest of the GPU suite runs mpcq_default_params() with only polish*, max_iter, dual_warm and
device changed, so an engine that hard-coded mu, scaling or the check interval, ignored sigma, or
miscounted to_check / to_adapt when the two intervals are not multiples of each other would pass
it.  Here each case of tests/param_cases.py (19 loop-control / solver settings, 9 formulation
constants; each shown to move the oracle's result by test_oracle_params.py) runs at one horizon
per engine layout (12, 16, 20, 33, 49, 50) on a small mixed-gait batch:

* fused solve vs oracle: status, iteration count, rho updates and ADMM status equal on every
  instance, forces and x within F_TOL = 5e-8 (test_gpu_horizons.py's fused-batch tolerance: 45x
  above the 1.1e-9 the oracle's own two CPU builds differ by on these cases, 200x below the
  smallest effect of any case, 1e-5);
* the general (not explicit-inverse) loop at N = 16, reached through the polish = 2 instantiation;
* forces on the KKT-certified optimum under non-default constants (oracle/certify.py, which does
  not pass through the oracle's ADMM);
* the formulation kernel against the reference-generated golden_params.npz and the oracle;
* the QP entry point (bounds from lo_of / hi_of instead of the fused path's rebuilt ones);
* slicing with counters that are not aligned (bit-identical to the unsliced solve);
* a closed-loop session with non-default engine and planner parameters.

Observed max |f0 - f0_oracle| over the 28 fused cases, per horizon (MI355X), iteration counts,
rho updates and statuses equal on every instance of every case: N = 12 4.6e-11, 16 1.3e-10,
20 1.7e-9, 33 1.2e-10, 49 2.4e-9, 50 6.6e-10.  No horizon's seed had to be changed: no instance
sat on a rounding knife-edge.  The other comparisons: formulation 4.4e-16 relative at most,
polished forces 7.3e-11 from the certified optimum, qp_solve x 1.1e-9 and y 9.8e-11 relative,
sessions 4.8e-10 over the four ticks.
"""
import numpy as np
import pytest

import param_cases as PC

pytestmark = pytest.mark.gpu

F_TOL = 5e-8        # tests/test_gpu_horizons.py
FORM_TOL = 1e-13    # tests/test_gpu_horizons.py
POLISH_TOL = 1e-8   # tests/test_gpu_parity.py
Y_RTOL = 1e-6       # tests/test_gpu_parity.py::test_dual_warm_vs_oracle

WORST = {}          # horizon -> largest |f0 - f0_oracle| seen by the fused comparison in this run
_ORACLE = {}        # (N, case key) -> the oracle's result, computed once and never modified


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _oracle_batch(oracle, N, key, ov):
    if (N, key) not in _ORACLE:
        s = PC.make_batch(N)
        o = oracle.solve_batch(s["xref"], s["fsteps"], 0, params=oracle.default_params(**ov), nthreads=16,
                               want_x=True)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        _ORACLE[(N, key)] = o
    return _ORACLE[(N, key)]


def _assert_equals_oracle(r, o, tag, polish=False):
    """Every instance: the integer outcomes equal, forces and x within F_TOL.  Returns max |f0 - f0_oracle|."""
    B = o["status"].shape[0]
    assert r["status"].shape == (B,)
    for k in ("status", "iters", "rho_updates", "admm_status") + (("polish",) if polish else ()):
        assert np.array_equal(r[k], o[k]), (tag, k, r[k].tolist(), o[k].tolist())
    ef = float(np.abs(r["f0"] - o["f0"]).max())
    ex = float(np.abs(r["x"] - o["x"]).max())
    print(f"{tag}: max|f0 - f0_oracle| {ef:.2e}, max|x - x_oracle| {ex:.2e}, iters {o['iters'].min()}..{o['iters'].max()}, "
          f"rho updates up to {o['rho_updates'].max()}, statuses {np.unique(o['status']).tolist()}")
    assert ef < F_TOL, (tag, ef)
    assert ex < F_TOL, (tag, ex)
    return ef


@pytest.mark.parametrize("case", list(PC.CASES))
@pytest.mark.parametrize("N", PC.HORIZONS)
def test_fused_solve_vs_oracle(mpcq, oracle, N, case):
    ov = PC.CASES[case]
    s = PC.make_batch(N)
    with mpcq.Engine(N, **ov) as e:
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
    ef = _assert_equals_oracle(r, _oracle_batch(oracle, N, case, ov), f"N={N} {case}")
    WORST[N] = max(WORST.get(N, 0.0), ef)
    print(f"N={N}: max|f0 - f0_oracle| over the cases so far {WORST[N]:.2e}")


@pytest.mark.parametrize("case", ["chk7_adp30", "chk30_adp20", "mi137"])
def test_general_loop_at_16_stages(mpcq, oracle, case):
    """The polish = 2 instantiation at N = 16 iterates in the general loop, not the
    explicit-inverse one: the same counters, another code path."""
    N = 16
    ov = dict(PC.CASES[case], **PC.POLISH2)
    s = PC.make_batch(N)
    with mpcq.Engine(N, **ov) as e:
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True)
    _assert_equals_oracle(r, _oracle_batch(oracle, N, case + "+polish2", ov), f"N={N} {case} polish=2", polish=True)


@pytest.mark.parametrize("N", [16, 20, 50])
def test_forces_on_certified_optimum_under_form_all(mpcq, oracle, N):
    """form_all with polish = 2: forces within POLISH_TOL of each QP's KKT-certified optimum, which
    certify.py computes from the parameters by active-set steps on the unscaled KKT system -- the
    oracle's ADMM is not involved (the oracle itself lands within 2e-14)."""
    from oracle import certify
    ov = dict(PC.CASES["form_all"], **PC.POLISH2)
    s = PC.make_batch(N)
    with mpcq.Engine(N, **ov) as e:
        r = e.solve(s["xref"], s["fsteps"], 0, want_x=True, want_y=True)
    assert (r["status"] == mpcq.STATUS_SOLVED).all(), r["status"]
    assert (r["polish"] == 1).all(), r["polish"]
    fstar, kkt, ok = certify.certified_forces(s["xref"], s["fsteps"], r["x"], r["y"], params=oracle.default_params(**ov))
    assert ok.all(), kkt
    d = float(np.abs(r["f0"] - fstar).max())
    print(f"N={N} form_all polish=2: max|f0 - f0*| {d:.2e}, KKT residual max {kkt.max():.1e}")
    assert d < POLISH_TOL


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.array_equal(np.isinf(a), np.isinf(b))
    fa, fb = np.where(np.isinf(a), 0, a), np.where(np.isinf(b), 0, b)
    return float((np.abs(fa - fb) / np.maximum(1.0, np.abs(fb))).max(initial=0))


@pytest.mark.parametrize("entry", range(9))
def test_formulation_vs_reference_under_params(mpcq, entry):
    """The formulation kernel against what the unmodified reference hands to OSQP under
    non-default mass / mu / gI / dt / default footholds (golden_params.npz), both modes."""
    g = PC.load_golden_params()[entry]
    with mpcq.Engine(g["N"], **g["overrides"]) as e:
        for mode, sfx in ((0, ""), (1, "_setup")):
            r = e.formulate(g["xref"], g["fsteps"], mode)
            assert (r["status"] == 0).all()
            err = max(_rel(r["Ax"], g["Ax" + sfx]), _rel(r["l"], g["l" + sfx]), _rel(r["u"], g["u" + sfx]))
            print(f"entry {entry} ({g['name']}, N={g['N']}) mode {mode}: {err:.2e}")
            assert err <= FORM_TOL, (mode, err)


@pytest.mark.parametrize("case", ["g3.7", "fz12", "form_all"])
@pytest.mark.parametrize("N", [16, 20, 50])
def test_formulation_vs_oracle_under_params(mpcq, oracle, N, case):
    """gravity, fz_max and the weights are literals in the reference: the oracle is the checker."""
    ov = PC.CASES[case]
    p = oracle.default_params(**ov)
    s = PC.make_batch(N)
    with mpcq.Engine(N, **ov) as e:
        for mode in (0, 1):
            r = e.formulate(s["xref"], s["fsteps"], mode)
            assert (r["status"] == 0).all()
            err = 0.0
            for b in range(s["xref"].shape[0]):
                Ax, l, u = oracle.formulate(s["xref"][b], s["fsteps"][b], mode, params=p)
                err = max(err, _rel(r["Ax"][b], Ax), _rel(r["l"][b], l), _rel(r["u"][b], u))
            print(f"N={N} {case} mode {mode}: {err:.2e}")
            assert err <= FORM_TOL, (mode, err)


@pytest.mark.parametrize("case", ["chk7_adp30", "scaling0", "sigma1e-4", "epsabs0"])
@pytest.mark.parametrize("N", [16, 20])
def test_qp_entry_point_vs_oracle(mpcq, oracle, N, case):
    ov = PC.CASES[case]
    p = oracle.default_params(**ov)
    s = PC.make_batch(N)
    B = s["xref"].shape[0]
    qp = [oracle.formulate(s["xref"][b], s["fsteps"][b], 0, params=p) for b in range(B)]
    Ax, l, u = (np.stack([q[i] for q in qp]) for i in range(3))
    with mpcq.Engine(N, **ov) as e:
        r = e.qp_solve(Ax, l, u)
    ex = ey = 0.0
    for b in range(B):
        o = oracle.qp_solve(N, Ax[b], l[b], u[b], params=p)
        for k in ("status", "iters", "rho_updates"):
            assert r[k][b] == o[k], (b, k, r[k][b], o[k])
        dx = float(np.abs(r["x"][b] - o["x"]).max())
        dy = float(np.abs(r["y"][b] - o["y"]).max() / max(1.0, np.abs(o["y"]).max()))
        ex, ey = max(ex, dx), max(ey, dy)
        assert dx < F_TOL, (b, dx)
        assert dy < Y_RTOL, (b, dy)
    print(f"N={N} {case} qp_solve: max|x - x_oracle| {ex:.2e}, y relative {ey:.2e}")


@pytest.mark.parametrize("case", ["chk7_adp30", "mi137"])
def test_slices_with_unaligned_counters(mpcq, oracle, case):
    """N = 20, suspended after 10 and after 45 iterations: the saved countdowns to the next check
    and the next rho update are neither zero nor equal.  Bit-identical to the unsliced solve, which
    equals the oracle."""
    from test_gpu_slice import _same
    N = 20
    ov = PC.CASES[case]
    s = PC.make_batch(N)
    kw = dict(want_x=True, want_y=True)
    with mpcq.Engine(N, **ov) as e0:
        ref = e0.solve(s["xref"], s["fsteps"], 0, **kw)
    _assert_equals_oracle(ref, _oracle_batch(oracle, N, case, ov), f"N={N} {case} unsliced")
    assert ref["iters"].min() > 45     # every instance is suspended by both slices
    for q in (10, 45):
        with mpcq.Engine(N, **ov) as e1:
            e1.set_slice(q)
            _same(ref, e1.solve(s["xref"], s["fsteps"], 0, **kw), f"N={N} {case} slice={q}")


@pytest.mark.parametrize("N", [16, 20])
def test_session_under_params_vs_oracle(mpcq, N):
    """Four host-fed ticks with form_all + chk7_adp30 + dual_warm = 1 and a non-default planner:
    the planner kernel, the retrieve kernel's cost weights and shoulders and the session's
    half-period with anything but defaults.  Tolerances: test_gpu_session.py's."""
    from oracle import oracle as O
    from test_gpu_session import _compare, _gaits, _inputs
    B, T = 6, 4
    ov = dict(PC.CASES["form_all"], **PC.CASES["chk7_adp30"], dual_warm=1)
    gaits = _gaits(B, N)
    rng = np.random.default_rng(11 + N)
    agree, worst = [], 0.0
    with mpcq.Engine(N, **ov) as eng, \
            mpcq.Session(eng, B, gait0=gaits, planner_params=mpcq.default_planner_params(**PC.PLANNER_OVERRIDES)) as sess:
        ors = [O.Session(N, gaits[b], params=O.default_params(**ov),
                         planner_params=O.default_planner_params(**PC.PLANNER_OVERRIDES)) for b in range(B)]
        for k in range(T):
            state, l_feet, v_ref = _inputs(rng, B, k)
            red = (np.arange(B) % 5 == 0).astype(np.int32)
            sess.tick(v_ref, state=state, l_feet=l_feet, reduced=red, k=k)
            for b, o in enumerate(ors):
                o.tick(k, v_ref[b], state=state[b], l_feet=l_feet[b], reduced=bool(red[b]))
            d, _ = _compare(sess, ors, mpcq, k, agree)
            worst = max(worst, d)
    assert len(agree) == B * T and all(agree)
    print(f"N={N}: max |f0 - f0_oracle| over {T} ticks = {worst:.2e}")
