"""GPU: every compiled horizon, N = 4 ... 64 -- one code object each, each through the assembly
pass on its own -- against the reference fixtures (horizon_cases.golden_for) and the oracle.

One test function per check, each parametrised over all 61 horizons, at most 12 instances per
case (a fixture with more is thinned evenly, first and last instance kept):

a. formulation: mode 0 against the reference fixture, mode 1 against the oracle (whose setup
   mode test_horizons.py pins to the reference), relative error <= FORM_TOL.
b. qp_solve on the fixture QPs against the oracle: status and iteration count equal, x within
   X_TOL of the solution's scale; then polish = 2 on the certified optimum x*, which does not
   depend on the oracle sharing the engine's algorithm.
c. the fused cold solve of synth_batch(N, 700) against oracle.solve_batch (status and iterations
   array-equal, f0 within F_TOL), then the QPs of synth_batch(N, 800) warm-started from the cold
   x, y, rho under both dual carry-overs, against the oracle warm-started from its own cold
   result: status and iterations equal, x within W_TOL of the scale and y within Y_RTOL
   relative; beyond 48 stages x within test_gpu_session.py's SCALED_TOL (its docstring says
   where the difference at those layouts comes from), y within Y_RTOL as below.  These bounds
   come from test_gpu_parity.py (N = 16) and test_gpu_session.py (N = 49 ... 64), not from
   these horizons; DESIGN.md has the table of what each horizon showed.
d. set_slice(40) and set_slice(150) on the cold batch of (c): bit-identical outputs on every key
   of test_gpu_slice.KEYS.  Up to 16 stages slicing is compiled out and must stay a no-op;
   beyond, some instance has to iterate past the longer slice, or the case checked nothing.

The oracle's cold batch solve is computed once per horizon and shared by the two cases of (c)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from horizon_cases import ALL_HORIZONS, golden_for, synth_batch
from test_gpu_slice import KEYS

pytestmark = pytest.mark.gpu

FORM_TOL = 1e-13   # test_gpu_parity.FORM_TOL
X_TOL = 1e-9       # test_gpu_horizons.X_TOL, relative to max(1, max |x|)
F_TOL = 5e-8       # test_gpu_horizons.F_TOL
POLISH_TOL = 1e-8  # test_gpu_parity.test_polish_reaches_optimum
W_TOL, Y_RTOL = 1e-8, 1e-6  # test_gpu_parity.test_dual_warm_vs_oracle, relative to max(1, max |.|)
SCALED_TOL = 5e-7  # test_gpu_session.SCALED_TOL: x beyond 48 stages, relative to max(1, max |x|)
POLISH = dict(polish=2, polish_rounds=8, polish_refine_iter=10)
SLICES = (40, 150)
THREADS = 12


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.array_equal(np.isinf(a), np.isinf(b))
    fa, fb = np.where(np.isinf(a), 0, a), np.where(np.isinf(b), 0, b)
    return float((np.abs(fa - fb) / np.maximum(1.0, np.abs(fb))).max(initial=0))


def _scaled(a, b):
    """max |a - b| relative to max(1, max |b|)."""
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _fixture(N):
    """The fixture at N, thinned to at most 12 instances."""
    g = golden_for(N)
    B = g["xref"].shape[0]
    idx = np.unique(np.linspace(0, B - 1, min(B, 12)).round().astype(int))
    return {k: g[k][idx] for k in ("xref", "fsteps", "Ax", "l", "u", "x_star")}


def _each(fn, B):
    """fn(b) for every instance, on host threads (the oracle's C code holds no global state)."""
    with ThreadPoolExecutor(THREADS) as pool:
        return list(pool.map(fn, range(B)))


@functools.lru_cache(maxsize=None)
def _oracle_batch(N):
    from oracle import oracle as O
    O.build()
    s = synth_batch(N, 700)
    return O.solve_batch(s["xref"], s["fsteps"], 0, nthreads=16)


def _oracle_cold(N, dual_warm):
    """The oracle on synth_batch(N, 700): solve_batch's status / iters / f0, and x, y, rho of the
    same solves instance by instance (solve_batch returns no y or rho; y is the carry-over of
    ``dual_warm``), which must agree with the batch."""
    from oracle import oracle as O
    ob = _oracle_batch(N)
    s = synth_batch(N, 700)
    p = O.default_params(dual_warm=dual_warm)

    def one(b):
        Ax, l, u = O.formulate(s["xref"][b], s["fsteps"][b], 0, p)
        return O.qp_solve(N, Ax, l, u, params=p)
    oc = _each(one, 12)
    assert [o["status"] for o in oc] == ob["status"].tolist()
    assert [o["iters"] for o in oc] == ob["iters"].tolist()
    assert np.array_equal(np.array([o["x"][12 * N:12 * N + 12] for o in oc]), ob["f0"])
    return ob, oc


@pytest.mark.parametrize("N", ALL_HORIZONS)
def test_formulation(mpcq, oracle, N):
    g = _fixture(N)
    B = g["xref"].shape[0]
    with mpcq.Engine(N) as e:
        r0 = e.formulate(g["xref"], g["fsteps"], 0)
        r1 = e.formulate(g["xref"], g["fsteps"], 1)
    assert (r0["status"] == 0).all() and (r1["status"] == 0).all()
    err0 = max(_rel(r0[k], g[k]) for k in ("Ax", "l", "u"))
    err1 = 0.0
    for b in range(B):
        Ax, l, u = oracle.formulate(g["xref"][b], g["fsteps"][b], 1)
        err1 = max(err1, _rel(r1["Ax"][b], Ax), _rel(r1["l"][b], l), _rel(r1["u"][b], u))
    print(f"OBS a N={N} B={B} form0={err0:.2e} form1={err1:.2e}")
    assert err0 <= FORM_TOL, err0
    assert err1 <= FORM_TOL, err1


@pytest.mark.parametrize("N", ALL_HORIZONS)
def test_qp_solve_and_polish(mpcq, oracle, N):
    g = _fixture(N)
    B = g["Ax"].shape[0]
    with mpcq.Engine(N) as e:
        r = e.qp_solve(g["Ax"], g["l"], g["u"])
    with mpcq.Engine(N, **POLISH) as e:
        rp = e.qp_solve(g["Ax"], g["l"], g["u"])
    oracle.default_params()
    os_ = _each(lambda b: oracle.qp_solve(N, g["Ax"][b], g["l"][b], g["u"][b]), B)
    xerr = max(_scaled(r["x"][b], o["x"]) for b, o in enumerate(os_))
    d = float(np.abs(rp["x"][:, 12 * N:] - g["x_star"][:, 12 * N:]).max())
    print(f"OBS b N={N} B={B} x={xerr:.2e} polished={d:.2e} iters_max={int(r['iters'].max())}")
    for b, o in enumerate(os_):
        assert r["status"][b] == o["status"], (b, r["status"][b], o["status"])
        assert r["iters"][b] == o["iters"], (b, r["iters"][b], o["iters"])
        assert _scaled(r["x"][b], o["x"]) < X_TOL, (b, _scaled(r["x"][b], o["x"]))
    assert (rp["status"] == 1).all(), rp["status"]
    assert (rp["polish"] == 1).all(), rp["polish"]
    assert d < POLISH_TOL, d


@pytest.mark.parametrize("N", ALL_HORIZONS)
@pytest.mark.parametrize("dual_warm", [0, 1])
def test_cold_then_warm(mpcq, oracle, N, dual_warm):
    """With these seeds the oracle ends every cold instance with status 1, except one each at
    N = 48, 59, 60 and two at N = 64 that stop at max_iter with status 2: the max-iter exit of
    those layouts."""
    s7, s8 = synth_batch(N, 700), synth_batch(N, 800)
    ob, oc = _oracle_cold(N, dual_warm)
    p = oracle.default_params(dual_warm=dual_warm)

    def warm(b):
        Ax, l, u = oracle.formulate(s8["xref"][b], s8["fsteps"][b], 0, p)
        return oracle.qp_solve(N, Ax, l, u, params=p, warm_x=oc[b]["x"], warm_y=oc[b]["y"], rho=oc[b]["rho"])
    ow = _each(warm, 12)
    with mpcq.Engine(N, dual_warm=dual_warm) as e:
        rc = e.solve(s7["xref"], s7["fsteps"], 0, want_x=True, want_y=True)
        rw = e.solve(s8["xref"], s8["fsteps"], 0, warm_x=rc["x"], warm_y=rc["y"], rho=rc["rho"],
                     want_x=True, want_y=True)
    ferr = float(np.abs(rc["f0"] - ob["f0"]).max())
    xw = max(_scaled(rw["x"][b], o["x"]) for b, o in enumerate(ow))
    yw = max(_scaled(rw["y"][b], o["y"]) for b, o in enumerate(ow))
    print(f"OBS c N={N} dw={dual_warm} f0={ferr:.2e} warm_x={xw:.2e} warm_y={yw:.2e} "
          f"cold_iters_max={int(rc['iters'].max())} cold_status2={int((rc['status'] == 2).sum())} "
          f"warm_iters_max={int(rw['iters'].max())}")
    assert np.isin(ob["status"], (1, 2)).all()
    assert np.array_equal(rc["status"], ob["status"]), (rc["status"], ob["status"])
    assert np.array_equal(rc["iters"], ob["iters"]), (rc["iters"], ob["iters"])
    assert ferr < F_TOL, ferr
    x_tol = W_TOL if N <= 48 else SCALED_TOL
    for b, o in enumerate(ow):
        assert rw["status"][b] == o["status"], (b, rw["status"][b], o["status"])
        assert rw["iters"][b] == o["iters"], (b, rw["iters"][b], o["iters"])
        assert _scaled(rw["x"][b], o["x"]) < x_tol, (b, _scaled(rw["x"][b], o["x"]))
        assert _scaled(rw["y"][b], o["y"]) < Y_RTOL, (b, _scaled(rw["y"][b], o["y"]))


@pytest.mark.parametrize("N", ALL_HORIZONS)
def test_slices_change_no_result(mpcq, N):
    s = synth_batch(N, 700)
    kw = dict(want_x=True, want_y=True)
    with mpcq.Engine(N) as e0:
        ref = e0.solve(s["xref"], s["fsteps"], 0, **kw)
    assert np.isin(ref["status"], (1, 2)).all(), ref["status"]
    if N > 16:
        assert ref["iters"].max() > max(SLICES), ref["iters"]  # both slice lengths are crossed
    with mpcq.Engine(N) as e1:
        for q in SLICES:
            e1.set_slice(q)
            got = e1.solve(s["xref"], s["fsteps"], 0, **kw)
            for k in KEYS:
                assert ref[k] is not None
                assert np.array_equal(ref[k], got[k], equal_nan=True), (N, q, k)
