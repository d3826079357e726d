"""GPU: the segment boundary of the N <= 32 ADMM loop (the checked iteration, infeas_cheap,
update_info, the decision, the refill of the held right-hand-side operands) against the oracle.

The loop leaves its innermost loop every min(to_check, to_adapt, iterations left) iterations; what
happens there depends on which of the three ended the segment.  Batches of 8 seeded trot instances
at N = 4 (one wave), 7 (two waves, a phantom row), 16 (the flagship), 17 (five waves, three phantom
rows) and 32 (eight waves), under settings that move the boundary (check_termination /
adaptive_rho_interval):

* default        25 / 100;
* chk1_adp1      1 / 1: every segment is a lone checked iteration, a rho update may follow each;
* chk2_adp3      2 / 3: check and adapt points interleave and coincide every 6 iterations;
* chk7_adp10_mi23  7 / 10, max_iter 23: the last iteration falls mid-segment and is unchecked;
* mi100          25 / 100, max_iter 100: a rho update is due on the last iteration;
* adp_off        adaptive_rho off.

and one warm start at N = 16 (a second launch from the first one's x, y and rho, so the operands
are refilled after a carried-over rho).  Per case: status, iteration count and rho-update count
equal the oracle's on every instance, forces and x within X_TOL = 1e-9 (tests/test_gpu_parity.py's
bound for GPU vs oracle solutions; the warm start within its W_TOL = 1e-8, test_dual_warm_vs_oracle),
and a repeated launch is bitwise equal.

What the oracle alone says about the cases (CPU, seeds 80 + N; asserted below from the oracle's
result, so a changed seed or default that empties a case fails here and not silently): default,
chk1_adp1 and chk2_adp3 each have instances that end by convergence and instances that cross a rho
update at every horizon (chk1_adp1 also has instances that reach max_iter after hundreds of
updates); chk7_adp10_mi23 and mi100 end at max_iter by construction, every instance after at
least one rho update; adp_off ends at max_iter (4000) without one, by construction.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_TOL = 1e-9   # tests/test_gpu_parity.py: GPU vs oracle solutions
W_TOL = 1e-8   # tests/test_gpu_parity.py::test_dual_warm_vs_oracle: the second of two solves

HORIZONS = (4, 7, 16, 17, 32)
CASES = {
    "default": dict(),
    "chk1_adp1": dict(check_termination=1, adaptive_rho_interval=1),
    "chk2_adp3": dict(check_termination=2, adaptive_rho_interval=3),
    "chk7_adp10_mi23": dict(check_termination=7, adaptive_rho_interval=10, max_iter=23),
    "mi100": dict(max_iter=100),
    "adp_off": dict(adaptive_rho=0),
}
# what each case can show: (an instance that ends by convergence, one that crosses a rho update)
EXPECT = {
    "default": (True, True), "chk1_adp1": (True, True), "chk2_adp3": (True, True),
    "chk7_adp10_mi23": (False, True), "mi100": (False, True), "adp_off": (False, False),
}

_BATCH = {}
_ORACLE = {}  # (N, case) -> the oracle's result, computed once and never modified


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def _batch(mpcq, N, shift=0):
    if (N, shift) not in _BATCH:
        _BATCH[(N, shift)] = mpcq.synth.make_batch(8, N, gaits=("trot",), seed=80 + N + shift)
    return _BATCH[(N, shift)]


def _freeze(o):
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return o


def _oracle_case(oracle, mpcq, N, case):
    if (N, case) not in _ORACLE:
        b = _batch(mpcq, N)
        _ORACLE[(N, case)] = _freeze(oracle.solve_batch(
            b["xref"], b["fsteps"], 0, params=oracle.default_params(**CASES[case]), nthreads=8, want_x=True))
    return _ORACLE[(N, case)]


def _bitwise(a, b, tag):
    for k in ("f0", "x", "status", "iters", "rho", "rho_updates"):
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), \
            (tag, "repeated launch differs in", k)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("N", HORIZONS)
def test_boundary_vs_oracle(mpcq, oracle, N, case):
    o = _oracle_case(oracle, mpcq, N, case)
    conv, upd = EXPECT[case]
    assert bool((o["status"] == mpcq.STATUS_SOLVED).any()) == conv, (N, case, o["status"].tolist())
    assert bool((o["rho_updates"] > 0).any()) == upd, (N, case, o["rho_updates"].tolist())
    b = _batch(mpcq, N)
    with mpcq.Engine(N, **CASES[case]) as e:
        r = e.solve(b["xref"], b["fsteps"], mpcq.MODE_UPDATE, want_x=True)
        r2 = e.solve(b["xref"], b["fsteps"], mpcq.MODE_UPDATE, want_x=True)
    ef = float(np.abs(r["f0"] - o["f0"]).max())
    ex = float(np.abs(r["x"] - o["x"]).max())
    print(f"N={N} {case}: max|f0 - f0_oracle| {ef:.2e}, max|x - x_oracle| {ex:.2e}, iters {o['iters'].tolist()}, "
          f"rho updates {o['rho_updates'].tolist()}, statuses {o['status'].tolist()}")
    for k in ("status", "iters", "rho_updates"):
        assert np.array_equal(r[k], o[k]), (N, case, k, r[k].tolist(), o[k].tolist())
    assert ef < X_TOL, (N, case, ef)
    assert ex < X_TOL, (N, case, ex)
    _bitwise(r, r2, (N, case))


def test_warm_start_second_launch(mpcq, oracle):
    """Two launches at N = 16: a cold solve of one batch, then another batch warm-started from its
    x, y and rho (MODE_UPDATE), so the first segment's operands are refilled after a factorisation
    at the carried-over rho.  The oracle takes the same two steps per instance."""
    N = 16
    b1, b2 = _batch(mpcq, N), _batch(mpcq, N, shift=100)
    with mpcq.Engine(N) as e:
        r1 = e.solve(b1["xref"], b1["fsteps"], mpcq.MODE_UPDATE, want_x=True, want_y=True)
        w = dict(warm_x=r1["x"], warm_y=r1["y"], rho=r1["rho"], want_x=True)
        r2 = e.solve(b2["xref"], b2["fsteps"], mpcq.MODE_UPDATE, **w)
        r3 = e.solve(b2["xref"], b2["fsteps"], mpcq.MODE_UPDATE, **w)
    _bitwise(r2, r3, "warm")
    conv = upd = False
    for i in range(8):
        o1 = oracle.qp_solve(N, *oracle.formulate(b1["xref"][i], b1["fsteps"][i], 0))
        assert abs(o1["rho"] - 0.1) > 1e-3, (i, o1["rho"])  # the carried-over rho is not the default
        o2 = oracle.qp_solve(N, *oracle.formulate(b2["xref"][i], b2["fsteps"][i], 0),
                             warm_x=o1["x"], warm_y=o1["y"], rho=o1["rho"])
        conv |= o2["status"] == mpcq.STATUS_SOLVED
        upd |= o2["rho_updates"] > 0
        got = (int(r2["status"][i]), int(r2["iters"][i]), int(r2["rho_updates"][i]))
        assert got == (o2["status"], o2["iters"], o2["rho_updates"]), (i, got, o2["status"], o2["iters"], o2["rho_updates"])
        ex = float(np.abs(r2["x"][i] - o2["x"]).max())
        ef = float(np.abs(r2["f0"][i] - o2["x"][12 * N:12 * N + 12]).max())
        print(f"warm {i}: iters {o2['iters']}, rho updates {o2['rho_updates']}, max|x - x_oracle| {ex:.2e}")
        assert ex < W_TOL and ef < W_TOL, (i, ex, ef)
    assert conv and upd
