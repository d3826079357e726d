"""CPU: every (case, horizon) of tests/infeas_cases.py has the power it claims, on the oracle alone.

For each pair: the case's EXPECT condition holds on the oracle's result (so a changed seed or value
cannot quietly empty the case), and the result is robust -- statuses and iteration counts are
identical with the case's eps_prim_inf / eps_dual_inf scaled by 1.001 and by 0.999.  The GPU and
the oracle differ by ~1e-9 relative on these solves (tests/test_gpu_params.py), so six decades lie
between a legitimate rounding difference and a flipped decision: a disagreement of the GPU on one
of these instances (tests/test_gpu_infeas.py) is a finding in the engine, not a knife-edge.

The variants the GPU module runs on top of the table -- polish = 2 at N = 16, a per-robot table
at N = 16 / 33, the sessions -- are shown robust in the same way.
"""
import numpy as np
import pytest

import infeas_cases as IC

SCALES = (1.001, 0.999)


def _same_outcome(a, b, tag):
    for k in ("status", "iters", "rho_updates", "admm_status"):
        assert np.array_equal(a[k], b[k]), (tag, k, a[k].tolist(), b[k].tolist())


def test_table_covers_the_layouts():
    """All nine horizons for the hand-made rows, fused_epi and dinf_first; for every other case at
    least one horizon with the exit status in LDS (N <= 16), one with it re-derived (17..48, which
    has 33's global workspace), and one beyond 48."""
    for name, c in IC.CASES.items():
        Ns = set(c["params"])
        if name.startswith("hand_") or name in ("fused_epi", "dinf_first"):
            assert Ns == set(IC.HORIZONS), name
        assert Ns <= set(IC.HORIZONS)
        assert any(n <= 16 for n in Ns) and any(17 <= n <= 32 for n in Ns) and 33 in Ns and any(n > 48 for n in Ns), name


@pytest.mark.parametrize("name,N", IC.PAIRS)
def test_case_has_power_and_is_robust(oracle, name, N):
    o = IC.oracle_solve(oracle, N, name)
    print(f"{name} N={N}: statuses {o['status'].tolist()}, iters {o['iters'].tolist()}")
    IC.EXPECT[name](N, o, IC.base_solve(oracle, N, name))
    nan = np.isin(o["status"], IC.NAN_STATUSES)
    assert np.isnan(o["x"][nan]).all() and np.isnan(o["y"][nan]).all()
    assert np.isfinite(o["x"][~nan]).all() and np.isfinite(o["y"][~nan]).all()
    for sc in SCALES:
        _same_outcome(o, IC.oracle_solve(oracle, N, name, scale=sc), f"{name} N={N} x{sc}")


@pytest.mark.parametrize("name", ["hand_mid", "fused_epi"])
def test_polish2_variant_is_robust(oracle, name):
    """polish = 2 at N = 16 (the engine's general loop): an infeasible exit is never polished."""
    import param_cases as PC
    N = 16
    o = IC.oracle_solve(oracle, N, name, extra=PC.POLISH2)
    IC.EXPECT[name](N, o, IC.oracle_solve(oracle, N, name, extra=PC.POLISH2, base=True))
    nan = np.isin(o["status"], IC.NAN_STATUSES)
    assert nan.any() and (o["polish"][nan] == 0).all() and np.array_equal(o["admm_status"][nan], o["status"][nan])
    for sc in SCALES:
        r = IC.oracle_solve(oracle, N, name, scale=sc, extra=PC.POLISH2)
        _same_outcome(o, r, f"{name} polish=2 x{sc}")
        assert np.array_equal(o["polish"], r["polish"])


@pytest.mark.parametrize("N", [16, 33])
def test_robot_table_variant_has_power_and_is_robust(oracle, N):
    """fused_epi under a per-robot table: -3 and SOLVED both occur, the table moves at least one
    outcome away from the default robot's, and nothing flips at 1 +- 1e-3."""
    import robot_cases as RC
    rob = RC.make_robots(N, IC.B)
    assert len(set(rob["fz_max"].tolist())) == IC.B and len(set(rob["mu"].tolist())) == IC.B
    o = IC.oracle_solve(oracle, N, "fused_epi", robots=rob)
    print(f"fused_epi N={N} robots: statuses {o['status'].tolist()}, iters {o['iters'].tolist()}")
    assert (o["status"] == IC.PINF).sum() >= 2 and (o["status"] == IC.SOLVED).any(), o["status"].tolist()
    d = IC.oracle_solve(oracle, N, "fused_epi")
    assert not (np.array_equal(o["status"], d["status"]) and np.array_equal(o["iters"], d["iters"]))
    for sc in SCALES:
        _same_outcome(o, IC.oracle_solve(oracle, N, "fused_epi", scale=sc, robots=rob), f"robots N={N} x{sc}")


@pytest.mark.parametrize("N", sorted(IC.SESSION_EPI))
def test_session_fails_and_recovers_robustly(oracle, N):
    st, it = IC.oracle_session_run(oracle, N)
    print(f"session N={N}: statuses {st.tolist()}, iters {it.tolist()}")
    IC.expect_session(st)
    for sc in SCALES:
        s2, i2 = IC.oracle_session_run(oracle, N, sc)
        assert np.array_equal(st, s2) and np.array_equal(it, i2), (sc, s2.tolist(), i2.tolist())


def test_generalised_instance_contains_the_first_stage_one(oracle, golden16):
    """tests/test_infeasibility.py's instance (stage 0 only) is the generalised one where a foot
    swings at stage 0."""
    from test_infeasibility import infeasible_instance
    seen = 0
    for b in range(0, 50, 5):
        a = infeasible_instance(golden16, b)
        if a is None:
            continue
        g = IC.infeasible_instance(16, golden16["Ax"][b], golden16["l"][b], golden16["u"][b], golden16["fsteps"][b], "first")
        assert IC.infeasible_row(16, golden16["fsteps"][b], "first")[0] == 0
        assert all(np.array_equal(p, q) for p, q in zip(a, g))
        seen += 1
    assert seen >= 5
