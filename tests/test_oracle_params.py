"""CPU: the oracle under non-default mpcq_params (tests/param_cases.py).

test_gpu_params.py compares the engine with the oracle under every case of the table, so
two things are pinned here, without a GPU:

* each case has power: on the N = 16 and N = 33 batches it moves the oracle's iteration
  counts (>= 2 instances) and forces (>= 1e-5 on >= 1 instance) away from the defaults'.  A
  kernel that ignored the field would then miss the oracle by 200x the GPU tolerance.  This
  is a condition on the inputs, not a tolerance: a case that fails it is replaced, not relaxed.
* the oracle's formulation under non-default mass / mu / gI (not symmetric) / dt / default
  footholds equals the unmodified reference's (tests/golden/golden_params.npz, written by
  gen_golden.py params), within the 1e-14 relative of test_oracle_golden.py.
"""
import numpy as np
import pytest

import param_cases as PC

FORM_TOL = 1e-14   # as test_oracle_golden.py (observed <= 4.4e-16)
POWER_HORIZONS = (16, 33)


@pytest.fixture(scope="module")
def default_runs(oracle):
    out = {}
    for N in POWER_HORIZONS:
        s = PC.make_batch(N)
        out[N] = (s, oracle.solve_batch(s["xref"], s["fsteps"], 0, nthreads=8))
    return out


def test_case_table_is_complete(oracle):
    assert len(PC.LOOP_CASES) == 19 and len(PC.FORM_CASES) == 9 and len(PC.CASES) == 28
    fields = {name for name, _ in oracle.Params._fields_}
    for name, ov in PC.CASES.items():
        assert set(ov) <= fields, name
        p, d = oracle.default_params(**ov), oracle.default_params()
        for k, v in ov.items():  # every override is a change
            a, b = getattr(p, k), getattr(d, k)
            assert (list(a) != list(b)) if hasattr(a, "__len__") else (a != b), (name, k)


@pytest.mark.parametrize("N", POWER_HORIZONS)
@pytest.mark.parametrize("case", list(PC.CASES))
def test_case_has_power(oracle, default_runs, case, N):
    s, d = default_runs[N]
    r = oracle.solve_batch(s["xref"], s["fsteps"], 0, params=oracle.default_params(**PC.CASES[case]), nthreads=8)
    n_iters = int((r["iters"] != d["iters"]).sum())
    df = np.abs(r["f0"] - d["f0"]).max(axis=1)
    assert n_iters >= 2, (n_iters, r["iters"], d["iters"])
    assert (df >= 1e-5).sum() >= 1, df.max()


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.array_equal(np.isinf(a), np.isinf(b))
    fa, fb = np.where(np.isinf(a), 0.0, a), np.where(np.isinf(b), 0.0, b)
    return float((np.abs(fa - fb) / np.maximum(1.0, np.abs(fb))).max(initial=0.0))


def test_golden_params_fixture_covers_the_issue():
    ents = PC.load_golden_params()
    assert [(e["name"], e["N"]) for e in ents] == [("all", 5), ("all", 16), ("all", 20), ("all", 50), ("mass", 16),
                                                   ("mu", 16), ("gI", 16), ("dt", 16), ("footholds", 16)]
    for e in ents:
        assert e["xref"].shape == (3, 12, e["N"] + 1) and e["Ax"].shape == (3, 126 * e["N"] - 18)
    a = ents[1]["overrides"]
    assert (a["mass"], a["mu"], a["dt"], a["gI"]) == (3.3, 0.55, 0.025, PC.gI_t)


@pytest.mark.parametrize("entry", range(9))
def test_formulation_matches_reference_under_params(oracle, entry):
    """oracle.formulate(params=) against what the unmodified reference hands to OSQP with the same
    mass / mu / gI / dt / footholds (the values are read from the fixture), both modes.
    gravity, fz_max, force_weight and state_weights are literals in the reference (MPC.py:201,
    :228, :255-275), so no reference run can vary them: for those the oracle is the only checker
    (its reading of them is pinned at the defaults by test_oracle_golden.py, and certify.py's KKT
    check in test_gpu_params.py takes the weights from the parameters independently of the ADMM)."""
    e = PC.load_golden_params()[entry]
    p = oracle.default_params(**e["overrides"])
    d = oracle.default_params()
    changed = [k for k, v in e["overrides"].items()
               if (list(getattr(p, k)) != list(getattr(d, k)) if isinstance(v, tuple) else getattr(p, k) != getattr(d, k))]
    assert changed == (["dt", "mass", "mu", "gI", "footholds"] if e["name"] == "all" else [e["name"]])
    worst = 0.0
    for mode, sfx in ((0, ""), (1, "_setup")):
        for b in range(3):
            Ax, l, u = oracle.formulate(e["xref"][b], e["fsteps"][b], mode, params=p)
            worst = max(worst, _rel(Ax, e["Ax" + sfx][b]), _rel(l, e["l" + sfx][b]), _rel(u, e["u" + sfx][b]))
            # the entry has power: the defaults miss the fixture
            A0, l0, u0 = oracle.formulate(e["xref"][b], e["fsteps"][b], mode)
            if mode == 1 or e["name"] != "footholds":   # the default footholds enter the setup mode only
                assert max(_rel(A0, e["Ax" + sfx][b]), _rel(l0, e["l" + sfx][b])) > 1e-6, (mode, b)
    print(f"entry {entry} ({e['name']}, N={e['N']}): worst relative {worst:.2e}")
    assert worst <= FORM_TOL, worst
