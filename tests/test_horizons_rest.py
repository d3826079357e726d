"""CPU: the oracle at the 41 horizons that test_horizons.py leaves out (horizon_cases.REST_HORIZONS),
pinned to fixtures captured from the unmodified reference MPC.py (tests/golden/gen_golden.py
horizons_rest: golden_horizons_rest_a.npz for N <= 32, three instances each, and _b.npz beyond,
one instance each): the CSC pattern of the oracle and of the library, the update-mode A / l / u
handed to OSQP, the polished solve on the certified optimum x*, the malformed gaits.  Setup mode
is not in these files; test_horizons.py pins the oracle's at 18 horizons.

test_every_compiled_horizon_has_a_fixture is the coverage assertion: all fixture files together
hold N = 4 ... 64 exactly once each, the horizons the engine compiles."""
import numpy as np
import pytest
from horizon_cases import ALL_HORIZONS, REST_HORIZONS, fixture_horizons, golden_for
from test_horizons import FORM_TOL, _rel

FIELDS = {"xref", "fsteps", "gait", "Ax", "l", "u", "x_star", "kkt", "P", "indptr", "indices",
          "bad_fsteps", "bad_raises", "bad_xref"}


@pytest.fixture(scope="module")
def mpcq():
    import mpcq as M
    return M


def test_every_compiled_horizon_has_a_fixture(mpcq):
    from conftest import FIXTURE_HORIZONS
    assert fixture_horizons() == ALL_HORIZONS == tuple(range(4, 65))
    assert tuple(mpcq.supported_horizons()) == ALL_HORIZONS
    assert tuple(sorted(set(REST_HORIZONS) | set(FIXTURE_HORIZONS) | {16, 32})) == ALL_HORIZONS
    assert len(REST_HORIZONS) == 41 and not set(REST_HORIZONS) & (set(FIXTURE_HORIZONS) | {16, 32})


@pytest.mark.parametrize("N", REST_HORIZONS)
def test_fixture_shapes(N):
    g = golden_for(N)
    assert set(g) == FIELDS
    B = 3 if N <= 32 else 1
    assert g["xref"].shape == (B, 12, N + 1) and g["fsteps"].shape == (B, 20, 13)
    assert g["gait"].tolist() == ([0, 1, 2] if N <= 32 else [N % 3])
    assert g["Ax"].shape == (B, 126 * N - 18)
    assert g["l"].shape == g["u"].shape == (B, 44 * N)
    assert g["x_star"].shape == (B, 24 * N) and g["P"].shape == (24 * N,)
    assert g["kkt"].shape == (B, 4)
    assert g["kkt"].max() < 1e-12  # x* certified by its KKT residuals
    assert g["bad_fsteps"].shape == (3, 20, 13) and g["bad_xref"].shape == (12, N + 1)


@pytest.mark.parametrize("N", REST_HORIZONS)
def test_pattern(oracle, mpcq, N):
    g = golden_for(N)
    for indptr, indices in (oracle.pattern(N), mpcq.pattern(N)):
        assert np.array_equal(indptr, g["indptr"])
        assert np.array_equal(indices, g["indices"])


@pytest.mark.parametrize("N", REST_HORIZONS)
def test_formulation(oracle, N):
    g = golden_for(N)
    worst = 0.0
    for b in range(g["xref"].shape[0]):
        Ax, l, u = oracle.formulate(g["xref"][b], g["fsteps"][b], 0)
        worst = max(worst, _rel(Ax, g["Ax"][b]), _rel(l, g["l"][b]), _rel(u, g["u"][b]))
    assert worst <= FORM_TOL, worst


@pytest.mark.parametrize("N", REST_HORIZONS)
def test_polish_reaches_optimum(oracle, N):
    g = golden_for(N)
    p = oracle.default_params(polish=2, polish_rounds=8, polish_refine_iter=10)
    worst = 0.0
    for b in range(g["xref"].shape[0]):
        r = oracle.qp_solve(N, g["Ax"][b], g["l"][b], g["u"][b], params=p)
        assert r["status"] == 1
        worst = max(worst, np.abs(r["x"][12 * N:] - g["x_star"][b][12 * N:]).max())
    assert worst < 1e-8, worst


@pytest.mark.parametrize("N", REST_HORIZONS)
def test_bad_gaits_rejected_like_reference(oracle, N):
    g = golden_for(N)
    assert all(len(s) > 0 for s in g["bad_raises"])
    for f in g["bad_fsteps"]:
        with pytest.raises(ValueError):
            oracle.formulate(g["bad_xref"], f, 0)
