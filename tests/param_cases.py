"""Non-default mpcq_params settings shared by test_oracle_params.py (CPU) and
test_gpu_params.py (GPU): one dict of overrides per case.  The same kwargs go to
``mpcq.Engine(N, **ov)`` and to ``oracle.default_params(**ov)``; array fields are tuples.

Every case must move the oracle's result away from the defaults' (iteration counts
and forces, test_oracle_params.py::test_case_has_power), so a kernel that ignored the
field, or hard-coded its default, cannot pass the GPU comparison.
"""
import numpy as np

gI_t = (0.05, 0.004, -0.003, 0.002, 0.03, 0.001, -0.001, 0.006, 0.08)   # not symmetric
sw_t = tuple(float(v) for v in np.linspace(0.05, 3.0, 12))

# the ADMM loop's counters and the OSQP settings
LOOP_CASES = {
    "chk7_adp30": dict(check_termination=7, adaptive_rho_interval=30),       # adapt without check
    "chk25_adp40": dict(adaptive_rho_interval=40),
    "chk30_adp20": dict(check_termination=30, adaptive_rho_interval=20),     # check interval the longer
    "chk0_mi500": dict(check_termination=0, max_iter=500),
    "noadapt_mi600": dict(adaptive_rho=0, max_iter=600),
    "adpint0_mi600": dict(adaptive_rho_interval=0, max_iter=600),
    "tol1.5": dict(adaptive_rho_tolerance=1.5),
    "alpha1": dict(alpha=1.0),
    "alpha1.9": dict(alpha=1.9),
    "rho1": dict(rho=1.0),
    "rho1e-3": dict(rho=1e-3),
    "sigma1e-4": dict(sigma=1e-4),
    "scaling0": dict(scaling=0),
    "scaling3": dict(scaling=3),
    "eps1e-4": dict(eps_abs=1e-4, eps_rel=1e-4),
    "epsrel0": dict(eps_rel=0.0, eps_abs=1e-6),
    "epsabs0": dict(eps_abs=0.0, eps_rel=1e-6),
    "mi100": dict(max_iter=100),                                             # a rho update on the last iteration
    "mi137": dict(max_iter=137, check_termination=10, adaptive_rho_interval=35),  # ends unchecked
}

# the formulation's constants
FORM_CASES = {
    "mu0.4": dict(mu=0.4),
    "fz12": dict(fz_max=12.0),
    "mass5": dict(mass=5.0),
    "dt0.01": dict(dt=0.01),
    "g3.7": dict(gravity=3.71),
    "fw1e-3": dict(force_weight=1e-3),
    "sw": dict(state_weights=sw_t),
    "gI": dict(gI=gI_t),
    "form_all": dict(mu=0.55, fz_max=14.0, mass=3.3, dt=0.025, gravity=3.71, gI=gI_t, force_weight=1e-4,
                     state_weights=sw_t),
}

CASES = {**LOOP_CASES, **FORM_CASES}

# one horizon per engine layout: 12 (exit status from LDS, no explicit inverse, no slicing), 16 (the
# explicit-inverse loop), 20 (sliceable, exit status re-derived), 33 (global workspace), 49 (13
# waves), 50 (constraint values in the workspace)
HORIZONS = (12, 16, 20, 33, 49, 50)

POLISH2 = dict(polish=2, polish_rounds=8, polish_refine_iter=10)

PLANNER_OVERRIDES = dict(dt=0.025, T_gait=0.4, h_ref=0.24, t_stance=0.2, L=0.09, g=3.71, cmd_threshold=0.08,
                         shoulders=(0.21, 0.21, -0.17, -0.17, 0.13, -0.13, 0.16, -0.16),
                         reduced_offset=(0.01, 0.02, -0.01, -0.02, 0.03, -0.03, 0.02, -0.02))


def load_golden_params():
    """tests/golden/golden_params.npz (gen_golden.py params) as a list of entries:
    dict(name, N, xref, fsteps, Ax, l, u, Ax_setup, l_setup, u_setup, overrides), where
    ``overrides`` are the stored parameter values as kwargs of default_params / Engine."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_params.npz"))
    out = []
    for i in range(int(d["entries"])):
        pre = f"e{i}_"
        e = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
        e["name"], e["N"] = str(e["name"]), int(e["N"])
        e["overrides"] = dict(dt=float(e.pop("dt")), mass=float(e.pop("mass")), mu=float(e.pop("mu")),
                              gI=tuple(float(v) for v in e.pop("gI")),
                              footholds=tuple(float(v) for v in e.pop("footholds")))
        out.append(e)
    return out


def batch_size(N):
    return 16 if N <= 20 else 8


def make_batch(N):
    """The synthetic mixed-gait batch every test of these cases uses at horizon N."""
    from mpcq import synth
    return synth.make_batch(batch_size(N), N, gaits=synth.GAITS, seed=40 + N)
