"""Per-robot constants (mpcq_robot tables) shared by test_robots_host.py (CPU) and
test_gpu_robots.py (GPU).

For horizon N the inputs are ``param_cases.make_batch(N)`` and the robots come from
``np.random.default_rng(700 + N)``, drawn per instance in this order: three inertia scales,
a (not symmetric) off-diagonal perturbation, mass, mu, fz_max.  test_robots_host.py shows that
the recipe has power on the oracle: every instance solves, its forces move away from the default
robot's and from its neighbour's robot's, and the oracle's two CPU builds agree on status and
iteration count -- so a kernel that ignores the table, or reads another row, cannot pass the GPU
comparison, and no instance sits on a rounding knife-edge.

The oracle side is one solve per instance with that instance's Params (the oracle takes one
Params per call); the results are computed once per (N, variant) and never modified.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import param_cases as PC

HORIZONS = PC.HORIZONS
_CACHE = {}


def make_robots(N, B=None):
    """The randomised (B,) table of horizon N (mpcq.ROBOT_DTYPE)."""
    import mpcq
    B = PC.batch_size(N) if B is None else B
    d = np.diag(np.array(mpcq.default_params().gI[:]).reshape(3, 3))
    rng = np.random.default_rng(700 + N)
    mass, mu, fz, gI = np.empty(B), np.empty(B), np.empty(B), np.empty((B, 3, 3))
    for b in range(B):
        sc = rng.uniform(0.5, 2.0, 3)
        off = rng.uniform(-0.1, 0.1, (3, 3)) * np.sqrt(np.outer(d * sc, d * sc))
        np.fill_diagonal(off, 0.0)
        gI[b] = np.diag(d * sc) + off
        mass[b] = rng.uniform(1.5, 4.0)
        mu[b] = rng.uniform(0.4, 1.0)
        fz[b] = rng.uniform(20, 30)
    return mpcq.robots(B, mass=mass, gI=gI, mu=mu, fz_max=fz)


def oracle_params(oracle, rob, **ov):
    """The oracle Params of one table row."""
    return oracle.default_params(mass=float(rob["mass"]), gI=tuple(float(v) for v in rob["gI"].ravel()),
                                 mu=float(rob["mu"]), fz_max=float(rob["fz_max"]), **ov)


def oracle_solve(oracle, N, robots=None, native=False, key=None, **ov):
    """Per-instance oracle solves of make_batch(N), instance b with robots[b] (None: the default
    robot), stacked like oracle.solve_batch's result.  ``key`` names the variant in the cache."""
    ck = (N, key, native, tuple(sorted(ov.items())))
    if key is not None and ck in _CACHE:
        return _CACHE[ck]
    s = PC.make_batch(N)
    B = s["xref"].shape[0]
    if native:
        oracle.native_lib()  # (built once, before the threads ask for it)

    def one(b):
        p = oracle.default_params(**ov) if robots is None else oracle_params(oracle, robots[b], **ov)
        return oracle.solve_batch(s["xref"][b:b + 1], s["fsteps"][b:b + 1], 0, params=p, nthreads=1, want_x=True,
                                  native=native)

    with ThreadPoolExecutor(max_workers=8) as ex:
        rs = list(ex.map(one, range(B)))
    out = {k: np.concatenate([r[k] for r in rs]) for k in rs[0]}
    for v in out.values():
        v.flags.writeable = False
    if key is not None:
        _CACHE[ck] = out
    return out
