"""Per-instance disturbance accelerations (mpcq_disturbance tables) shared by
test_disturbance_host.py (CPU) and test_gpu_disturbance.py (GPU).

For horizon N the inputs are ``param_cases.make_batch(N)`` and the rows come from
``np.random.default_rng(1100 + N)``, drawn per instance in this order: two ``uniform(-2, 2)``
(a_x, a_y), one ``uniform(-3, 3)`` (a_z), three ``uniform(-5, 5)`` (the angular part).
test_disturbance_host.py shows that the recipe has power on the oracle: the statuses are the
unshifted batch's, every instance's forces move away from the unshifted result and from the
result under its neighbour's row -- so a kernel that ignores the table, or reads another row,
cannot pass the GPU comparison.

The reference has no disturbance (its model knows gravity only), so the oracle side is built at
the QP level: ``oracle.formulate`` of the instance, then ``l[12k+6 : 12k+12] += -(dt * a)`` and the
same on ``u`` for every stage k (in MPC.py's terms g[6+i] += dt * a[i]), then ``oracle.qp_solve``.
The results are computed once per (N, variant) and never modified.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import param_cases as PC

HORIZONS = PC.HORIZONS
_CACHE = {}


def make_disturbances(N, B=None):
    """The randomised (B,) table of horizon N (mpcq.DISTURBANCE_DTYPE)."""
    import mpcq
    B = PC.batch_size(N) if B is None else B
    rng = np.random.default_rng(1100 + N)
    a = np.empty((B, 6))
    for b in range(B):
        a[b, 0:2] = rng.uniform(-2, 2, 2)
        a[b, 2] = rng.uniform(-3, 3)
        a[b, 3:6] = rng.uniform(-5, 5, 3)
    return mpcq.disturbances(B, lin=a[:, :3], ang=a[:, 3:])


def shift_bounds(l, u, N, dt, a):
    """l, u of one instance (copies) with the disturbance ``a`` [6] in every stage's dynamics rows."""
    l, u = l.copy(), u.copy()
    d = -(dt * np.asarray(a, np.float64))
    for k in range(N):
        l[12 * k + 6:12 * k + 12] += d
        u[12 * k + 6:12 * k + 12] += d
    return l, u


def oracle_formulate(oracle, xref, fsteps, a, params=None, mode=0):
    """oracle.formulate of one instance, then the shift: (Ax, l, u)."""
    p = params or oracle.default_params()
    Ax, l, u = oracle.formulate(xref, fsteps, mode, p)
    N = xref.shape[1] - 1
    if a is not None:
        l, u = shift_bounds(l, u, N, p.dt, a)
    return Ax, l, u


def oracle_solve_one(oracle, xref, fsteps, a, params=None, mode=0, **warm):
    """One instance through formulate -> shift -> qp_solve; qp_solve's dict plus f0, Ax, l, u."""
    p = params or oracle.default_params()
    N = xref.shape[1] - 1
    Ax, l, u = oracle_formulate(oracle, xref, fsteps, a, p, mode)
    r = oracle.qp_solve(N, Ax, l, u, p, **warm)
    r["f0"] = r["x"][12 * N:12 * N + 12].copy()
    r["Ax"], r["l"], r["u"] = Ax, l, u
    return r


def oracle_solve(oracle, N, table=None, robots=None, weights=None, key=None):
    """Per-instance reference solves of make_batch(N), instance b with a = table[b]["a"] (None: no
    shift), robots[b] and weights[b] in its Params (None: the defaults), stacked like
    oracle.solve_batch's result (f0, x, status, iters, rho_updates, admm_status) plus l, u.
    ``key`` names the variant in the cache."""
    import robot_cases as RC
    import weight_cases as WC
    ck = (N, key)
    if key is not None and ck in _CACHE:
        return _CACHE[ck]
    s = PC.make_batch(N)
    B = s["xref"].shape[0]
    oracle.lib()  # (built once, before the threads ask for it)

    def one(b):
        kw = {} if weights is None else WC.oracle_overrides(weights[b])
        p = oracle.default_params(**kw) if robots is None else RC.oracle_params(oracle, robots[b], **kw)
        return oracle_solve_one(oracle, s["xref"][b], s["fsteps"][b], None if table is None else table["a"][b], p)

    with ThreadPoolExecutor(max_workers=8) as ex:
        rs = list(ex.map(one, range(B)))
    out = {k: np.stack([np.asarray(r[k]) for r in rs])
           for k in ("f0", "x", "status", "iters", "rho_updates", "admm_status", "Ax", "l", "u")}
    for k in ("status", "iters", "rho_updates", "admm_status"):
        out[k] = out[k].astype(np.int32)
    for v in out.values():
        v.flags.writeable = False
    if key is not None:
        _CACHE[ck] = out
    return out
