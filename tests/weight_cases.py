"""Per-instance cost weights (mpcq_weights tables) shared by test_weights_host.py (CPU) and
test_gpu_weights.py (GPU).

For horizon N the inputs are ``param_cases.make_batch(N)`` and the weights come from
``np.random.default_rng(900 + N)``, drawn per instance in this order: twelve factors
exp(uniform(-ln 4, ln 4)) on the default state weights, then force = 1e-5 * 10**uniform(-1, 2).
test_weights_host.py shows that the recipe has power on the oracle: every instance solves, its
forces move away from the default weights' and from its neighbour's row's, and the oracle's two
CPU builds agree on status and iteration count -- so a kernel that ignores the table, or reads
another row, cannot pass the GPU comparison, and no instance sits on a rounding knife-edge.

The oracle side is one solve per instance with that instance's Params (the oracle takes one
Params per call); the results are computed once per (N, variant) and never modified.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import param_cases as PC

HORIZONS = PC.HORIZONS
_CACHE = {}


def make_weights(N, B=None):
    """The randomised (B,) table of horizon N (mpcq.WEIGHTS_DTYPE)."""
    import mpcq
    B = PC.batch_size(N) if B is None else B
    d = mpcq.default_params()
    sw0, fw0 = np.array(d.state_weights[:]), d.force_weight
    rng = np.random.default_rng(900 + N)
    sw, fw = np.empty((B, 12)), np.empty(B)
    for b in range(B):
        sw[b] = sw0 * np.exp(rng.uniform(-np.log(4), np.log(4), 12))
        fw[b] = fw0 * 10 ** rng.uniform(-1, 2)
    return mpcq.weights(B, state=sw, force=fw)


def oracle_overrides(row):
    """The oracle Params overrides of one table row."""
    return dict(state_weights=tuple(float(v) for v in row["state"]), force_weight=float(row["force"]))


def oracle_solve(oracle, N, weights=None, robots=None, native=False, key=None, **ov):
    """Per-instance oracle solves of make_batch(N), instance b with weights[b] (None: the default
    weights) and robots[b] (None: the default robot), stacked like oracle.solve_batch's result.
    ``key`` names the variant in the cache."""
    import robot_cases as RC
    ck = (N, key, native, tuple(sorted(ov.items())))
    if key is not None and ck in _CACHE:
        return _CACHE[ck]
    s = PC.make_batch(N)
    B = s["xref"].shape[0]
    if native:
        oracle.native_lib()  # (built once, before the threads ask for it)

    def one(b):
        kw = dict(ov)
        if weights is not None:
            kw.update(oracle_overrides(weights[b]))
        p = oracle.default_params(**kw) if robots is None else RC.oracle_params(oracle, robots[b], **kw)
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
