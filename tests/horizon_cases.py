"""Fixtures and synthetic batches at every compiled horizon (N = 4 ... 64).

The engine is one code object per horizon; tests/golden/ holds a reference fixture for each:
golden_n16 / golden_n32.npz, the three golden_horizons*.npz that conftest.golden_h loads, and
golden_horizons_rest_a / _b.npz (gen_golden.py horizons_rest) for REST_HORIZONS, the 41 that
the earlier files leave out.  The rest files carry a reduced field set: no Ax_setup / l_setup /
u_setup / y_star.  Used by test_horizons_rest.py (CPU) and test_gpu_every_horizon.py (GPU)."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ALL_HORIZONS = tuple(range(4, 65))
REST_HORIZONS = (7, 9, 11, 14, 15, 17, 18, 19, 21, 22, 23, 25, 26, 27, 29, 30, 31,
                 34, 35, 37, 38, 39, 41, 42, 43, 44, 45, 46, 47,
                 51, 52, 53, 54, 55, 56, 58, 59, 60, 61, 62, 63)

SINGLE_FILES = {16: "golden_n16.npz", 32: "golden_n32.npz"}
HORIZON_FILES = ("golden_horizons.npz", "golden_horizons_r3.npz", "golden_horizons_r4.npz",
                 "golden_horizons_rest_a.npz", "golden_horizons_rest_b.npz")


@functools.lru_cache(maxsize=None)
def _file_horizons(name):
    with np.load(os.path.join(GOLDEN, name)) as d:
        return tuple(int(N) for N in d["horizons"])


def fixture_horizons():
    """Every horizon a committed fixture file holds, one entry per (file, horizon): sorted,
    with repeats if two files hold the same one."""
    out = list(SINGLE_FILES)
    for name in HORIZON_FILES:
        out.extend(_file_horizons(name))
    return tuple(sorted(out))


@functools.lru_cache(maxsize=None)
def golden_for(N):
    """{field: array} of the reference fixture at horizon N, from whichever file holds it."""
    N = int(N)
    if N in SINGLE_FILES:
        with np.load(os.path.join(GOLDEN, SINGLE_FILES[N])) as d:
            return {k: d[k] for k in d.files}
    for name in HORIZON_FILES:
        if N in _file_horizons(name):
            pre = f"n{N}_"
            with np.load(os.path.join(GOLDEN, name)) as d:
                return {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
    raise KeyError(f"no fixture at N = {N}")


def synth_batch(N, seed_base):
    """12 mixed-gait synthetic instances at horizon N."""
    import mpcq
    return mpcq.synth.make_batch(12, N, gaits=mpcq.synth.GAITS, seed=seed_base + N)
