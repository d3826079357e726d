"""The disturbance observer in front of the solve.

``Disturb(engine, params).step(...)`` runs the HIP disturb kernel on its own
(mpcq_disturb_step_batch): for each of ``B`` robots one tick of an observer that samples the
constant acceleration the controller's model lacks -- (the measurement - the model's step from
the previous measurement under the recorded forces, acting ``f_lag`` ticks late) / dt --, filters
it with gain ``alpha`` and clips it to ``d_max``.  ``Session.enable_disturb`` runs the same kernel
inside every tick, after the estimator and before the planner, and (with ``compensate``) hands
the estimate to the solve as each robot's disturbance row.  The kernel runs on the device; there
is no CPU fallback for it.  include/mpcq.h has the rules.

``unpack`` splits the stage's rows into their named parts.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import _stage as S
from .engine import DISTURBANCE_DTYPE, Engine, _p

F_INIT = np.tile([0.0, 0.0, 8.0], 4)  # the result before any solve (MPC_Wrapper.py:78)


def new_rows(B: int) -> np.ndarray:
    """(B, DIST_ROW) zeros: rows that run a first tick at their first tick."""
    return np.zeros((int(B), L.DIST_ROW))


def unpack(rows) -> dict:
    """Views into rows (..., DIST_ROW): ``d`` (..., 6) the estimate, ``prev`` (..., 12) the previous
    measurement, ``valid`` / ``tau_next`` (...,) int32, ``ring`` (..., 5, 12) the slots' f0."""
    r = np.asarray(rows)
    if r.dtype != np.float64 or r.shape[-1] != L.DIST_ROW or not r.flags.c_contiguous:
        raise ValueError(f"rows must be contiguous float64 (..., {L.DIST_ROW})")
    lead = r.shape[:-1]
    clock = r[..., L.DIST_CLOCK:L.DIST_CLOCK + 2].view(np.int32)
    return dict(d=r[..., L.DIST_D:L.DIST_D + 6], prev=r[..., L.DIST_PREV:L.DIST_PREV + 12], valid=clock[..., 0],
                tau_next=clock[..., 1], ring=r[..., L.DIST_RING:].reshape(lead + (L.DIST_SLOTS, 12)))


class Disturb:
    def __init__(self, engine: Engine, params: L.DisturbParams | None = None):
        self.engine = engine
        self.params = params or L.default_disturb_params()

    def step(self, meas, f_prev, feet_prev, rows=None, first=None, all_first: bool = False, failed_prev=None,
             robots=None):
        """One tick: ``meas`` (B, 12) the measurement, ``f_prev`` (B, 12) and ``feet_prev``
        (B, 3, 4) (NaN = swing) the previous tick's forces and feet, ``rows`` (B, DIST_ROW) the
        stage's state, updated in place (None: new rows), ``first`` / ``failed_prev`` (B,)
        nonzero = a first tick / the previous tick failed, ``robots`` (B,) ROBOT_DTYPE the
        robots the controller believes (None: the engine's parameters).  Returns (dist (B,)
        DISTURBANCE_DTYPE, resid (B, 6), rows)."""
        B, rows, (fi, *ins) = S.model_inputs("meas", meas, f_prev, feet_prev, rows, L.DIST_ROW, first, failed_prev,
                                             robots)
        dist = np.empty(B, DISTURBANCE_DTYPE)
        resid = np.empty((B, 6))
        self.engine._call("mpcq_disturb_step_batch", self.engine._h, C.byref(self.params), B, _p(fi),
                          int(bool(all_first)), *map(_p, ins), _p(dist), _p(resid), 0)
        return dist, resid, rows

    def step_device(self, batch: int, meas_ptr: int, f_prev_ptr: int, feet_prev_ptr: int, row_ptr: int, dist_ptr: int,
                    resid_ptr: int = 0, first_ptr: int = 0, all_first: bool = False, failed_prev_ptr: int = 0,
                    robots_ptr: int = 0, asynchronous: bool = True):
        """step on device-resident arrays (pointers on the engine's device; 0 = absent)."""
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_disturb_step_batch", self.engine._h, C.byref(self.params), int(batch), v(first_ptr),
                          int(bool(all_first)), v(meas_ptr), v(f_prev_ptr), v(feet_prev_ptr), v(failed_prev_ptr),
                          v(robots_ptr), v(row_ptr), v(dist_ptr), v(resid_ptr), flags)
