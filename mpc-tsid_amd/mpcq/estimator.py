"""The delay-compensating state estimator in front of the planner.

``Estimator(engine, params).step(...)`` runs the HIP estimate kernel on its own
(mpcq_estimator_step_batch): for each of ``B`` robots one tick of a Kalman filter on the MPC's
own discrete model, which keeps its posterior at the time the measurement was taken (``lag``
ticks ago) and predicts forward to now through the forces the MPC commanded (acting ``f_lag``
ticks late) and the footholds it planned.  ``Session.enable_estimator`` runs the same kernel
inside every tick, between the channel's observe stage and the planner.  The kernel runs on the
device; there is no CPU fallback for it.  include/mpcq.h has the rules.

``unpack`` splits filter rows into their named parts.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import _stage as S
from .engine import Engine, _p

F_INIT = np.tile([0.0, 0.0, 8.0], 4)  # the result before any solve (MPC_Wrapper.py:78)


def new_rows(B: int) -> np.ndarray:
    """(B, EST_ROW) zeros: filters that initialise at their first tick."""
    return np.zeros((int(B), L.EST_ROW))


def unpack(rows) -> dict:
    """Views into filter rows (..., EST_ROW): ``post`` (..., 12), ``prev_obs`` (..., 12), ``P``
    (..., 6, 3) the blocks' (p_pp, p_pv, p_vv), ``valid`` / ``s`` / ``tau_next`` (...,) int32,
    ``ring`` (..., 12, 24) the slots' f0 [12] and feet [3][4]."""
    r = np.asarray(rows)
    if r.dtype != np.float64 or r.shape[-1] != L.EST_ROW or not r.flags.c_contiguous:
        raise ValueError(f"rows must be contiguous float64 (..., {L.EST_ROW})")
    lead = r.shape[:-1]
    clock = r[..., L.EST_CLOCK:L.EST_CLOCK + 2].view(np.int32)
    return dict(post=r[..., L.EST_POST:L.EST_POST + 12], prev_obs=r[..., L.EST_PREV:L.EST_PREV + 12],
                P=r[..., L.EST_P:L.EST_P + 18].reshape(lead + (6, 3)), valid=clock[..., 0], s=clock[..., 1],
                tau_next=clock[..., 2], ring=r[..., L.EST_RING:].reshape(lead + (L.EST_SLOTS, 24)))


class Estimator:
    def __init__(self, engine: Engine, params: L.EstimatorParams | None = None):
        self.engine = engine
        self.params = params or L.default_estimator_params()

    def step(self, obs, f_prev, feet_prev, rows=None, first=None, all_first: bool = False, failed_prev=None,
             robots=None):
        """One tick: ``obs`` (B, 12) the measurement, ``f_prev`` (B, 12) and ``feet_prev``
        (B, 3, 4) (NaN = swing) the previous tick's forces and feet, ``rows`` (B, EST_ROW) the
        filter state, updated in place (None: new filters), ``first`` / ``failed_prev`` (B,)
        nonzero = a first tick / the previous tick failed, ``robots`` (B,) ROBOT_DTYPE the
        robots the controller believes (None: the engine's parameters).  Returns (est (B, 12),
        rows)."""
        B, rows, (fi, *ins) = S.model_inputs("obs", obs, f_prev, feet_prev, rows, L.EST_ROW, first, failed_prev,
                                             robots)
        est = np.empty((B, 12))
        self.engine._call("mpcq_estimator_step_batch", self.engine._h, C.byref(self.params), B, _p(fi),
                          int(bool(all_first)), *map(_p, ins), _p(est), 0)
        return est, rows

    def step_device(self, batch: int, obs_ptr: int, f_prev_ptr: int, feet_prev_ptr: int, row_ptr: int, est_ptr: int,
                    first_ptr: int = 0, all_first: bool = False, failed_prev_ptr: int = 0, robots_ptr: int = 0,
                    asynchronous: bool = True):
        """step on device-resident arrays (pointers on the engine's device; 0 = absent)."""
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_estimator_step_batch", self.engine._h, C.byref(self.params), int(batch), v(first_ptr),
                          int(bool(all_first)), v(obs_ptr), v(f_prev_ptr), v(feet_prev_ptr), v(failed_prev_ptr),
                          v(robots_ptr), v(row_ptr), v(est_ptr), flags)
