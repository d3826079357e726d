"""Batched rigid-body plant over the HIP plant kernel (mpcq_plant_step_batch).

``Plant(engine, params).step(state, feet, f)`` advances ``B`` single rigid bodies by one MPC
tick under the forces ``f`` of their stance feet: the object the MPC is a discretisation of,
with constants of its own (``robots``: a table of true robots, ``mpcq.robots()``) and an
external wrench.  ``PLANT_MODEL`` is the MPC's own discrete step, ``PLANT_RIGID`` ``n_sub``
semi-implicit Euler substeps of the full rotational dynamics (include/mpcq.h has the
equations).  ``Session.enable_plant`` runs the same kernel inside every tick.  Every method
runs on the device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import _stage as S
from .engine import Engine, _f64, _p, _robot_table


class Plant:
    def __init__(self, engine: Engine, params: L.PlantParams | None = None):
        self.engine = engine
        self.params = params or L.default_plant_params(dt=engine.params.dt)

    # ------------------------------------------------------------------ host arrays
    def step(self, state, feet, f, wrench=None, robots=None):
        """One tick: state (B, 12) = c, rpy, v, w; feet (B, 3, 4) laid out as l_feet, NaN = a
        swing foot; f (B, 12) foot-major as f_applied; wrench (B, 6) or None: force, then
        torque about the centre of mass; robots (B,) ROBOT_DTYPE or None (the engine's
        parameters) -- all in one inertial frame.  Returns (state_out (B, 12), f_eff (B, 12):
        the forces the plant applied)."""
        state = _f64(state)
        B = state.shape[0]
        state = _f64(state, (B, 12))
        feet = _f64(feet, (B, 3, 4))
        f = _f64(f, (B, 12))
        wrench = _f64(wrench, (B, 6))
        t = None if robots is None else _robot_table(robots, B)
        out = np.empty((B, 12))
        f_eff = np.empty((B, 12))
        self.engine._call("mpcq_plant_step_batch", self.engine._h, C.byref(self.params), B, _p(state), _p(feet),
                          _p(f), _p(wrench), _p(t), _p(out), _p(f_eff), 0)
        return out, f_eff

    # ------------------------------------------------------------------ device pointers
    def step_device(self, batch: int, state_ptr: int, feet_ptr: int, f_ptr: int, state_out_ptr: int,
                    f_eff_ptr: int = 0, wrench_ptr: int = 0, robots_ptr: int = 0, asynchronous: bool = True):
        """step on device-resident arrays (pointers on the engine's device; 0 = absent);
        ``state_out_ptr`` may be ``state_ptr``.  A device robots table is not validated."""
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_plant_step_batch", self.engine._h, C.byref(self.params), int(batch), v(state_ptr),
                          v(feet_ptr), v(f_ptr), v(wrench_ptr), v(robots_ptr), v(state_out_ptr), v(f_eff_ptr), flags)
