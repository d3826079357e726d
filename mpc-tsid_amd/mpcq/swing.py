"""Batched swing-foot trajectories over the HIP swing kernel (mpcq_swing_batch).

``Swing(engine, batch)`` holds the foot trajectory generators of ``batch`` robots (the
reference keeps four ``Foot_trajectory_generator`` objects, ``mgoals`` and ``t_swing`` per
controller, TSID_Debug_controller_four_legs_fb_vel.py:85-98, 130) as one array
``state [B][4][SWING_STATE]`` and advances them:

  step(args)      one ``get_next_foot`` per (robot, foot) with explicit arguments
  advance(...)    substeps ``k_sub0 .. k_sub0 + n_sub - 1`` of update_footsteps +
                  update_feet_tasks (TSID:247-327, 471-487) from a tick's gait / fsteps

The frame (the reference's ``oMl`` as x, y, yaw) is held for a whole ``advance`` call: one
call per substep follows a frame that moves every substep, as the reference does.  Every
method runs on the device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import _stage as S
from .engine import Engine, _f64, _p


class Swing:
    def __init__(self, engine: Engine, batch: int, params: L.SwingParams | None = None):
        self.engine = engine
        self.batch = int(batch)
        self.params = params or L.default_swing_params()
        self.state = np.zeros((self.batch, 4, L.SWING_STATE))  # all-zero = new generators
        self.status = np.zeros(self.batch, np.int32)
        self.t0 = None

    def reset(self):
        self.state[:] = 0.0

    # ------------------------------------------------------------------ host arrays
    def step(self, args):
        """get_next_foot for every (robot, foot): args (B, 4, 10) = x0, dx0, ddx0, y0, dy0,
        ddy0, x1, y1, t0, t1.  Returns (B, 4, 11), the reference's return list; a foot whose
        t0 is NaN is skipped (NaN outputs, state untouched)."""
        B = self.batch
        a = _f64(args, (B, 4, 10))
        out = np.empty((B, 4, 11))
        self.engine._call("mpcq_swing_step_batch", self.engine._h, C.byref(self.params), B, _p(a),
                          _p(self.state), _p(out), 0)
        return out

    def advance(self, gait, fsteps, frame, k_sub0: int = 0, n_sub: int | None = None, feet0=None):
        """Swing references of substeps k_sub0 .. k_sub0 + n_sub - 1 (n_sub None: up to
        k_mpc): returns ref (B, n_sub, 4, 9) = pos xyz, vel xyz, acc xyz per foot, NaN for
        stance feet.  ``self.t0`` (B, n_sub, 4) and ``self.status`` (B,) hold the call's t0
        and status (STATUS_BAD_GAIT: state unchanged, outputs NaN)."""
        B = self.batch
        n = int(self.params.k_mpc) - int(k_sub0) if n_sub is None else int(n_sub)
        gait = _f64(gait, (B, 20, 5))
        fsteps = _f64(fsteps, (B, 20, 13))
        frame = _f64(frame, (B, 3))
        feet0 = _f64(feet0, (B, 4, 6))
        ref = np.empty((B, max(n, 0), 4, 9))
        t0 = np.empty((B, max(n, 0), 4))
        self.engine._call("mpcq_swing_batch", self.engine._h, C.byref(self.params), B, int(k_sub0), n,
                          _p(gait), _p(fsteps), _p(frame), _p(feet0), _p(self.state), _p(ref), _p(t0),
                          _p(self.status), 0)
        self.t0 = t0
        return ref

    # ------------------------------------------------------------------ device pointers
    def step_device(self, in_ptr: int, state_ptr: int, out_ptr: int, asynchronous: bool = True):
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_swing_step_batch", self.engine._h, C.byref(self.params), self.batch, v(in_ptr),
                          v(state_ptr), v(out_ptr), flags)

    def advance_device(self, gait_ptr: int, fsteps_ptr: int, frame_ptr: int, state_ptr: int, ref_ptr: int,
                       k_sub0: int = 0, n_sub: int | None = None, feet0_ptr: int = 0, t0_ptr: int = 0,
                       status_ptr: int = 0, asynchronous: bool = True):
        """advance on device-resident arrays (pointers on the engine's device); the state is
        the caller's device array, not ``self.state``."""
        n = int(self.params.k_mpc) - int(k_sub0) if n_sub is None else int(n_sub)
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_swing_batch", self.engine._h, C.byref(self.params), self.batch, int(k_sub0), n,
                          v(gait_ptr), v(fsteps_ptr), v(frame_ptr), v(feet0_ptr), v(state_ptr), v(ref_ptr),
                          v(t0_ptr), v(status_ptr), flags)
