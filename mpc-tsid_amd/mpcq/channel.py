"""The channel between plant and controller: noisy, delayed state feedback and delayed forces.

``Channel(engine, params).observe(...)`` / ``.actuate(...)`` run the two HIP channel kernels on
their own (mpcq_channel_observe_batch / mpcq_channel_actuate_batch): for each of ``B`` robots the
observation the planner gets of the true state (``delay`` ticks late, plus a per-episode bias and
per-tick noise, or the previous observation again on a dropped frame) and the forces the plant
gets of the solve's (``latency`` ticks late -- one tick is the reference's asynchronous mode,
MPC_Wrapper.py:57-78 --, times a per-episode leg gain, plus per-tick noise).
``Session.enable_channel`` runs the same kernels inside every tick.  The kernels run on the
device; there is no CPU fallback for them.

``normal``, ``bias``, ``gain`` and ``held`` are the statement of the device's draws in numpy,
vectorised, for users: each is a pure function of (params, robot, epoch, tau), exact or a single
rounding, and agrees with the kernels bit for bit (include/mpcq.h has the rules).  They reuse
``mpcq.scenario.philox`` under the channel's own seed and streams.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import _stage as S
from .engine import Engine, _p
from .scenario import _key, philox, u01

STREAM_NOISE, STREAM_HOLD, STREAM_FORCE, STREAM_BIAS, STREAM_GAIN = 0x100, 0x110, 0x120, 0x200, 0x210
F_INIT = np.tile([0.0, 0.0, 8.0], 4)  # the result before any solve (MPC_Wrapper.py:78)
_CENTRE = np.int64(8589934590)         # the mean of the sum of four words
_SCALE = np.float64(1.7320508075688772) * 2.0 ** -32


def _normal(w):
    """n(w): the centred sum of the four words at unit variance, |n| <= 2 sqrt(3)."""
    s = (w[0] + w[1] + w[2] + w[3]).astype(np.int64) - _CENTRE
    return s.astype(np.float64) * _SCALE


def _sym(w):
    """sym(w) = 2 u(w0, w1) - 1 in [-1, 1), exact."""
    return 2.0 * u01(w[0], w[1]) - 1.0


def normal(params, robots, epochs, ticks, stream):
    """The unit draw n of ``stream`` (STREAM_NOISE + i for state component i, STREAM_FORCE + j
    for force component j) at the ticks ``ticks`` of the episodes ``epochs`` of ``robots`` (the
    inputs broadcast)."""
    k0, k1 = _key(params)
    return _normal(philox(robots, epochs, ticks, stream, k0, k1))


def bias(params, robots, epochs):
    """(..., 12): the bias the episodes ``epochs`` of ``robots`` drew, ``bias[i] * sym``."""
    k0, k1 = _key(params)
    r, e = np.broadcast_arrays(np.asarray(robots, np.int64), np.asarray(epochs, np.int64))
    amp = np.array(params.bias[:], np.float64)
    return amp * _sym(philox(r[..., None], e[..., None], 0, STREAM_BIAS + np.arange(12), k0, k1))


def gain(params, robots, epochs):
    """(..., 4): the leg gains of those episodes, ``1 + f_gain * sym``."""
    k0, k1 = _key(params)
    r, e = np.broadcast_arrays(np.asarray(robots, np.int64), np.asarray(epochs, np.int64))
    return 1.0 + np.float64(params.f_gain) * _sym(philox(r[..., None], e[..., None], 0, STREAM_GAIN + np.arange(4), k0, k1))


def held(params, robots, epochs, ticks):
    """bool: the hold decision of those robot-ticks (a tick that is first or priming never
    holds, whatever this says)."""
    k0, k1 = _key(params)
    _, w1, _, _ = philox(robots, epochs, ticks, STREAM_HOLD, k0, k1)
    return w1.astype(np.float64) * 2.0 ** -32 < np.float64(params.hold_prob)


def new_state(B: int) -> dict:
    """What ``Channel`` carries between calls: the six arrays of a session's channel (HV_*) as
    a first enable leaves them -- zero, every robot waiting to be primed."""
    clock = np.zeros((B, 2), np.int32)
    clock[:, 1] = -1
    return dict(clock=clock, obs=np.zeros((B, 12)), f_cmd=np.zeros((B, 12)), draw=np.zeros((B, 16)),
                s_ring=np.zeros((B, L.CHANNEL_MAX_DELAY, 12)), f_ring=np.zeros((B, L.CHANNEL_MAX_LATENCY, 12)))


_WANT = {"clock": ((2,), np.int32), "obs": ((12,), np.float64), "f_cmd": ((12,), np.float64),
         "draw": ((16,), np.float64), "s_ring": ((L.CHANNEL_MAX_DELAY, 12), np.float64),
         "f_ring": ((L.CHANNEL_MAX_LATENCY, 12), np.float64)}


def _check(state: dict) -> int:
    B = state["clock"].shape[0]
    for name, (tail, dt) in _WANT.items():
        a = state[name]
        if not (isinstance(a, np.ndarray) and a.shape == (B,) + tail and a.dtype == dt and a.flags.c_contiguous):
            raise ValueError(f"state[{name!r}] must be a contiguous {np.dtype(dt).name} array of shape {(B,) + tail}")
    return B


class Channel:
    def __init__(self, engine: Engine, params: L.ChannelParams | None = None):
        self.engine = engine
        self.params = params or L.default_channel_params()

    # ------------------------------------------------------------------ host arrays
    def observe(self, truth, state: dict | None = None, first=None, all_first: bool = False):
        """The observe stage of one tick: ``truth`` (B, 12); ``state`` the dict of ``new_state``
        (None: new), its ``clock``, ``obs``, ``draw``, ``s_ring`` and ``f_ring`` updated in
        place; ``first`` (B,) nonzero = a first tick, ``all_first`` for every robot.  Returns
        (obs (B, 12), state)."""
        truth = np.ascontiguousarray(truth, np.float64)
        if truth.ndim != 2 or truth.shape[1] != 12:
            raise ValueError("truth must be (B, 12)")
        if state is None:
            state = new_state(truth.shape[0])
        B = _check(state)
        if truth.shape[0] != B:
            raise ValueError(f"truth has {truth.shape[0]} rows, the state {B}")
        f = None if first is None else np.ascontiguousarray(np.broadcast_to(np.asarray(first) != 0, (B,)), np.int32)
        self.engine._call("mpcq_channel_observe_batch", self.engine._h, C.byref(self.params), B, _p(f),
                          int(bool(all_first)), _p(truth), _p(state["clock"]), _p(state["obs"]), _p(state["draw"]),
                          _p(state["s_ring"]), _p(state["f_ring"]), 0)
        return state["obs"].copy(), state

    def actuate(self, f0, state: dict):
        """The actuate stage of the same tick, after ``observe``: ``f0`` (B, 12) the tick's
        forces; ``state``'s ``f_ring``, ``f_cmd`` and the pending mark in ``draw`` updated in
        place.  Returns (f_cmd (B, 12), state)."""
        B = _check(state)
        f0 = np.ascontiguousarray(f0, np.float64)
        if f0.shape != (B, 12):
            raise ValueError(f"f0 must be ({B}, 12)")
        self.engine._call("mpcq_channel_actuate_batch", self.engine._h, C.byref(self.params), B, _p(f0),
                          _p(state["clock"]), _p(state["draw"]), _p(state["f_ring"]), _p(state["f_cmd"]), 0)
        return state["f_cmd"].copy(), state

    # ------------------------------------------------------------------ device pointers
    def observe_device(self, batch: int, truth_ptr: int, clock_ptr: int, obs_ptr: int, draw_ptr: int, s_ring_ptr: int,
                       f_ring_ptr: int, first_ptr: int = 0, all_first: bool = False, asynchronous: bool = True):
        """observe on device-resident arrays (pointers on the engine's device; 0 = absent)."""
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_channel_observe_batch", self.engine._h, C.byref(self.params), int(batch), v(first_ptr),
                          int(bool(all_first)), v(truth_ptr), v(clock_ptr), v(obs_ptr), v(draw_ptr), v(s_ring_ptr),
                          v(f_ring_ptr), flags)

    def actuate_device(self, batch: int, f0_ptr: int, clock_ptr: int, draw_ptr: int, f_ring_ptr: int, f_cmd_ptr: int,
                       asynchronous: bool = True):
        """actuate on device-resident arrays."""
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_channel_actuate_batch", self.engine._h, C.byref(self.params), int(batch), v(f0_ptr),
                          v(clock_ptr), v(draw_ptr), v(f_ring_ptr), v(f_cmd_ptr), flags)
