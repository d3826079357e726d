"""Gait transitions over the HIP gait kernel (mpcq_gait_roll_batch).

``Gait(engine, cycles, ...).roll(gait, state, v_ref)`` is one call of the gait stage for ``B``
robots: the planner's roll of each ``[20][5]`` gait table with the step that enters the horizon
taken from a desired gait cycle (include/mpcq.h has the rules: requests, switches at phase
boundaries, selection by the commanded speed).  ``Session.enable_gait`` runs the same kernel
inside every tick.  ``cycle`` builds the library's entries.  Every method runs on the device;
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import _stage as S
from .engine import Engine, _f64, _p
from .planner import _MASKS

# "pace" is the lateral-pair gait, which the reference calls side walking: the same masks
_CYCLE_MASKS = dict(_MASKS, pace=_MASKS["side"])


def cycle(name: str, dt: float = 0.02, T_gait: float = 0.32) -> np.ndarray:
    """One period of a gait in the gait table's format, (20, 5): "trot", "bound", "pace", "side"
    are [1 all][half - 1 A][1 all][half - 1 B] with half = int(0.5 T_gait / dt) and the masks
    of FootstepPlanner's tables; "stand" is the one-row cycle [1, 1, 1, 1, 1]."""
    g = np.zeros((20, 5))
    if name == "stand":
        g[0] = 1.0
        return g
    if name not in _CYCLE_MASKS:
        raise ValueError(f"unknown gait {name!r}: one of {sorted(_CYCLE_MASKS) + ['stand']}")
    half = int(0.5 * T_gait / dt)
    if half < 2:
        raise ValueError(f"T_gait / dt = {T_gait / dt:g} leaves no swing phase")
    g[:4, 0] = (1, half - 1, 1, half - 1)
    g[:4, 1:] = _CYCLE_MASKS[name]
    return g


def library(cycles) -> np.ndarray:
    """Cycles (names for ``cycle``'s defaults, or (20, 5) arrays) as one (n, 20, 5) array."""
    out = [cycle(c) if isinstance(c, str) else np.asarray(c, np.float64) for c in cycles]
    for c in out:
        if c.shape != (20, 5):
            raise ValueError(f"a gait cycle has shape (20, 5), not {c.shape}")
    if not 1 <= len(out) <= L.GAIT_MAX:
        raise ValueError(f"a gait library holds 1 to {L.GAIT_MAX} cycles, not {len(out)}")
    return np.ascontiguousarray(np.stack(out))


def new_state(B: int) -> np.ndarray:
    """The rows before a robot's first call: (want, active, phase, switches) = (-1, -1, 0, 0)."""
    st = np.zeros((B, 4), np.int32)
    st[:, :2] = -1
    return st


def params_for(cycles: np.ndarray, params: L.GaitParams | None = None, **overrides) -> L.GaitParams:
    """``params`` as it is, or the defaults with ``overrides`` and n_gaits = len(cycles)."""
    if params is not None:
        if overrides:
            raise ValueError("pass params or overrides, not both")
        return params
    overrides.setdefault("n_gaits", len(cycles))
    return L.default_gait_params(**overrides)


class Gait:
    def __init__(self, engine: Engine, cycles, params: L.GaitParams | None = None, **overrides):
        self.engine = engine
        self.cycles = library(cycles)
        self.params = params_for(self.cycles, params, **overrides)

    # ------------------------------------------------------------------ host arrays
    def roll(self, gait, state=None, v_ref=None):
        """One call: gait (B, 20, 5) and state (B, 4) int32 (None: ``new_state``) are updated in
        place (contiguous arrays of the right type; otherwise copies are) and returned; v_ref
        (B, 6) is read with GAIT_BY_SPEED only."""
        gait = _f64(gait)
        B = gait.shape[0]
        gait = _f64(gait, (B, 20, 5))
        state = new_state(B) if state is None else np.ascontiguousarray(state, np.int32)
        if state.shape != (B, 4):
            raise ValueError(f"expected a state of shape {(B, 4)}")
        if v_ref is not None:
            v_ref = np.ascontiguousarray(np.broadcast_to(np.asarray(v_ref, np.float64), (B, 6)))
        self.engine._call("mpcq_gait_roll_batch", self.engine._h, C.byref(self.params), _p(self.cycles), B,
                          _p(v_ref), _p(gait), _p(state), 0)
        return gait, state

    # ------------------------------------------------------------------ device pointers
    def roll_device(self, batch: int, gait_ptr: int, state_ptr: int, v_ref_ptr: int = 0, asynchronous: bool = True):
        """roll on device-resident arrays (pointers on the engine's device; 0 = absent)."""
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_gait_roll_batch", self.engine._h, C.byref(self.params), _p(self.cycles), int(batch),
                          v(v_ref_ptr), v(gait_ptr), v(state_ptr), flags)
