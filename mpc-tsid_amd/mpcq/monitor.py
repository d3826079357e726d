"""Batched episode monitor over the HIP monitor kernel (mpcq_monitor_step_batch).

``Monitor(engine, params).step(...)`` looks at what one tick left of ``B`` robots and decides
per robot whether its episode ended (``DONE_*`` bits: a non-finite pose, tilt, height, a failed
solve, a tick limit), keeps the running episode's accumulators, and counts batch totals
(include/mpcq.h has the rules).  ``Session.enable_monitor`` runs the same kernel inside every
tick.  Every method runs on the device; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import _stage as S
from .engine import Engine, _f64, _p


def new_state(B: int) -> dict:
    """The accumulators before a robot's first tick, as ``Monitor.step`` carries them."""
    ep = np.zeros((B, 8))
    ep[:, 4] = np.inf
    return dict(ep=ep, ep_ticks=np.zeros(B, np.int32), episodes=np.zeros(B, np.int32),
                last=np.zeros((B, 16)), totals=np.zeros(8, np.uint64))


class Monitor:
    def __init__(self, engine: Engine, params: L.MonitorParams | None = None):
        self.engine = engine
        self.params = params or L.default_monitor_params()

    # ------------------------------------------------------------------ host arrays
    def step(self, q_w, status, iters, f0, cost, state, v_ref, acc: dict | None = None, trace: bool = True):
        """One tick: q_w (B, 6), status (B,), iters (B,), f0 (B, 12), cost (B, 13), state
        (B, 12), v_ref (B, 6) as a session's tick leaves them; ``acc`` the accumulators of
        ``new_state`` (None: a first tick), updated in place.  Returns (done (B,) int32, acc,
        trace (B, TRACE) or None)."""
        q_w = _f64(q_w)
        B = q_w.shape[0]
        q_w = _f64(q_w, (B, 6))
        f0 = _f64(f0, (B, 12))
        cost = _f64(cost, (B, 13))
        state = _f64(state, (B, 12))
        v_ref = np.ascontiguousarray(np.broadcast_to(np.asarray(v_ref, np.float64), (B, 6)))
        status = np.ascontiguousarray(status, np.int32)
        iters = np.ascontiguousarray(iters, np.int32)
        if status.shape != (B,) or iters.shape != (B,):
            raise ValueError(f"expected status and iters of shape {(B,)}")
        acc = new_state(B) if acc is None else acc
        want = {"ep": ((B, 8), np.float64), "ep_ticks": ((B,), np.int32), "episodes": ((B,), np.int32),
                "last": ((B, 16), np.float64), "totals": ((8,), np.uint64)}
        for name, (shape, dt) in want.items():
            a = acc[name]
            if not (isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dt and a.flags.c_contiguous):
                raise ValueError(f"acc[{name!r}] must be a contiguous {np.dtype(dt).name} array of shape {shape}")
        done = np.zeros(B, np.int32)
        tr = np.zeros((B, L.TRACE)) if trace else None
        self.engine._call("mpcq_monitor_step_batch", self.engine._h, C.byref(self.params), B, _p(q_w), _p(status),
                          _p(iters), _p(f0), _p(cost), _p(state), _p(v_ref), _p(acc["ep"]), _p(acc["ep_ticks"]),
                          _p(acc["episodes"]), _p(acc["last"]), _p(done), _p(acc["totals"]), _p(tr), 0)
        return done, acc, tr

    # ------------------------------------------------------------------ device pointers
    def step_device(self, batch: int, q_w_ptr: int, status_ptr: int, iters_ptr: int, f0_ptr: int, cost_ptr: int,
                    state_ptr: int, v_ref_ptr: int, ep_ptr: int, ep_ticks_ptr: int, done_ptr: int,
                    episodes_ptr: int = 0, last_ptr: int = 0, totals_ptr: int = 0, trace_ptr: int = 0,
                    asynchronous: bool = True):
        """step on device-resident arrays (pointers on the engine's device; 0 = absent)."""
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_monitor_step_batch", self.engine._h, C.byref(self.params), int(batch), v(q_w_ptr),
                          v(status_ptr), v(iters_ptr), v(f0_ptr), v(cost_ptr), v(state_ptr), v(v_ref_ptr), v(ep_ptr),
                          v(ep_ticks_ptr), v(episodes_ptr), v(last_ptr), v(done_ptr), v(totals_ptr), v(trace_ptr),
                          flags)
