"""Scenarios: per-episode random commands, pushes and payloads drawn on the device.

``Scenario(engine, params).step(...)`` runs the HIP scenario kernel on its own
(mpcq_scenario_step_batch): for each of ``B`` robots one tick of its episode -- the command
``v_ref`` (a ramp from rest to a drawn target, segment after segment: the reference's
Joystick.update_v_ref_predefined, Joystick.py:82-83, is the default), the push of the tick, and
on a robot's first tick the episode's true mass and friction.  ``Session.enable_scenario`` runs
the same kernel at the head of every tick.  The kernel runs on the device; there is no CPU
fallback for it.

``philox``, ``constants``, ``command``, ``push`` and ``apply_constants`` are the statement of
the device's arithmetic in numpy, vectorised, for users: everything is a pure function of
(params, robot, epoch, tick), every derived value is exact or a single rounding, and they agree
with the kernel bit for bit (include/mpcq.h has the rules).  A sweep uses them to recover which
draw an ended episode had: with auto-reset only, the n-th ended episode of robot ``b``
(``MV_EPISODES``) ran under epoch n.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import _stage as S
from .engine import ROBOT_DTYPE, Engine, _p, _robot_table

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u32(a):
    """Integers (any sign) as 32-bit words in uint64 arrays."""
    return (np.asarray(a).astype(np.int64) & np.int64(0xFFFFFFFF)).astype(np.uint64)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counter words (c0, c1, c2, c3) under the key (k0, k1); the inputs
    broadcast; returns four uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u32(x) for x in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def _key(params):
    seed = int(params.seed)
    return seed & 0xFFFFFFFF, seed >> 32


def u01(wa, wb):
    """53 bits of two words as a double in [0, 1)."""
    return ((wa >> np.uint64(5)).astype(np.float64) * 67108864.0 + (wb >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


def _range(lo, hi, u):
    return np.float64(lo) + (np.float64(hi) - np.float64(lo)) * u


def constants(params, robots, epochs):
    """(mass_scale, mu) the episodes ``epochs`` of ``robots`` drew (the inputs broadcast)."""
    k0, k1 = _key(params)
    w0, w1, w2, w3 = philox(robots, epochs, 0, 0, k0, k1)
    return (_range(params.mass_scale_lo, params.mass_scale_hi, u01(w0, w1)),
            _range(params.mu_lo, params.mu_hi, u01(w2, w3)))


def apply_constants(params, base, mass_scale, mu):
    """The rows of CV_ROBOTS: ``base`` ((B,) ROBOT_DTYPE) with the bits of ``params.robots``
    applied (1: mass and gI times mass_scale; 2: mu replaced)."""
    out = _robot_table(base).copy()
    if params.robots & 1:
        out["mass"] = out["mass"] * mass_scale
        out["gI"] = out["gI"] * np.asarray(mass_scale, np.float64)[..., None, None]
    if params.robots & 2:
        out["mu"] = mu
    return out


def _target(params, robots, epochs, j, k0, k1):
    j = _u32(j)
    w0, w1, w2, w3 = philox(robots, epochs, j * np.uint64(2), 1, k0, k1)
    q0, q1, _, _ = philox(robots, epochs, j * np.uint64(2) + np.uint64(1), 1, k0, k1)
    return np.stack([_range(params.v_lo[0], params.v_hi[0], u01(w0, w1)),
                     _range(params.v_lo[1], params.v_hi[1], u01(w2, w3)),
                     _range(params.v_lo[2], params.v_hi[2], u01(q0, q1))], axis=-1)


def command(params, robots, epochs, ticks):
    """v_ref (..., 6) of the ticks ``ticks`` (0 = the episode's first) of the episodes
    ``epochs`` of ``robots`` (the inputs broadcast); zeros with ``params.commands == 0``."""
    robots, epochs, ticks = np.broadcast_arrays(np.asarray(robots, np.int64), np.asarray(epochs, np.int64),
                                                np.asarray(ticks, np.int64))
    out = np.zeros(ticks.shape + (6,))
    if not params.commands:
        return out
    k0, k1 = _key(params)
    period, start, ramp = int(params.cmd_period), int(params.cmd_start), int(params.cmd_ramp)
    j = ticks // period if period > 0 else np.zeros_like(ticks)
    t = ticks - j * period - np.where(j == 0, start, 0)
    if ramp > 0:
        alpha = np.clip(t.astype(np.float64) / np.float64(ramp), 0.0, 1.0)
    else:
        alpha = np.where(t >= 0, 1.0, 0.0)
    target = _target(params, robots, epochs, j, k0, k1)
    prev = np.where((j > 0)[..., None], _target(params, robots, epochs, np.maximum(j - 1, 0), k0, k1), 0.0)
    a = alpha[..., None]
    v = np.where(a == 1.0, target, np.where(a == 0.0, prev, prev + (target - prev) * a))
    out[..., 0], out[..., 1], out[..., 5] = v[..., 0], v[..., 1], v[..., 2]
    return out


def push(params, robots, epochs, ticks):
    """(push (..., 6), active (...) bool) of the same robot-ticks: the window's wrench while a
    window is active, else zeros."""
    robots, epochs, ticks = np.broadcast_arrays(np.asarray(robots, np.int64), np.asarray(epochs, np.int64),
                                                np.asarray(ticks, np.int64))
    out = np.zeros(ticks.shape + (6,))
    if not params.pushes:
        return out, np.zeros(ticks.shape, bool)
    k0, k1 = _key(params)
    first, period = int(params.push_first), int(params.push_period)
    late = ticks >= first
    j = np.where(late, (ticks - first) // period if period > 0 else 0, 0)
    i0 = _u32(j) * np.uint64(4)
    h0, h1, h2, _ = philox(robots, epochs, i0, 2, k0, k1)
    jitter = ((h0 * np.uint64(int(params.push_jitter) + 1)) >> _S32).astype(np.int64)
    occurs = h1.astype(np.float64) * 2.0 ** -32 < np.float64(params.push_prob)
    s = first + j * period + jitter
    active = late & occurs & (s <= ticks) & (ticks < s + int(params.push_ticks))
    flip = h2 & np.uint64(int(params.push_flip))
    for c in range(3):
        w0, w1, w2, w3 = philox(robots, epochs, i0 + np.uint64(1 + c), 2, k0, k1)
        for i, u in ((2 * c, u01(w0, w1)), (2 * c + 1, u01(w2, w3))):
            x = _range(params.wrench_lo[i], params.wrench_hi[i], u)
            x = np.where((flip >> np.uint64(i)) & np.uint64(1) != 0, -x, x)
            out[..., i] = np.where(active, x, 0.0)
    return out, active


def new_state(B: int) -> dict:
    """What ``Scenario.step`` carries between calls, before a robot's first tick."""
    return dict(epoch=np.zeros(B, np.int32), tick=np.zeros(B, np.int32), robots=np.zeros(B, ROBOT_DTYPE),
                draw=np.zeros((B, 8)))


class Scenario:
    def __init__(self, engine: Engine, params: L.ScenarioParams | None = None):
        self.engine = engine
        self.params = params or L.default_scenario_params()

    # ------------------------------------------------------------------ host arrays
    def step(self, state: dict | None = None, first=None, all_first: bool = False, base=None, wrench_in=None,
             batch: int | None = None, robots_out: bool = True, draw: bool = True):
        """One tick: ``state`` the dict of ``new_state`` (None: new, ``batch`` robots), its
        ``epoch`` and ``tick`` updated in place, its ``robots`` and ``draw`` rewritten for the
        robots on a first tick (``robots_out`` / ``draw`` False: not passed to the kernel);
        ``first`` (B,) nonzero = a first tick, ``all_first`` for every robot; ``base`` a (B,)
        ROBOT_DTYPE table (None: the engine's parameters); ``wrench_in`` broadcasts to (B, 6)
        (None: zeros).  Returns (v_ref (B, 6), push (B, 6), wrench_out (B, 6), state)."""
        if state is None:
            if batch is None:
                raise ValueError("pass state or batch")
            state = new_state(int(batch))
        B = state["epoch"].shape[0]
        want = {"epoch": ((B,), np.int32), "tick": ((B,), np.int32), "robots": ((B,), ROBOT_DTYPE),
                "draw": ((B, 8), np.float64)}
        for name, (shape, dt) in want.items():
            a = state[name]
            if not (isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dt and a.flags.c_contiguous):
                raise ValueError(f"state[{name!r}] must be a contiguous {np.dtype(dt).name} array of shape {shape}")
        f = None if first is None else np.ascontiguousarray(np.broadcast_to(np.asarray(first) != 0, (B,)), np.int32)
        bt = None if base is None else _robot_table(base, B)
        wi = None if wrench_in is None else np.ascontiguousarray(np.broadcast_to(np.asarray(wrench_in, np.float64), (B, 6)))
        v_ref, pu, wo = np.zeros((B, 6)), np.zeros((B, 6)), np.zeros((B, 6))
        self.engine._call("mpcq_scenario_step_batch", self.engine._h, C.byref(self.params), B, _p(f),
                          int(bool(all_first)), _p(state["epoch"]), _p(state["tick"]), _p(bt), _p(wi), _p(v_ref),
                          _p(pu), _p(wo), _p(state["robots"]) if robots_out else None,
                          _p(state["draw"]) if draw else None, 0)
        return v_ref, pu, wo, state

    # ------------------------------------------------------------------ device pointers
    def step_device(self, batch: int, epoch_ptr: int, tick_ptr: int, v_ref_ptr: int, push_ptr: int,
                    wrench_out_ptr: int, first_ptr: int = 0, all_first: bool = False, base_ptr: int = 0,
                    wrench_in_ptr: int = 0, robots_out_ptr: int = 0, draw_ptr: int = 0, asynchronous: bool = True):
        """step on device-resident arrays (pointers on the engine's device; 0 = absent)."""
        v, flags = S.v, S.device_flags(asynchronous)
        self.engine._call("mpcq_scenario_step_batch", self.engine._h, C.byref(self.params), int(batch), v(first_ptr),
                          int(bool(all_first)), v(epoch_ptr), v(tick_ptr), v(base_ptr), v(wrench_in_ptr), v(v_ref_ptr),
                          v(push_ptr), v(wrench_out_ptr), v(robots_out_ptr), v(draw_ptr), flags)
