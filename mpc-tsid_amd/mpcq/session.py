"""Closed-loop sessions: B robots whose whole per-tick MPC state stays in HBM.

``Session(engine, batch)`` wraps ``mpcq_session_*`` (include/mpcq.h).  A tick
is the reference's once-per-tick sequence for every robot —
FootstepPlanner.update_fsteps + getRefStates (processing.py:80-131), MPC.run
(MPC.py:460-514) with osqp's warm start carried over (shifted x, y, rho;
MPC.py:403-406), retrieve_result, the world pose q_w and the Logger's cost
components (Logger.py:406-418) — as three launches on the engine's stream.

Passing ``state=None`` / ``l_feet=None`` runs the virtual robot: the next
state is the previous tick's prediction x_robot[:, 0] re-expressed in the new
local frame (processing.py:33-38 is the reference's precedent).  With
``enable_plant`` the next state is instead where a rigid body with constants of
its own (``set_plant_robots``) and an external wrench (``set_wrench``) ends the
tick under the forces the MPC applied: a robot that can disagree with the model.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _lib as L
from .engine import (DISTURBANCE_DTYPE, ROBOT_DTYPE, WEIGHTS_DTYPE, Engine, _disturbance_table, _robot_table,
                     _weights_table)


def _shapes(B, N):
    return {
        L.SV_F0: ((B, 12), np.float64), L.SV_X: ((B, 24 * N), np.float64),
        L.SV_X_ROBOT: ((B, 12, N), np.float64), L.SV_Q_W: ((B, 6), np.float64),
        L.SV_COST: ((B, 13), np.float64), L.SV_XREF: ((B, 12, N + 1), np.float64),
        L.SV_FSTEPS: ((B, 20, 13), np.float64), L.SV_GAIT: ((B, 20, 5), np.float64),
        L.SV_STATUS: ((B,), np.int32), L.SV_ITERS: ((B,), np.int32), L.SV_RHO: ((B,), np.float64),
        L.SV_Y: ((B, 44 * N), np.float64), L.SV_STATE: ((B, 12), np.float64),
        L.SV_L_FEET: ((B, 3, 4), np.float64), L.SV_ROT_FLAG: ((B,), np.int32), L.SV_H_ROT: ((B,), np.float64),
        L.SV_ORDER: ((B,), np.int32), L.SV_FIRST: ((B,), np.int32),
    }


# The arrays of the opt-in groups: kind -> {array id: (shape from B, dtype)}.
_GROUPS = {
    "plant": {L.PV_STATE_END: (lambda B: (B, 12), np.float64), L.PV_F_EFF: (lambda B: (B, 12), np.float64),
              L.PV_WRENCH: (lambda B: (B, 6), np.float64)},
    "monitor": {L.MV_DONE: (lambda B: (B,), np.int32), L.MV_EP: (lambda B: (B, 8), np.float64),
                L.MV_EP_TICKS: (lambda B: (B,), np.int32), L.MV_EPISODES: (lambda B: (B,), np.int32),
                L.MV_LAST: (lambda B: (B, 16), np.float64), L.MV_TOTALS: (lambda B: (8,), np.uint64)},
    "scenario": {L.CV_EPOCH: (lambda B: (B,), np.int32), L.CV_TICK: (lambda B: (B,), np.int32),
                 L.CV_V_REF: (lambda B: (B, 6), np.float64), L.CV_PUSH: (lambda B: (B, 6), np.float64),
                 L.CV_WRENCH: (lambda B: (B, 6), np.float64), L.CV_ROBOTS: (lambda B: (B,), ROBOT_DTYPE),
                 L.CV_DRAW: (lambda B: (B, 8), np.float64)},
    "channel": {L.HV_CLOCK: (lambda B: (B, 2), np.int32), L.HV_OBS: (lambda B: (B, 12), np.float64),
                L.HV_F_CMD: (lambda B: (B, 12), np.float64), L.HV_DRAW: (lambda B: (B, 16), np.float64),
                L.HV_S_RING: (lambda B: (B, L.CHANNEL_MAX_DELAY, 12), np.float64),
                L.HV_F_RING: (lambda B: (B, L.CHANNEL_MAX_LATENCY, 12), np.float64)},
    "estimator": {L.EV_EST: (lambda B: (B, 12), np.float64), L.EV_ROW: (lambda B: (B, L.EST_ROW), np.float64)},
    "disturb": {L.DV_DIST: (lambda B: (B,), DISTURBANCE_DTYPE), L.DV_ROW: (lambda B: (B, L.DIST_ROW), np.float64),
                L.DV_RESID: (lambda B: (B, 6), np.float64)},
    "gait": {L.GV_STATE: (lambda B: (B, 4), np.int32)},
}


class Snapshot:
    """A device-resident copy of a session's robots (``Session.snapshot``): every per-robot array
    of every group the session holds, and ``Session.k`` at the save.  It belongs to the
    session's engine and may be restored into any session on it with the same groups enabled.
    A context manager: leaving it frees the device memory."""

    def __init__(self, session: "Session"):
        self.engine = session.engine
        self.session = session
        self.k = 0
        self.batch = 0
        h = C.c_void_p()
        self.engine._call("mpcq_session_snapshot_create", session._h, C.byref(h))
        self._h = h
        live = getattr(self.engine, "_snapshots", None)
        if live is not None:
            live.add(self)  # Engine.close frees it first

    def save(self):
        """Capture the session again, as it stands now (behind every queued tick)."""
        self.engine._call("mpcq_session_snapshot_save", self.session._h, self._h, 0)
        self.k = self.session.k
        self.batch = self.session.batch
        return self

    def nbytes(self) -> int:
        n = C.c_int64()
        self.engine._call("mpcq_session_snapshot_bytes", self._h, C.byref(n))
        return int(n.value)

    def tobytes(self) -> bytes:
        """The snapshot as one blob on the host (``Session.snapshot_from`` reads it back);
        ``Snapshot.k`` travels in the header's caller field."""
        buf = bytearray(self.nbytes())
        addr = C.addressof((C.c_char * len(buf)).from_buffer(buf))
        self.engine._call("mpcq_session_snapshot_export", self._h, C.c_void_p(addr), len(buf))
        struct.pack_into("<q", buf, L.SNAPSHOT_USER_OFFSET, int(self.k))
        return bytes(buf)

    def close(self):
        if getattr(self, "_h", None):
            # the native destroy needs the context: Engine.close closes its live snapshots first,
            # and one that outlives the engine all the same is only forgotten
            if getattr(self.engine, "_h", True):
                L.lib().mpcq_session_snapshot_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Session:
    """B robots in closed loop on one engine (device, horizon)."""

    def __init__(self, engine: Engine, batch: int, gait0=None, planner_params: L.PlannerParams | None = None):
        self.engine = engine
        self.batch = int(batch)
        self.n_steps = engine.n_steps
        self.planner_params = planner_params or L.default_planner_params(dt=engine.params.dt)
        self._shapes = _shapes(self.batch, self.n_steps)
        g = None
        if gait0 is not None:
            g = np.ascontiguousarray(np.broadcast_to(np.asarray(gait0, np.float64), (self.batch, 20, 5)))
        h = C.c_void_p()
        self.engine._call("mpcq_session_create", engine._h, self.batch, C.byref(self.planner_params),
                                            None if g is None else C.c_void_p(g.ctypes.data), C.byref(h))
        self._h = h
        self.k = 0
        self.swing_params = None
        self.plant_params = None
        self.monitor_params = None
        self.scenario_params = None
        self.channel_params = None
        self.estimator_params = None
        self.disturb_params = None
        self.gait_params = None
        self.gait_cycles = None

    # ------------------------------------------------------------------ the groups' arrays
    def _group_shape(self, kind: str, what: int):
        """(shape, dtype) of array ``what`` of a group; "session": the main group."""
        if kind == "session":
            if what not in self._shapes and what in (L.SV_SWING_REF, L.SV_SWING_STATE, L.SV_FRAME):
                raise L.MpcqError(L.E_INVALID, f"session array {what} needs enable_swing()")
            return self._shapes[what]
        if what not in _GROUPS[kind]:
            raise L.MpcqError(L.E_INVALID, f"unknown {kind} array {what}")
        shape, dt = _GROUPS[kind][what]
        return shape(self.batch), dt

    @staticmethod
    def _entry(kind: str, call: str) -> str:
        return f"mpcq_session_{call}" if kind == "session" else f"mpcq_session_{kind}_{call}"

    def _group_read(self, kind: str, what: int):
        out = np.empty(*self._group_shape(kind, what))
        self.engine._call(self._entry(kind, "read"), self._h, what, C.c_void_p(out.ctypes.data), 0)
        return out

    def _group_ptr(self, kind: str, what: int) -> int:
        out = C.c_void_p()
        self.engine._call(self._entry(kind, "device_ptr"), self._h, what, C.byref(out))
        return int(out.value or 0)

    def _enable(self, kind: str, params, overrides, *more):
        """``params``, or the group's defaults with ``overrides``, into mpcq_session_enable_<kind>
        (``more``: its further arguments) and, once the library has taken them, ``<kind>_params``."""
        if params is not None and overrides:
            raise ValueError("pass params or overrides, not both")
        p = params or getattr(L, f"default_{kind}_params")(**overrides)
        self.engine._call(f"mpcq_session_enable_{kind}", self._h, C.byref(p), *more)
        setattr(self, f"{kind}_params", p)

    def _disable(self, kind: str):
        self.engine._call(f"mpcq_session_disable_{kind}", self._h)
        setattr(self, f"{kind}_params", None)

    def enable_swing(self, params: L.SwingParams | None = None):
        """Opt in to the swing-foot references: every later tick appends one swing launch over
        substeps 0..k_mpc-1 of its gait / fsteps (SV_SWING_REF, SV_SWING_STATE, SV_FRAME)."""
        sp = params or L.default_swing_params()
        self.engine._call("mpcq_session_enable_swing", self._h, C.byref(sp))
        self.swing_params = sp
        B = self.batch
        self._shapes.update({
            L.SV_SWING_REF: ((B, int(sp.k_mpc), 4, 9), np.float64),
            L.SV_SWING_STATE: ((B, 4, L.SWING_STATE), np.float64),
            L.SV_FRAME: ((B, 3), np.float64),
        })

    def set_robots(self, table):
        """The session's own per-robot mass, gI, mu, fz_max (``mpcq.robots(B, ...)``), used from
        the next tick on; independent of the engine's table.  None clears it."""
        t = None if table is None else _robot_table(table, self.batch)
        self.engine._call("mpcq_session_set_robots", self._h, None if t is None else C.c_void_p(t.ctypes.data), 0)

    def set_weights(self, table):
        """The session's own per-robot cost weights (``mpcq.weights(B, ...)``), used from the next
        tick on by the solve and by SV_COST; None clears them.  The table is the controller's
        tuning: it persists across ``reset``, and no snapshot, ``restore`` or ``fork`` touches it
        (``fork(r)`` then ``set_weights(table)`` is a tuning sweep from one state)."""
        t = None if table is None else _weights_table(table, self.batch)
        self.engine._call("mpcq_session_set_weights", self._h, None if t is None else C.c_void_p(t.ctypes.data), 0)

    def get_weights(self):
        """The weights table in force, (B,) WEIGHTS_DTYPE (without one: the engine's parameters)."""
        out = np.zeros(self.batch, WEIGHTS_DTYPE)
        self.engine._call("mpcq_session_get_weights", self._h, C.c_void_p(out.ctypes.data), 0)
        return out

    def set_disturbance(self, table):
        """The session's own per-robot constant disturbance accelerations
        (``mpcq.disturbances(B, ...)``), in each tick's local frame, carried by the model of every
        solve from the next tick on; None clears them.  Like the weights the table is the
        controller's: it persists across ``reset``, and no snapshot, ``restore`` or ``fork`` touches it."""
        t = None if table is None else _disturbance_table(table, self.batch)
        self.engine._call("mpcq_session_set_disturbance", self._h, None if t is None else C.c_void_p(t.ctypes.data), 0)

    def get_disturbance(self):
        """The disturbance table in force, (B,) DISTURBANCE_DTYPE (without one: zeros)."""
        out = np.zeros(self.batch, DISTURBANCE_DTYPE)
        self.engine._call("mpcq_session_get_disturbance", self._h, C.c_void_p(out.ctypes.data), 0)
        return out

    def get_robots(self):
        """The table in force, (B,) ROBOT_DTYPE (without one: the engine's parameters)."""
        out = np.zeros(self.batch, ROBOT_DTYPE)
        self.engine._call("mpcq_session_get_robots", self._h, C.c_void_p(out.ctypes.data), 0)
        return out

    # ------------------------------------------------------------------ rigid-body plant
    def enable_plant(self, params: L.PlantParams | None = None):
        """Opt in to the rigid-body plant: every later tick integrates, directly after its
        retrieve, the state its planner read under SV_F0, the wrench and the plant's robots,
        and SV_Q_W / SV_STATE / SV_L_FEET follow the plant's end state instead of the MPC's
        prediction (``plant_read``: PV_STATE_END, PV_F_EFF, PV_WRENCH).  ``params`` None: the
        defaults with the engine's dt.  Calling it again replaces the parameters."""
        self._enable("plant", params, {} if params else dict(dt=self.engine.params.dt))

    def disable_plant(self):
        """The ticks after it run without the plant; the wrench and the plant's table stay."""
        self._disable("plant")

    def set_plant_robots(self, table):
        """The true robots the plant moves (``mpcq.robots(B, ...)``, or one entry for every
        robot), distinct from the model's table of ``set_robots``.  None clears it: the plant
        then uses the model's table, or without one the engine's parameters."""
        t = None
        if table is not None:
            t = _robot_table(table)
            if t.shape[0] == 1:
                t = np.ascontiguousarray(np.broadcast_to(t, (self.batch,)))
            t = _robot_table(t, self.batch)
        self.engine._call("mpcq_session_set_plant_robots", self._h, None if t is None else C.c_void_p(t.ctypes.data), 0)

    def set_wrench(self, w):
        """The external wrench on every robot: ``w`` broadcasts to (B, 6) = force, then torque
        about the centre of mass, in the WORLD frame.  None: zero.  It persists until changed,
        across ``reset`` too."""
        a = self._in(w, (self.batch, 6))
        self.engine._call("mpcq_session_set_wrench", self._h, None if a is None else C.c_void_p(a.ctypes.data), 0)

    def set_wrench_device(self, ptr: int, asynchronous: bool = True):
        """``set_wrench`` from a device array (B, 6) (0: zero), copied on the engine's stream."""
        flags = L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
        self.engine._call("mpcq_session_set_wrench", self._h, C.c_void_p(ptr) if ptr else None, flags)

    def plant_read(self, what: int):
        """PV_STATE_END (B, 12), PV_F_EFF (B, 12) or PV_WRENCH (B, 6)."""
        return self._group_read("plant", what)

    def plant_device_ptr(self, what: int) -> int:
        return self._group_ptr("plant", what)

    # ------------------------------------------------------------------ episode monitor
    def enable_monitor(self, params: L.MonitorParams | None = None, **overrides):
        """Opt in to episodes: every later tick runs the monitor directly after its plant launch
        (without a plant: after its retrieve): MV_DONE holds the tick's done bits (``DONE_*``), a
        device mask ``reset_device`` takes; MV_EP / MV_EP_TICKS the running episode, MV_LAST the
        last ended one, MV_EPISODES and MV_TOTALS the counts.  With ``auto_reset=1`` the tick
        itself restarts the robots whose episode ended.  ``params`` None: the defaults, with
        ``overrides`` (``max_tilt``, ``min_height``, ``max_ticks``, ``auto_reset``).  Calling it
        again replaces the parameters and keeps the arrays."""
        self._enable("monitor", params, overrides)

    def disable_monitor(self):
        """The ticks after it run without the monitor and its auto-reset; the arrays stay."""
        self._disable("monitor")

    def monitor_read(self, what: int):
        """MV_DONE (B,) int32, MV_EP (B, 8), MV_EP_TICKS (B,) int32, MV_EPISODES (B,) int32,
        MV_LAST (B, 16) or MV_TOTALS (8,) uint64."""
        return self._group_read("monitor", what)

    def monitor_device_ptr(self, what: int) -> int:
        return self._group_ptr("monitor", what)

    # ------------------------------------------------------------------ scenarios
    def enable_scenario(self, params: L.ScenarioParams | None = None, **overrides):
        """Opt in to scenarios: every later tick starts with the scenario launch, which gives
        each robot, for each of its episodes, a command profile relative to the episode's start
        (CV_V_REF: with ``commands`` set, ``tick`` / ``run`` take ``v_ref=None``), push windows
        on top of ``set_wrench`` (CV_PUSH, CV_WRENCH) and its own true mass and friction
        (CV_ROBOTS, CV_DRAW), all reproducible on the host from (seed, robot, epoch) with
        ``mpcq.scenario``; pushes and robots act through ``enable_plant``.  ``params`` None: the
        defaults (the reference's predefined joystick), with ``overrides``.  Calling it again
        replaces the parameters and keeps the arrays."""
        self._enable("scenario", params, overrides)

    def disable_scenario(self):
        """The ticks after it run without the scenario launch: the plant is back on the user's
        wrench and tables, ``v_ref=None`` is an error again; the arrays stay."""
        self._disable("scenario")

    def scenario_read(self, what: int):
        """CV_EPOCH (B,) int32, CV_TICK (B,) int32, CV_V_REF / CV_PUSH / CV_WRENCH (B, 6),
        CV_ROBOTS (B,) ROBOT_DTYPE or CV_DRAW (B, 8)."""
        return self._group_read("scenario", what)

    def scenario_device_ptr(self, what: int) -> int:
        return self._group_ptr("scenario", what)

    # ------------------------------------------------------------------ channel
    def enable_channel(self, params: L.ChannelParams | None = None, **overrides):
        """Opt in to the channel between plant and controller: every later tick observes the
        state it would have handed the planner through a measurement model (``delay`` ticks
        late, a per-episode ``bias``, per-tick noise ``sigma``, frames dropped with
        ``hold_prob``; HV_OBS is what the planner sees, the plant keeps the truth) and, with a
        plant, hands it the forces through an actuation model (``latency`` ticks late, a
        per-episode leg gain ``f_gain``, per-tick noise ``f_sigma``; HV_F_CMD).  Every draw is
        reproducible on the host from (seed, robot, epoch, tau) with ``mpcq.channel``.
        ``params`` None: the defaults (all zero: a channel that changes nothing), with
        ``overrides``.  Calling it again with the same delay and latency only replaces the
        amplitudes; other depths refill the rings at the next tick."""
        self._enable("channel", params, overrides)

    def disable_channel(self):
        """The ticks after it run without the channel's two launches; the arrays stay."""
        self._disable("channel")

    def channel_read(self, what: int):
        """HV_CLOCK (B, 2) int32 (epoch, next tau), HV_OBS / HV_F_CMD (B, 12), HV_DRAW (B, 16),
        HV_S_RING (B, 8, 12) or HV_F_RING (B, 4, 12)."""
        return self._group_read("channel", what)

    def channel_device_ptr(self, what: int) -> int:
        return self._group_ptr("channel", what)

    # ------------------------------------------------------------------ estimator
    def enable_estimator(self, params: L.EstimatorParams | None = None, **overrides):
        """Opt in to the state estimator: every later tick runs, between the channel's observe
        stage and the planner, a per-robot Kalman filter on the MPC's own model that takes what
        the planner would have read (HV_OBS, or the state as staged) as a measurement ``lag``
        ticks old and predicts forward to now through the recorded SV_F0 (acting ``f_lag`` ticks
        late) and footholds; the planner reads EV_EST, the plant and the monitor keep the
        truth.  Set ``lag`` / ``f_lag`` to the channel's ``delay`` / ``latency`` and ``r`` to its
        ``sigma**2``.  ``params`` None: the defaults, with ``overrides``.  Calling it while
        enabled only replaces the parameters (another ``lag`` re-initialises every robot at its
        next tick); enabling after a disable starts every filter anew."""
        self._enable("estimator", params, overrides)

    def disable_estimator(self):
        """The ticks after it run without the estimator's launch; the arrays stay."""
        self._disable("estimator")

    def estimator_read(self, what: int):
        """EV_EST (B, 12) the last tick's estimate, or EV_ROW (B, EST_ROW) the filter state
        (``mpcq.estimator.unpack`` names its parts)."""
        return self._group_read("estimator", what)

    def estimator_device_ptr(self, what: int) -> int:
        return self._group_ptr("estimator", what)

    # ------------------------------------------------------------------ disturbance stage
    def enable_disturb(self, params: L.DisturbParams | None = None, **overrides):
        """Opt in to the disturbance stage: every later tick runs, after the estimator and before
        the planner, a per-robot observer that samples the acceleration the controller's model
        lacks -- (what the planner is about to read - the model's step from the previous tick's
        reading under the recorded SV_F0, acting ``f_lag`` ticks late) / dt --, filters it with
        gain ``alpha``, clips it to ``d_max`` and writes DV_DIST.  With ``compensate`` (the
        default) the solve takes DV_DIST as its disturbance table, ahead of ``set_disturbance``'s;
        with ``compensate=0`` the stage only estimates.  Set ``f_lag`` to the channel's
        ``latency``.  ``params`` None: the defaults, with ``overrides``.  Calling it while
        enabled only replaces the parameters; enabling after a disable starts every row anew."""
        self._enable("disturb", params, overrides)

    def disable_disturb(self):
        """The ticks after it run without the stage's launch; the arrays stay."""
        self._disable("disturb")

    def disturb_read(self, what: int):
        """DV_DIST (B,) DISTURBANCE_DTYPE what the solve reads, DV_ROW (B, DIST_ROW) the stage's
        state (``mpcq.disturb.unpack`` names its parts), or DV_RESID (B, 6) the last tick's raw
        sample (NaN where none was taken)."""
        return self._group_read("disturb", what)

    def disturb_device_ptr(self, what: int) -> int:
        return self._group_ptr("disturb", what)

    # ------------------------------------------------------------------ gait transitions
    def enable_gait(self, cycles, params: L.GaitParams | None = None, **overrides):
        """Opt in to gait transitions: every later tick rolls each robot's gait table with the
        step that enters the horizon taken from a desired gait cycle (include/mpcq.h has the
        rules).  ``cycles``: 1 to GAIT_MAX library entries, names for ``mpcq.gait.cycle`` or
        (20, 5) arrays.  ``overrides``: ``select`` (GAIT_MANUAL: ``set_gait`` requests;
        GAIT_BY_SPEED: the kernel picks from the commanded speed by ``thresholds``, ``hysteresis``
        and ``yaw_weight``) and ``align`` (1: switch only at a phase boundary).  Calling it again
        replaces library and parameters; the robots' rows (GV_STATE) stay.  A refusal of the
        library leaves the settings in force."""
        from . import gait as G
        cy = G.library(cycles)
        gp = G.params_for(cy, params, **overrides)
        self.engine._call("mpcq_session_enable_gait", self._h, C.byref(gp), C.c_void_p(cy.ctypes.data))
        self.gait_params, self.gait_cycles = gp, cy

    def disable_gait(self):
        """The ticks after it run the planner's own roll again; GV_STATE stays."""
        self._disable("gait")

    def set_gait(self, ids):
        """Request library entry ``ids`` (a scalar broadcasts to (B,); -1 withdraws a request that
        has not been taken yet) under GAIT_MANUAL; each robot switches at its next phase
        boundary (``align`` 1) or at its next tick."""
        ids = np.ascontiguousarray(np.broadcast_to(np.asarray(ids, np.int32), (self.batch,)))
        self.engine._call("mpcq_session_set_gait", self._h, C.c_void_p(ids.ctypes.data), 0)

    def set_gait_device(self, ptr: int, asynchronous: bool = True):
        """``set_gait`` from a device-resident int32 [B], enqueued on the engine's stream."""
        flags = L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
        self.engine._call("mpcq_session_set_gait", self._h, C.c_void_p(ptr) if ptr else None, flags)

    def gait_state(self):
        """GV_STATE (B, 4) int32: (want, active, phase, switches) per robot."""
        return self._group_read("gait", L.GV_STATE)

    def gait_device_ptr(self, what: int = L.GV_STATE) -> int:
        return self._group_ptr("gait", what)

    # ------------------------------------------------------------------ rollouts
    def _to_device(self, a):
        """A host array on the engine's device through torch: (the tensor, which owns the memory,
        its address).  The copy has completed when this returns."""
        import torch
        t = torch.from_numpy(a).to(f"cuda:{self.engine.device}")
        return t, t.data_ptr()

    def _new_device(self, shape):
        """An uninitialised float64 device array through torch: (tensor, address, to_numpy)."""
        import torch
        t = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.engine.device}")
        return t, t.data_ptr(), lambda: t.cpu().numpy()

    def run(self, v_ref, n_ticks: int, trace: bool = False, k: int | None = None):
        """``n_ticks`` ticks of the virtual robot (or the plant) enqueued in one call.  ``v_ref``
        (host) is (6,) or (B, 6) for every tick, or a schedule (T, B, 6) whose last row is held
        once the ticks outrun it; None: the commands of ``enable_scenario``.  ``trace=True``
        (needs ``enable_monitor``) returns the monitor's per-tick rows (n_ticks, B, TRACE),
        otherwise None."""
        B = self.batch
        n_ticks = int(n_ticks)
        keep, v_ptr, v_ticks = None, 0, 1
        if v_ref is not None:
            v = np.asarray(v_ref, np.float64)
            if v.ndim < 3:
                v = np.broadcast_to(v, (1, B, 6))
            elif v.ndim != 3 or v.shape[0] < 1:
                raise ValueError(f"v_ref must be (6,), ({B}, 6) or (T, {B}, 6); got {v.shape}")
            v = np.ascontiguousarray(np.broadcast_to(v, (v.shape[0], B, 6)))
            keep, v_ptr = self._to_device(v)
            v_ticks = v.shape[0]
        tr, tr_ptr, fetch = self._new_device((max(n_ticks, 0), B, L.TRACE)) if trace else (None, 0, None)
        self.run_device(v_ptr, n_ticks, v_ref_ticks=v_ticks, trace_ptr=tr_ptr, k=k, asynchronous=False)
        del keep
        return fetch() if trace else None

    def run_device(self, v_ref_ptr: int, n_ticks: int, v_ref_ticks: int = 1, trace_ptr: int = 0,
                   k: int | None = None, asynchronous: bool = True):
        """``run`` on device arrays: v_ref (v_ref_ticks, B, 6) or 0 (the commands of
        ``enable_scenario``), trace (n_ticks, B, TRACE) or 0."""
        k = self.k if k is None else int(k)
        v = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        flags = L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
        self.engine._call("mpcq_session_run", self._h, k, int(n_ticks), v(v_ref_ptr), int(v_ref_ticks), v(trace_ptr),
                          flags)
        self.k = k + int(n_ticks)

    def close(self):
        if getattr(self, "_h", None):
            L.lib().mpcq_session_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _in(self, a, shape, dtype=np.float64):
        if a is None:
            return None
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype), shape))
        return a

    def tick(self, v_ref=None, state=None, l_feet=None, reduced=None, k: int | None = None):
        """One control tick for every robot (host arrays); returns f_applied (B, 12).  ``v_ref``
        None: the commands of ``enable_scenario``."""
        B = self.batch
        k = self.k if k is None else int(k)
        vr = self._in(v_ref, (B, 6))
        st = self._in(state, (B, 12))
        lf = self._in(l_feet, (B, 3, 4))
        rd = self._in(reduced, (B,), np.int32)
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        self.engine._call("mpcq_session_tick", self._h, k, p(st), p(lf), p(vr), p(rd), 0)
        self.k = k + 1
        return self.read(L.SV_F0)

    def tick_device(self, v_ref_ptr: int, state_ptr: int = 0, l_feet_ptr: int = 0, reduced_ptr: int = 0,
                    k: int | None = None, asynchronous: bool = True):
        """One tick on device-resident inputs (pointers on the engine's device; v_ref 0: the
        commands of ``enable_scenario``)."""
        k = self.k if k is None else int(k)
        v = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        flags = L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
        self.engine._call("mpcq_session_tick", self._h, k, v(state_ptr), v(l_feet_ptr), v(v_ref_ptr), v(reduced_ptr),
                                          flags)
        self.k = k + 1

    def reset(self, mask=None, gait0=None, q_w0=None):
        """Restart the robots with a nonzero ``mask`` entry (None: all) between two ticks (host
        arrays): their state goes back to what the constructor leaves, with the gait table
        ``gait0`` (None: the table the session was created with) and the world pose ``q_w0``
        (None: the default), and their next tick runs as a first tick whatever ``k`` is; the
        other robots are not touched.  ``mask`` broadcasts to (B,), ``gait0`` to (B, 20, 5),
        ``q_w0`` to (B, 6).  ``Session.k`` keeps counting."""
        B = self.batch
        m = None if mask is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mask) != 0, (B,)), np.int32)
        g = self._in(gait0, (B, 20, 5))
        q = self._in(q_w0, (B, 6))
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        self.engine._call("mpcq_session_reset", self._h, p(m), p(g), p(q), 0)

    def reset_device(self, mask_ptr: int = 0, gait0_ptr: int = 0, q_w0_ptr: int = 0, asynchronous: bool = True):
        """``reset`` on device-resident arrays (int32 mask [B], gait0 [B, 20, 5], q_w0 [B, 6]; 0 =
        absent), enqueued on the engine's stream: a mask computed on the device stays there."""
        v = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        flags = L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
        self.engine._call("mpcq_session_reset", self._h, v(mask_ptr), v(gait0_ptr), v(q_w0_ptr), flags)

    # ------------------------------------------------------------------ snapshots
    def snapshot(self) -> Snapshot:
        """Save every robot's state on the device and return the ``Snapshot``."""
        return Snapshot(self).save()

    def snapshot_from(self, blob: bytes) -> Snapshot:
        """The snapshot ``Snapshot.tobytes`` wrote, on this session's engine (the same horizon)."""
        blob = bytes(blob)
        snap = Snapshot(self)
        try:
            self.engine._call("mpcq_session_snapshot_import", self._h, snap._h, blob, len(blob))
        except L.MpcqError:
            snap.close()
            raise
        snap.batch, = struct.unpack_from("<q", blob, 16)
        snap.k, = struct.unpack_from("<q", blob, L.SNAPSHOT_USER_OFFSET)
        return snap

    def _map(self, map):  # noqa: A002
        return np.ascontiguousarray(np.broadcast_to(np.asarray(map, np.int32), (self.batch,)))

    def _restored(self, snap: Snapshot, full: bool):
        # a full restore goes back to the snapshot's tick index; a mapped one keeps counting,
        # unless this session has not ticked: its robots then hold the snapshot's state
        if full or self.k == 0:
            self.k = snap.k

    def restore(self, snap: Snapshot, map=None):  # noqa: A002
        """Slot b takes row ``map[b]`` of ``snap``; -1 leaves the robot alone.  ``map`` broadcasts
        to (B,) int32: a scalar r means every slot from row r.  None: the identity over every
        robot (the same batch), which also restores MV_TOTALS and sets ``Session.k`` back to the
        snapshot's.  A mapped restore leaves ``Session.k`` alone, unless this session has not
        ticked yet: it then takes the snapshot's."""
        m = None if map is None else self._map(map)
        self.engine._call("mpcq_session_snapshot_restore", self._h, snap._h,
                          None if m is None else C.c_void_p(m.ctypes.data), 0)
        self._restored(snap, m is None)

    def restore_device(self, snap: Snapshot, map_ptr: int, asynchronous: bool = True):
        """``restore`` from a device map (int32 [B]; 0: the identity), enqueued on the engine's
        stream; an entry outside the snapshot's rows acts as -1.  Ticked state into a session that
        has not ticked yet is refused from a device map (it would have to cover every robot, which
        only a host map lets the library check): use ``restore``."""
        flags = L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
        self.engine._call("mpcq_session_snapshot_restore", self._h, snap._h, C.c_void_p(map_ptr) if map_ptr else None,
                          flags)
        self._restored(snap, not map_ptr)

    def fork(self, map):  # noqa: A002
        """Branch inside the live session: slot b continues from robot ``map[b]`` as it stands now
        (-1: untouched; a scalar r: every slot from robot r).  ``Session.k`` keeps counting."""
        m = self._map(map)
        self.engine._call("mpcq_session_fork", self._h, C.c_void_p(m.ctypes.data), 0)

    def fork_device(self, map_ptr: int, asynchronous: bool = True):
        """``fork`` from a device map (int32 [B])."""
        flags = L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
        self.engine._call("mpcq_session_fork", self._h, C.c_void_p(map_ptr) if map_ptr else None, flags)

    def read(self, what: int):
        return self._group_read("session", what)

    def write(self, what: int, value):
        shape, dt = self._group_shape("session", what)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dt), shape))
        self.engine._call("mpcq_session_write", self._h, what, C.c_void_p(a.ctypes.data), 0)

    def device_ptr(self, what: int) -> int:
        return self._group_ptr("session", what)
