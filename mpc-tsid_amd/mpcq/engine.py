"""Batched engine: numpy (host) and device-pointer front ends over libmpcq.so.

``Engine(n_steps)`` is the batched counterpart of one ``MPC.MPC`` +
``osqp.OSQP`` pair (MPC.py:22-82): it owns a HIP context on one device.

* ``formulate(xref, fsteps, mode)``  -> A.data / l / u exactly as
  MPC.update_matrices (MPC.py:290-378) or create_matrices (MPC.py:84-234).
* ``qp_solve(Ax, l, u, ...)``        -> osqp update + warm_start + solve
  (MPC.py:419-428) for every instance.
* ``solve(xref, fsteps, mode, ...)`` -> the fused hot path of MPC.run
  (MPC.py:460-514): formulation + solve + f_applied.

Host arrays go through pinned-free staging inside the library; the
``*_device`` variants take raw device pointers (e.g. ``tensor.data_ptr()``)
so callers can keep inputs resident in HBM and time the kernel alone.
"""
from __future__ import annotations

import ctypes as C
import threading
import weakref

import numpy as np

from . import _lib as L


def dims(n_steps: int):
    return 24 * n_steps, 44 * n_steps, 126 * n_steps - 18


def pattern(n_steps: int):
    n, m, nnz = dims(n_steps)
    indptr = np.zeros(n + 1, np.int32)
    indices = np.zeros(nnz, np.int32)
    L.check(L.lib().mpcq_pattern(n_steps, indptr.ctypes.data_as(C.POINTER(C.c_int32)),
                                 indices.ctypes.data_as(C.POINTER(C.c_int32))))
    return indptr, indices


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _f64(a, shape=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


# numpy mirror of struct mpcq_robot (L.Robot), gI as the 3x3 it is
ROBOT_DTYPE = np.dtype([("mass", np.float64), ("gI", np.float64, (3, 3)), ("mu", np.float64),
                        ("fz_max", np.float64), ("reserved", np.float64, (4,))])


def robots(B: int, mass=None, gI=None, mu=None, fz_max=None, params: L.Params | None = None):
    """A table of per-robot constants for ``Engine.set_robots`` / ``Session.set_robots``: a
    contiguous (B,) array of ROBOT_DTYPE.  mass, mu, fz_max: a scalar or (B,); gI: (3,3) or
    (B,3,3).  A field left None comes from ``params`` (None: the default parameters)."""
    B = int(B)
    d = L.default_robot(params)
    out = np.zeros(B, ROBOT_DTYPE)
    for name, v in (("mass", mass), ("mu", mu), ("fz_max", fz_max)):
        out[name] = np.broadcast_to(np.asarray(getattr(d, name) if v is None else v, np.float64), (B,))
    g = np.array(d.gI[:]).reshape(3, 3) if gI is None else np.asarray(gI, np.float64)
    out["gI"] = np.broadcast_to(g, (B, 3, 3))
    return out


def _robot_table(table, count=None):
    """(B,) ROBOT_DTYPE, contiguous, from a ROBOT_DTYPE array or a ctypes array of L.Robot."""
    if not isinstance(table, np.ndarray):
        table = np.frombuffer(bytes(table), ROBOT_DTYPE)
    if table.dtype != ROBOT_DTYPE or table.ndim != 1:
        raise ValueError("a robot table is a (B,) array of mpcq.ROBOT_DTYPE (mpcq.robots())")
    if count is not None and table.shape[0] != count:
        raise ValueError(f"expected {count} robots, got {table.shape[0]}")
    return np.ascontiguousarray(table)


# numpy mirror of struct mpcq_weights (L.Weights)
WEIGHTS_DTYPE = np.dtype([("state", np.float64, (12,)), ("force", np.float64), ("reserved", np.float64, (3,))])


def weights(B: int, state=None, force=None, params: L.Params | None = None):
    """A table of per-instance cost weights for ``Engine.set_weights`` / ``Session.set_weights``:
    a contiguous (B,) array of WEIGHTS_DTYPE.  state: a scalar, (12,) or (B,12); force: a scalar or
    (B,).  A field left None comes from ``params`` (None: the default parameters)."""
    B = int(B)
    d = L.default_weights(params)
    out = np.zeros(B, WEIGHTS_DTYPE)
    out["state"] = np.broadcast_to(np.asarray(d.state[:] if state is None else state, np.float64), (B, 12))
    out["force"] = np.broadcast_to(np.asarray(d.force if force is None else force, np.float64), (B,))
    return out


def _weights_table(table, count=None):
    """(B,) WEIGHTS_DTYPE, contiguous, from a WEIGHTS_DTYPE array or a ctypes array of L.Weights."""
    if not isinstance(table, np.ndarray):
        table = np.frombuffer(bytes(table), WEIGHTS_DTYPE)
    if table.dtype != WEIGHTS_DTYPE or table.ndim != 1:
        raise ValueError("a weights table is a (B,) array of mpcq.WEIGHTS_DTYPE (mpcq.weights())")
    if count is not None and table.shape[0] != count:
        raise ValueError(f"expected {count} weight rows, got {table.shape[0]}")
    return np.ascontiguousarray(table)


# numpy mirror of struct mpcq_disturbance (L.Disturbance)
DISTURBANCE_DTYPE = np.dtype([("a", np.float64, (6,)), ("reserved", np.float64, (2,))])


def disturbances(B: int, lin=None, ang=None):
    """A table of per-instance constant disturbance accelerations for ``Engine.set_disturbance`` /
    ``Session.set_disturbance``: a contiguous (B,) array of DISTURBANCE_DTYPE.  lin [m/s^2] and
    ang [rad/s^2]: a scalar, (3,) or (B,3), in the instance's xref frame; None: zero."""
    B = int(B)
    out = np.zeros(B, DISTURBANCE_DTYPE)
    out["a"][:, :3] = np.broadcast_to(np.asarray(0.0 if lin is None else lin, np.float64), (B, 3))
    out["a"][:, 3:] = np.broadcast_to(np.asarray(0.0 if ang is None else ang, np.float64), (B, 3))
    return out


def _disturbance_table(table, count=None):
    """(B,) DISTURBANCE_DTYPE, contiguous, from such an array or a ctypes array of L.Disturbance."""
    if not isinstance(table, np.ndarray):
        table = np.frombuffer(bytes(table), DISTURBANCE_DTYPE)
    if table.dtype != DISTURBANCE_DTYPE or table.ndim != 1:
        raise ValueError("a disturbance table is a (B,) array of mpcq.DISTURBANCE_DTYPE (mpcq.disturbances())")
    if count is not None and table.shape[0] != count:
        raise ValueError(f"expected {count} disturbance rows, got {table.shape[0]}")
    return np.ascontiguousarray(table)


class Engine:
    """One HIP context (device, horizon N, parameters)."""

    def __init__(self, n_steps: int = 16, device: int = 0, params: L.Params | None = None, **overrides):
        self.n_steps = int(n_steps)
        self.device = int(device)
        self.params = params if params is not None else L.default_params()
        for k, v in overrides.items():
            setattr(self.params, k, v)
        self.n, self.m, self.nnz = dims(self.n_steps)
        self.lock = threading.RLock()
        self.has_robots = False  # whether a per-robot table is in force (set_robots / set_robots_device)
        self.has_weights = False  # whether a weights table is in force (set_weights / set_weights_device)
        self.has_disturbance = False  # the same for set_disturbance / set_disturbance_device
        h = C.c_void_p()
        L.check(L.lib().mpcq_create(self.device, self.n_steps, C.byref(self.params), C.byref(h)))
        self._h = h
        self._snapshots = weakref.WeakSet()  # live mpcq.Snapshot objects: closed before the context

    def _call(self, name: str, *args):
        """One C-ABI call on this context.  A context is used by one host thread at a
        time (include/mpcq.h): the lock serialises callers that share the Engine
        (the asynchronous MPC_Wrapper's worker and the caller's thread)."""
        with self.lock:
            return L.check(getattr(L.lib(), name)(*args))

    def close(self):
        if getattr(self, "_h", None):
            for snap in list(getattr(self, "_snapshots", ())):  # their destroy needs the context
                snap.close()
            with self.lock:
                L.lib().mpcq_destroy(self._h)
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

    # ------------------------------------------------------------------ host arrays
    def _batch_inputs(self, xref, fsteps):
        xref = _f64(xref)
        fsteps = _f64(fsteps)
        if xref.ndim == 2:
            xref = xref[None]
        if fsteps.ndim == 2:
            fsteps = fsteps[None]
        B = xref.shape[0]
        if xref.shape != (B, 12, self.n_steps + 1) or fsteps.shape != (B, 20, 13):
            raise ValueError(f"xref must be (B,12,{self.n_steps + 1}) and fsteps (B,20,13); got "
                             f"{xref.shape}, {fsteps.shape}")
        return np.ascontiguousarray(xref), np.ascontiguousarray(fsteps), B

    def formulate(self, xref, fsteps, mode: int = L.MODE_UPDATE):
        xref, fsteps, B = self._batch_inputs(xref, fsteps)
        Ax = np.empty((B, self.nnz))
        l = np.empty((B, self.m))
        u = np.empty((B, self.m))
        st = np.empty(B, np.int32)
        self._call("mpcq_formulate_batch", self._h, B, _p(xref), _p(fsteps), mode, _p(Ax), _p(l), _p(u),
                                             _p(st), 0)
        return dict(Ax=Ax, l=l, u=u, status=st)

    def qp_solve(self, Ax, l, u, warm_x=None, warm_y=None, rho=None, want_y: bool = True):
        Ax = _f64(Ax)
        B = Ax.shape[0] if Ax.ndim == 2 else 1
        Ax = Ax.reshape(B, self.nnz)
        l = _f64(l).reshape(B, self.m)
        u = _f64(u).reshape(B, self.m)
        wx = None if warm_x is None else _f64(warm_x).reshape(B, self.n)
        wy = None if warm_y is None else _f64(warm_y).reshape(B, self.m)
        rho_in = None if rho is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rho, np.float64), (B,)))
        x = np.empty((B, self.n))
        y = np.empty((B, self.m)) if want_y else None
        st = np.empty(B, np.int32)
        it = np.empty(B, np.int32)
        ro = np.empty(B)
        info = np.empty((B, 4), np.int32)
        self._call("mpcq_qp_solve_batch", self._h, B, _p(Ax), _p(l), _p(u), _p(wx), _p(wy), _p(rho_in),
                                            _p(x), _p(y), _p(st), _p(it), _p(ro), _p(info), 0)
        return dict(x=x, y=y, status=st, iters=it, rho=ro, rho_updates=info[:, 0], polish=info[:, 1],
                    polish_rounds=info[:, 2], admm_status=info[:, 3])

    def solve(self, xref, fsteps, mode: int = L.MODE_UPDATE, warm_x=None, warm_y=None, rho=None,
              want_x: bool = True, want_y: bool = False, order_by_class: bool = False):
        """Fused formulation + solve (mpcq_solve_batch): MPC.run's QP for a batch, with
        the osqp workspace of the previous tick (warm_x, warm_y, rho) when given.
        order_by_class: MPCQ_FLAG_ORDER_BY_CLASS (dispatch by the mean iteration count each
        gait class has shown on this engine; results unchanged)."""
        xref, fsteps, B = self._batch_inputs(xref, fsteps)
        wx = None if warm_x is None else _f64(warm_x).reshape(B, self.n)
        wy = None if warm_y is None else _f64(warm_y).reshape(B, self.m)
        rin = None if rho is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rho, np.float64), (B,)))
        f0 = np.empty((B, 12))
        x = np.empty((B, self.n)) if want_x else None
        y = np.empty((B, self.m)) if want_y else None
        rout = np.empty(B)
        st = np.empty(B, np.int32)
        it = np.empty(B, np.int32)
        info = np.empty((B, 4), np.int32)
        self._call("mpcq_solve_batch", self._h, B, _p(xref), _p(fsteps), mode, _p(wx), _p(wy), _p(rin), _p(f0),
                                         _p(x), _p(y), _p(rout), _p(st), _p(it), _p(info),
                   L.FLAG_ORDER_BY_CLASS if order_by_class else 0)
        return dict(f0=f0, x=x, y=y, rho=rout, status=st, iters=it, rho_updates=info[:, 0], polish=info[:, 1],
                    polish_rounds=info[:, 2], admm_status=info[:, 3])

    # ------------------------------------------------------------------ footstep planner
    def plan(self, ops: int, k: int, state, l_feet, v_ref, gait, rot_flag, h_rot, xref, fsteps,
             reduced=None, v_cur=None, h=None, params: L.PlannerParams | None = None):
        """FootstepPlanner.update_fsteps + getRefStates for a batch (mpcq_plan_batch).

        ``gait`` (B,20,5), ``rot_flag`` (B,) int32, ``h_rot`` (B,), ``xref`` (B,12,N+1) and
        ``fsteps`` (B,20,13) are C-contiguous arrays updated in place.  Returns status (B,):
        0, or STATUS_BAD_GAIT where the reference raises (that instance left unchanged)."""
        B = int(np.shape(state)[0])
        N = self.n_steps
        state = _f64(state, (B, 12))
        v_ref = _f64(v_ref, (B, 6))
        l_feet = None if l_feet is None else _f64(l_feet, (B, 3, 4))
        v_cur = None if v_cur is None else _f64(v_cur, (B, 6))
        h = None if h is None else _f64(h, (B,))
        red = None if reduced is None else np.ascontiguousarray(np.broadcast_to(np.asarray(reduced, np.int32), (B,)))
        for name, arr, shp, dt in (("gait", gait, (B, 20, 5), np.float64), ("rot_flag", rot_flag, (B,), np.int32),
                                   ("h_rot", h_rot, (B,), np.float64), ("xref", xref, (B, 12, N + 1), np.float64),
                                   ("fsteps", fsteps, (B, 20, 13), np.float64)):
            if arr is None:
                continue
            if arr.shape != shp or arr.dtype != dt or not arr.flags.c_contiguous:
                raise ValueError(f"{name} must be a C-contiguous {np.dtype(dt).name} array of shape {shp}")
        st = np.empty(B, np.int32)
        pp = params if params is not None else L.default_planner_params(dt=self.params.dt)
        self._call("mpcq_plan_batch", self._h, C.byref(pp), B, ops, int(k), _p(state), _p(v_cur), _p(h),
                                        _p(l_feet), _p(v_ref), _p(red), _p(gait), _p(rot_flag), _p(h_rot),
                                        _p(xref), _p(fsteps), _p(st), 0)
        return st

    def plan_device(self, batch: int, ops: int, k: int, state_ptr: int, l_feet_ptr: int, v_ref_ptr: int,
                    gait_ptr: int, rot_flag_ptr: int, h_rot_ptr: int, xref_ptr: int, fsteps_ptr: int,
                    status_ptr: int = 0, reduced_ptr: int = 0, v_cur_ptr: int = 0, h_ptr: int = 0,
                    params: L.PlannerParams | None = None, asynchronous: bool = False):
        flags = L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
        v = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        pp = params if params is not None else L.default_planner_params(dt=self.params.dt)
        self._call("mpcq_plan_batch", self._h, C.byref(pp), int(batch), ops, int(k), v(state_ptr), v(v_cur_ptr),
                                        v(h_ptr), v(l_feet_ptr), v(v_ref_ptr), v(reduced_ptr), v(gait_ptr),
                                        v(rot_flag_ptr), v(h_rot_ptr), v(xref_ptr), v(fsteps_ptr), v(status_ptr),
                                        flags)

    # ------------------------------------------------------------------ device pointers
    def set_stream(self, stream_handle: int | None):
        self._call("mpcq_set_stream", self._h, C.c_void_p(stream_handle or 0))

    def set_slice(self, slice_iters: int):
        """Sliced batch solves (mpcq_set_slice): beyond 16 stages each batch solve suspends the
        instances still iterating after ``slice_iters`` ADMM iterations and resumes them in a
        second launch, the farthest from convergence first, to their end -- bit-identical
        outputs, a shorter dispatch tail.  0: off."""
        self._call("mpcq_set_slice", self._h, int(slice_iters))

    def set_robots(self, table):
        """Per-instance mass, gI, mu, fz_max (mpcq_set_robots): instance b of every later
        formulate / solve takes them from ``table[b]`` (``mpcq.robots()``), everything else from
        the engine's parameters; a batch larger than the table is an error.  None clears it."""
        if table is None:
            self._call("mpcq_set_robots", self._h, 0, None, 0)
            self.has_robots = False
            return
        t = _robot_table(table)
        self._call("mpcq_set_robots", self._h, t.shape[0], _p(t), 0)
        self.has_robots = t.shape[0] > 0

    def set_weights(self, table):
        """Per-instance diagonal of P (mpcq_set_weights): instance b of every later solve takes
        state_weights and force_weight from ``table[b]`` (``mpcq.weights()``), everything else from
        the engine's parameters (and the robots table, where set).  None clears the table."""
        if table is None:
            self._call("mpcq_set_weights", self._h, 0, None, 0)
            self.has_weights = False
            return
        t = _weights_table(table)
        self._call("mpcq_set_weights", self._h, t.shape[0], _p(t), 0)
        self.has_weights = t.shape[0] > 0

    def set_weights_device(self, ptr: int, count: int):
        """The same from ``count`` mpcq_weights records in device memory (copied on the engine's
        stream, not validated).  ``count`` 0 or a null ``ptr`` clears the table."""
        self._call("mpcq_set_weights", self._h, int(count), C.c_void_p(ptr) if ptr else None, L.FLAG_DEVICE_PTRS)
        self.has_weights = bool(ptr) and int(count) > 0

    def set_disturbance(self, table):
        """Per-instance constant disturbance acceleration (mpcq_set_disturbance): the model of
        instance b of every later formulate / solve carries ``table[b]`` (``mpcq.disturbances()``)
        beside gravity through its whole horizon, in the instance's xref frame.  None clears it."""
        if table is None:
            self._call("mpcq_set_disturbance", self._h, 0, None, 0)
            self.has_disturbance = False
            return
        t = _disturbance_table(table)
        self._call("mpcq_set_disturbance", self._h, t.shape[0], _p(t), 0)
        self.has_disturbance = t.shape[0] > 0

    def set_disturbance_device(self, ptr: int, count: int):
        """The same from ``count`` mpcq_disturbance records in device memory (copied on the
        engine's stream, not validated).  ``count`` 0 or a null ``ptr`` clears the table."""
        self._call("mpcq_set_disturbance", self._h, int(count), C.c_void_p(ptr) if ptr else None, L.FLAG_DEVICE_PTRS)
        self.has_disturbance = bool(ptr) and int(count) > 0

    def set_robots_device(self, ptr: int, count: int):
        """The same from ``count`` mpcq_robot records in device memory (copied on the engine's
        stream, not validated)."""
        self._call("mpcq_set_robots", self._h, int(count), C.c_void_p(ptr) if ptr else None, L.FLAG_DEVICE_PTRS)
        self.has_robots = bool(ptr) and int(count) > 0

    def solve_device(self, batch: int, xref_ptr: int, fsteps_ptr: int, f0_ptr: int, status_ptr: int,
                     iters_ptr: int = 0, x_ptr: int = 0, y_ptr: int = 0, mode: int = L.MODE_UPDATE,
                     warm_x_ptr: int = 0, warm_y_ptr: int = 0, info_ptr: int = 0,
                     asynchronous: bool = False, order_by_class: bool = False):
        flags = (L.FLAG_DEVICE_PTRS | (L.FLAG_ASYNC if asynchronous else 0)
                 | (L.FLAG_ORDER_BY_CLASS if order_by_class else 0))
        v = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        self._call("mpcq_solve_batch", self._h, int(batch), v(xref_ptr), v(fsteps_ptr), mode, v(warm_x_ptr),
                                         v(warm_y_ptr), None, v(f0_ptr), v(x_ptr), v(y_ptr), None, v(status_ptr),
                                         v(iters_ptr), v(info_ptr), flags)

    # ------------------------------------------------------------------ diagnostics
    # The dispatch-order kernels on their own (mpcq_debug_*, include/mpcq.h): no engine launch.
    @staticmethod
    def class_table_slots() -> int:
        return L.lib().mpcq_debug_class_table_slots()

    @staticmethod
    def suspended_status() -> int:
        return L.lib().mpcq_debug_suspended_status()

    def class_table(self):
        """(sum, cnt): this engine's class table, uint64 per slot."""
        k = self.class_table_slots()
        s, n = np.empty(k, np.uint64), np.empty(k, np.uint64)
        self._call("mpcq_debug_class_table_read", self._h, _p(s), _p(n))
        return s, n

    def set_class_table(self, sum, cnt):  # noqa: A002
        k = self.class_table_slots()
        s = np.ascontiguousarray(sum, dtype=np.uint64)
        n = np.ascontiguousarray(cnt, dtype=np.uint64)
        if s.shape != (k,) or n.shape != (k,):
            raise ValueError(f"the class table has {k} slots")
        self._call("mpcq_debug_class_table_write", self._h, _p(s), _p(n))

    def class_order(self, fsteps):
        """(cls, order) of fsteps (B,20,13) on the table as it stands."""
        fsteps = np.ascontiguousarray(fsteps, dtype=np.float64)
        B = fsteps.shape[0]
        if fsteps.shape != (B, 20, 13):
            raise ValueError(f"fsteps must be (B,20,13); got {fsteps.shape}")
        cls, order = np.empty(B, np.int32), np.empty(B, np.int32)
        self._call("mpcq_debug_class_order", self._h, B, _p(fsteps), _p(cls), _p(order))
        return cls, order

    def class_learn(self, cls, iters):
        cls = np.ascontiguousarray(cls, dtype=np.int32)
        iters = np.ascontiguousarray(iters, dtype=np.int32)
        if cls.ndim != 1 or cls.shape != iters.shape:
            raise ValueError("cls and iters must be 1-d arrays of one length")
        self._call("mpcq_debug_class_learn", self._h, cls.shape[0], _p(cls), _p(iters))

    def suspended_list(self, prev, n: int, status, key):
        """(list[:count], count): the resumed launch's list from prev (n,) or None, status (M,)
        and key (M,2)."""
        prev = None if prev is None else np.ascontiguousarray(prev, dtype=np.int32)
        status = np.ascontiguousarray(status, dtype=np.int32)
        key = np.ascontiguousarray(key, dtype=np.float64)
        M = status.shape[0]
        if key.shape != (M, 2) or (prev is not None and prev.shape != (n,)):
            raise ValueError("status (M,), key (M,2), prev (n,) or None")
        lst = np.empty(n, np.int32)
        cnt = C.c_int32()
        self._call("mpcq_debug_suspended", self._h, int(n), M, _p(prev), _p(status), _p(key), _p(lst), C.byref(cnt))
        return lst[:cnt.value], cnt.value

    def session_order(self, iters):
        iters = np.ascontiguousarray(iters, dtype=np.int32)
        order = np.empty(iters.shape[0], np.int32)
        self._call("mpcq_debug_session_order", self._h, iters.shape[0], _p(iters), _p(order))
        return order

    def last_dispatch(self):
        """What the last solve / qp_solve dispatched by: dict(batch, sliced, by_class, cls, order
        (None unless by_class), list (the resumed launch's instances in its order; empty unless
        sliced), count, key (B,2), None unless sliced)."""
        B = C.c_int64()
        self._call("mpcq_debug_last_dispatch", self._h, C.byref(B), None, None, None, None, None, None, None)
        B = B.value
        sl, bc, cnt = C.c_int32(), C.c_int32(), C.c_int32()
        cls, order, lst = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
        key = np.empty((B, 2))
        self._call("mpcq_debug_last_dispatch", self._h, None, C.byref(sl), C.byref(bc), _p(cls), _p(order),
                   _p(lst), C.byref(cnt), _p(key))
        return dict(batch=B, sliced=bool(sl.value), by_class=bool(bc.value),
                    cls=cls if bc.value else None, order=order if bc.value else None,
                    list=lst[:cnt.value].copy(), count=cnt.value, key=key if sl.value else None)

    def last_kernel_ms(self):
        f = C.c_double()
        s = C.c_double()
        self._call("mpcq_last_kernel_ms", self._h, C.byref(f), C.byref(s))
        return f.value, s.value
