"""ctypes binding of libmpcq.so (the C ABI in include/mpcq.h).

The shared library is built in-tree (mpc-tsid_amd/csrc/Makefile ->
mpc-tsid_amd/mpcq/libmpcq.so) and loaded from here.  There is no fallback:
if the library or a HIP device is missing, the calls raise.

torch bundles its own HIP runtime (torch/lib/libamdhip64.so, soname
libamdhip64.so.7, the same as /opt/rocm's).  If libmpcq.so were loaded first
it would bind /opt/rocm's copy, torch would load its own next to it, and two
runtimes in one process leave torch without a device (tools/diag_runtime.py).
So before loading libmpcq.so this module loads the HIP runtime torch will use
(torch's own copy, found without importing torch) with RTLD_GLOBAL: libmpcq.so
binds to it whatever the import order, and there is one runtime per process.
Without torch installed, /opt/rocm's runtime is used.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")
# MPCQ_LIB_VARIANT=stamps loads the diagnostic build of the same Makefile
# (per-phase cycle stamps, tools/stamps.py); MPCQ_LIB_VARIANT=exp:<name> loads an
# experiment build from csrc/build/variants (tools/build_variant.sh, timing tools
# only -- outside the package, never shipped)
_VARIANT = os.environ.get("MPCQ_LIB_VARIANT") or ""
if _VARIANT == "stamps":
    LIB_PATH = os.path.join(HERE, "libmpcq_stamps.so")
elif _VARIANT.startswith("exp:"):
    LIB_PATH = os.path.join(CSRC, "build", "variants", f"libmpcq_{_VARIANT[4:]}.so")
elif _VARIANT:
    raise ImportError(f"MPCQ_LIB_VARIANT={_VARIANT!r}: 'stamps' or 'exp:<name>'")
else:
    LIB_PATH = os.path.join(HERE, "libmpcq.so")

# return codes / status / flags / modes (include/mpcq.h)
OK = 0
E_INVALID, E_DEVICE, E_NOMEM, E_UNSUPPORTED = -1, -2, -3, -4
STATUS_SOLVED = 1
STATUS_SOLVED_INACCURATE = 2
STATUS_MAX_ITER_REACHED = -2
STATUS_PRIMAL_INFEASIBLE = -3
STATUS_DUAL_INFEASIBLE = -4
STATUS_PRIMAL_INFEASIBLE_INACCURATE = 3
STATUS_DUAL_INFEASIBLE_INACCURATE = 4
STATUS_NONFINITE = -10
STATUS_BAD_GAIT = -11
STATUS_FACTOR_FAILED = -12
STATUS_BAD_BOUNDS = -13
FLAG_DEVICE_PTRS = 1
FLAG_ASYNC = 2
FLAG_ORDER_BY_CLASS = 4  # mpcq_solve_batch: dispatch by the learned cost of each gait class
MODE_UPDATE = 0
MODE_SETUP = 1
PLAN_ROLL, PLAN_FOOTSTEPS, PLAN_REFSTATES = 1, 2, 4
PLAN_TICK = PLAN_ROLL | PLAN_FOOTSTEPS | PLAN_REFSTATES
# closed-loop session arrays (MPCQ_SV_*)
SV_F0, SV_X, SV_X_ROBOT, SV_Q_W, SV_COST, SV_XREF, SV_FSTEPS, SV_GAIT = range(8)
SV_STATUS, SV_ITERS, SV_RHO, SV_Y, SV_STATE, SV_L_FEET, SV_ROT_FLAG, SV_H_ROT = range(8, 16)
SV_ORDER = 16  # read-only: the next tick's dispatch order
# only on a session with enable_swing: the tick's swing-foot references (read-only), the
# generators' state, the frame of the tick's fsteps (read-only)
SV_SWING_REF, SV_SWING_STATE, SV_FRAME = 17, 18, 19
SV_FIRST = 20  # read-only: 1 = a reset is pending, the robot's next tick runs as a first tick
SWING_STATE = 40  # MPCQ_SWING_STATE: doubles per foot
# the rigid-body plant: integrators (MPCQ_PLANT_*) and a session's plant arrays (MPCQ_PV_*)
PLANT_MODEL, PLANT_RIGID = 0, 1
PV_STATE_END, PV_F_EFF, PV_WRENCH = 0, 1, 2
# the episode monitor: done bits (MPCQ_DONE_*), a session's monitor arrays (MPCQ_MV_*), the
# doubles of a trace row (MPCQ_TRACE)
DONE_NONFINITE, DONE_TILT, DONE_HEIGHT, DONE_SOLVER, DONE_TIMEOUT = 1, 2, 4, 8, 16
MV_DONE, MV_EP, MV_EP_TICKS, MV_EPISODES, MV_LAST, MV_TOTALS = range(6)
TRACE = 16
# the scenario stage: a session's scenario arrays (MPCQ_CV_*)
CV_EPOCH, CV_TICK, CV_V_REF, CV_PUSH, CV_WRENCH, CV_ROBOTS, CV_DRAW = range(7)
# the channel: a session's channel arrays (MPCQ_HV_*), the ring depths
HV_CLOCK, HV_OBS, HV_F_CMD, HV_DRAW, HV_S_RING, HV_F_RING = range(6)
CHANNEL_MAX_DELAY, CHANNEL_MAX_LATENCY = 8, 4
# the estimator: a session's estimator arrays (MPCQ_EV_*), the filter row's offsets in doubles
# (MPCQ_EST_*), the greatest lags
EV_EST, EV_ROW = range(2)
EST_POST, EST_PREV, EST_P, EST_CLOCK, EST_RING, EST_SLOTS, EST_ROW = 0, 12, 24, 42, 44, 12, 332
# the disturbance stage: a session's disturb arrays (MPCQ_DV_*), its row's offsets in doubles
# (MPCQ_DIST_*), the greatest force lag
DV_DIST, DV_ROW, DV_RESID = range(3)
DIST_D, DIST_PREV, DIST_CLOCK, DIST_RING, DIST_SLOTS, DIST_ROW = 0, 6, 18, 20, 5, 80
DISTURB_MAX_F_LAG = 4
ESTIMATOR_MAX_LAG, ESTIMATOR_MAX_F_LAG = 8, 4
# the gait stage: a session's gait array (MPCQ_GV_*), the library's bound, the selection modes
GV_STATE = 0
GAIT_MAX = 8
GAIT_MANUAL, GAIT_BY_SPEED = 0, 1
SNAPSHOT_USER_OFFSET = 96  # a snapshot blob's header: the int64 left to the caller (include/mpcq.h)

EXPORTS = ("mpcq_abi_version", "mpcq_default_params", "mpcq_dims", "mpcq_pattern",
           "mpcq_supported_horizons", "mpcq_last_error", "mpcq_create", "mpcq_destroy",
           "mpcq_set_stream", "mpcq_set_slice", "mpcq_last_kernel_ms", "mpcq_formulate_batch",
           "mpcq_qp_solve_batch", "mpcq_solve_batch", "mpcq_default_planner_params",
           "mpcq_plan_batch", "mpcq_session_create", "mpcq_session_destroy", "mpcq_session_tick",
           "mpcq_session_read", "mpcq_session_write", "mpcq_session_device_ptr", "mpcq_debug_set_stamps",
           "mpcq_build_info",
           "mpcq_debug_class_table_slots", "mpcq_debug_class_table_read", "mpcq_debug_class_table_write",
           "mpcq_debug_class_order", "mpcq_debug_class_learn", "mpcq_debug_suspended_status",
           "mpcq_debug_suspended", "mpcq_debug_session_order", "mpcq_debug_last_dispatch",
           "mpcq_default_swing_params", "mpcq_swing_step_batch", "mpcq_swing_batch",
           "mpcq_session_enable_swing",
           "mpcq_default_robot", "mpcq_set_robots", "mpcq_session_set_robots", "mpcq_session_get_robots",
           "mpcq_default_weights", "mpcq_set_weights", "mpcq_session_set_weights", "mpcq_session_get_weights",
           "mpcq_set_disturbance", "mpcq_session_set_disturbance", "mpcq_session_get_disturbance",
           "mpcq_default_disturb_params", "mpcq_disturb_step_batch", "mpcq_session_enable_disturb",
           "mpcq_session_disable_disturb", "mpcq_session_disturb_read", "mpcq_session_disturb_device_ptr",
           "mpcq_session_reset",
           "mpcq_default_plant_params", "mpcq_plant_step_batch", "mpcq_session_enable_plant",
           "mpcq_session_disable_plant", "mpcq_session_set_plant_robots", "mpcq_session_set_wrench",
           "mpcq_session_plant_read", "mpcq_session_plant_device_ptr",
           "mpcq_default_monitor_params", "mpcq_monitor_step_batch", "mpcq_session_enable_monitor",
           "mpcq_session_disable_monitor", "mpcq_session_monitor_read", "mpcq_session_monitor_device_ptr",
           "mpcq_session_run",
           "mpcq_default_scenario_params", "mpcq_scenario_step_batch", "mpcq_session_enable_scenario",
           "mpcq_session_disable_scenario", "mpcq_session_scenario_read", "mpcq_session_scenario_device_ptr",
           "mpcq_default_channel_params", "mpcq_channel_observe_batch", "mpcq_channel_actuate_batch",
           "mpcq_session_enable_channel", "mpcq_session_disable_channel", "mpcq_session_channel_read",
           "mpcq_session_channel_device_ptr",
           "mpcq_default_estimator_params", "mpcq_estimator_step_batch", "mpcq_session_enable_estimator",
           "mpcq_session_disable_estimator", "mpcq_session_estimator_read", "mpcq_session_estimator_device_ptr",
           "mpcq_default_gait_params", "mpcq_gait_roll_batch", "mpcq_session_enable_gait",
           "mpcq_session_disable_gait", "mpcq_session_set_gait", "mpcq_session_gait_read",
           "mpcq_session_gait_device_ptr",
           "mpcq_session_snapshot_create", "mpcq_session_snapshot_destroy", "mpcq_session_snapshot_save",
           "mpcq_session_snapshot_restore", "mpcq_session_fork", "mpcq_session_snapshot_bytes",
           "mpcq_session_snapshot_export", "mpcq_session_snapshot_import", "mpcq_debug_gather_rows")


class MpcqError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mpcq error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """struct mpcq_params (include/mpcq.h)."""

    _fields_ = [
        ("dt", C.c_double),
        ("mass", C.c_double),
        ("gI", C.c_double * 9),
        ("mu", C.c_double),
        ("fz_max", C.c_double),
        ("gravity", C.c_double),
        ("state_weights", C.c_double * 12),
        ("force_weight", C.c_double),
        ("footholds", C.c_double * 12),
        ("rho", C.c_double),
        ("sigma", C.c_double),
        ("alpha", C.c_double),
        ("eps_abs", C.c_double),
        ("eps_rel", C.c_double),
        ("adaptive_rho_tolerance", C.c_double),
        ("delta", C.c_double),
        ("eps_prim_inf", C.c_double),
        ("eps_dual_inf", C.c_double),
        ("max_iter", C.c_int32),
        ("check_termination", C.c_int32),
        ("adaptive_rho", C.c_int32),
        ("adaptive_rho_interval", C.c_int32),
        ("scaling", C.c_int32),
        ("polish", C.c_int32),
        ("polish_refine_iter", C.c_int32),
        ("polish_rounds", C.c_int32),
        ("dual_warm", C.c_int32),
        ("reserved", C.c_int32 * 7),
    ]

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out


class PlannerParams(C.Structure):
    """struct mpcq_planner_params (include/mpcq.h)."""

    _fields_ = [
        ("dt", C.c_double),
        ("T_gait", C.c_double),
        ("h_ref", C.c_double),
        ("k_feedback", C.c_double),
        ("L", C.c_double),
        ("g", C.c_double),
        ("t_stance", C.c_double),
        ("cmd_threshold", C.c_double),
        ("shoulders", C.c_double * 8),
        ("reduced_offset", C.c_double * 8),
        ("reserved", C.c_int32 * 8),
    ]


class SwingParams(C.Structure):
    """struct mpcq_swing_params (include/mpcq.h)."""

    _fields_ = [
        ("dt", C.c_double),
        ("max_height", C.c_double),
        ("t_lock", C.c_double),
        ("feet_z", C.c_double),
        ("k_mpc", C.c_int32),
        ("reserved", C.c_int32 * 7),
    ]


class PlantParams(C.Structure):
    """struct mpcq_plant_params (include/mpcq.h)."""

    _fields_ = [
        ("dt", C.c_double),
        ("gravity", C.c_double),
        ("n_sub", C.c_int32),
        ("integrator", C.c_int32),
        ("clamp", C.c_int32),
        ("reserved", C.c_int32 * 5),
    ]


class MonitorParams(C.Structure):
    """struct mpcq_monitor_params (include/mpcq.h)."""

    _fields_ = [
        ("max_tilt", C.c_double),
        ("min_height", C.c_double),
        ("max_ticks", C.c_int32),
        ("auto_reset", C.c_int32),
        ("reserved", C.c_int32 * 10),
    ]


class ScenarioParams(C.Structure):
    """struct mpcq_scenario_params (include/mpcq.h)."""

    _fields_ = [
        ("seed", C.c_uint64),
        ("v_lo", C.c_double * 3),
        ("v_hi", C.c_double * 3),
        ("wrench_lo", C.c_double * 6),
        ("wrench_hi", C.c_double * 6),
        ("push_prob", C.c_double),
        ("mass_scale_lo", C.c_double),
        ("mass_scale_hi", C.c_double),
        ("mu_lo", C.c_double),
        ("mu_hi", C.c_double),
        ("commands", C.c_int32),
        ("cmd_start", C.c_int32),
        ("cmd_ramp", C.c_int32),
        ("cmd_period", C.c_int32),
        ("pushes", C.c_int32),
        ("push_first", C.c_int32),
        ("push_period", C.c_int32),
        ("push_jitter", C.c_int32),
        ("push_ticks", C.c_int32),
        ("push_flip", C.c_int32),
        ("robots", C.c_int32),
        ("reserved", C.c_int32 * 5),
    ]


class ChannelParams(C.Structure):
    """struct mpcq_channel_params (include/mpcq.h)."""

    _fields_ = [
        ("seed", C.c_uint64),
        ("delay", C.c_int32),
        ("latency", C.c_int32),
        ("hold_prob", C.c_double),
        ("sigma", C.c_double * 12),
        ("bias", C.c_double * 12),
        ("f_sigma", C.c_double * 3),
        ("f_gain", C.c_double),
        ("reserved", C.c_int32 * 2),
    ]


class EstimatorParams(C.Structure):
    """struct mpcq_estimator_params (include/mpcq.h)."""

    _fields_ = [
        ("lag", C.c_int32),
        ("f_lag", C.c_int32),
        ("skip_repeats", C.c_int32),
        ("reserved", C.c_int32 * 5),
        ("q", C.c_double * 12),
        ("r", C.c_double * 12),
        ("p0", C.c_double * 12),
    ]


class DisturbParams(C.Structure):
    """struct mpcq_disturb_params (include/mpcq.h)."""

    _fields_ = [
        ("alpha", C.c_double * 6),
        ("d_max", C.c_double * 6),
        ("f_lag", C.c_int32),
        ("compensate", C.c_int32),
        ("skip_repeats", C.c_int32),
        ("reserved", C.c_int32 * 5),
    ]


class GaitParams(C.Structure):
    """struct mpcq_gait_params (include/mpcq.h)."""

    _fields_ = [
        ("n_gaits", C.c_int32),
        ("select", C.c_int32),
        ("align", C.c_int32),
        ("reserved0", C.c_int32),
        ("thresholds", C.c_double * 7),
        ("hysteresis", C.c_double),
        ("yaw_weight", C.c_double),
        ("reserved", C.c_double * 5),
    ]


class Robot(C.Structure):
    """struct mpcq_robot (include/mpcq.h): the per-instance constants of a batch."""

    _fields_ = [
        ("mass", C.c_double),
        ("gI", C.c_double * 9),
        ("mu", C.c_double),
        ("fz_max", C.c_double),
        ("reserved", C.c_double * 4),
    ]


class Weights(C.Structure):
    """struct mpcq_weights (include/mpcq.h): the per-instance diagonal of P."""

    _fields_ = [
        ("state", C.c_double * 12),
        ("force", C.c_double),
        ("reserved", C.c_double * 3),
    ]


class Disturbance(C.Structure):
    """struct mpcq_disturbance (include/mpcq.h): the per-instance constant disturbance acceleration."""

    _fields_ = [
        ("a", C.c_double * 6),
        ("reserved", C.c_double * 2),
    ]


def build(force: bool = False) -> str:
    """Compile libmpcq.so for gfx950 with hipcc (csrc/Makefile)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", CSRC], check=True)
    return LIB_PATH


ABI_VERSION = 3  # include/mpcq.h MPCQ_ABI_VERSION these bindings follow
_lib = None
_hip_runtime = None


def hip_runtime_path():
    """The libamdhip64 this process uses: torch's bundled copy when torch is
    installed (whether or not it is imported yet), else the system one."""
    import importlib.util
    import sys
    t = sys.modules.get("torch")
    base = os.path.dirname(t.__file__) if t is not None and getattr(t, "__file__", None) else None
    if base is None:
        spec = importlib.util.find_spec("torch")
        base = os.path.dirname(spec.origin) if spec is not None and spec.origin else None
    if base is not None:
        cand = os.path.join(base, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            return cand
    return None


def _preload_hip_runtime():
    global _hip_runtime
    if _hip_runtime is None:
        path = hip_runtime_path()
        _hip_runtime = C.CDLL(path, mode=C.RTLD_GLOBAL) if path else False
    return _hip_runtime


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpcqError(E_DEVICE, f"{LIB_PATH} is missing: run `make -C {CSRC}` (or __graft_entry__.build())")
    _preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    PP = C.POINTER(Params)
    L.mpcq_abi_version.restype = C.c_int
    L.mpcq_default_params.argtypes = [PP]
    L.mpcq_default_params.restype = None
    L.mpcq_dims.argtypes = [C.c_int, ip, ip, ip]
    L.mpcq_pattern.argtypes = [C.c_int, ip, ip]
    L.mpcq_supported_horizons.argtypes = [ip, C.c_int]
    L.mpcq_last_error.restype = C.c_char_p
    L.mpcq_build_info.restype = C.c_char_p
    L.mpcq_create.argtypes = [C.c_int, C.c_int, PP, C.POINTER(vp)]
    L.mpcq_destroy.argtypes = [vp]
    L.mpcq_set_stream.argtypes = [vp, vp]
    L.mpcq_set_slice.argtypes = [vp, C.c_int32]
    L.mpcq_last_kernel_ms.argtypes = [vp, dp, dp]
    L.mpcq_formulate_batch.argtypes = [vp, C.c_int64, vp, vp, C.c_int, vp, vp, vp, vp, C.c_uint32]
    L.mpcq_qp_solve_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                      vp, C.c_uint32]
    L.mpcq_solve_batch.argtypes = [vp, C.c_int64, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                   vp, C.c_uint32]
    L.mpcq_debug_set_stamps.argtypes = [vp, vp]
    L.mpcq_default_planner_params.argtypes = [C.POINTER(PlannerParams)]
    L.mpcq_default_planner_params.restype = None
    L.mpcq_session_create.argtypes = [vp, C.c_int64, C.POINTER(PlannerParams), vp, C.POINTER(vp)]
    L.mpcq_session_destroy.argtypes = [vp]
    L.mpcq_session_tick.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_uint32]
    L.mpcq_session_read.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_write.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.mpcq_plan_batch.argtypes = [vp, C.POINTER(PlannerParams), C.c_int64, C.c_uint32, C.c_int] + [vp] * 12 + [C.c_uint32]
    L.mpcq_debug_class_table_slots.restype = C.c_int
    L.mpcq_debug_suspended_status.restype = C.c_int
    L.mpcq_debug_class_table_read.argtypes = [vp, vp, vp]
    L.mpcq_debug_class_table_write.argtypes = [vp, vp, vp]
    L.mpcq_debug_class_order.argtypes = [vp, C.c_int64, vp, vp, vp]
    L.mpcq_debug_class_learn.argtypes = [vp, C.c_int64, vp, vp]
    L.mpcq_debug_suspended.argtypes = [vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp]
    L.mpcq_debug_session_order.argtypes = [vp, C.c_int64, vp, vp]
    L.mpcq_debug_last_dispatch.argtypes = [vp, C.POINTER(C.c_int64), ip, ip, vp, vp, vp, ip, vp]
    SP = C.POINTER(SwingParams)
    L.mpcq_default_swing_params.argtypes = [SP]
    L.mpcq_default_swing_params.restype = None
    L.mpcq_swing_step_batch.argtypes = [vp, SP, C.c_int64, vp, vp, vp, C.c_uint32]
    L.mpcq_swing_batch.argtypes = [vp, SP, C.c_int64, C.c_int, C.c_int] + [vp] * 8 + [C.c_uint32]
    L.mpcq_session_enable_swing.argtypes = [vp, SP]
    for name in ("mpcq_swing_step_batch", "mpcq_swing_batch", "mpcq_session_enable_swing"):
        getattr(L, name).restype = C.c_int
    L.mpcq_default_robot.argtypes = [PP, C.POINTER(Robot)]
    L.mpcq_default_robot.restype = None
    L.mpcq_set_robots.argtypes = [vp, C.c_int64, vp, C.c_uint32]
    L.mpcq_session_set_robots.argtypes = [vp, vp, C.c_uint32]
    L.mpcq_session_get_robots.argtypes = [vp, vp, C.c_uint32]
    for name in ("mpcq_set_robots", "mpcq_session_set_robots", "mpcq_session_get_robots"):
        getattr(L, name).restype = C.c_int
    L.mpcq_session_reset.argtypes = [vp, vp, vp, vp, C.c_uint32]
    L.mpcq_session_reset.restype = C.c_int
    PL = C.POINTER(PlantParams)
    L.mpcq_default_plant_params.argtypes = [PL]
    L.mpcq_default_plant_params.restype = None
    L.mpcq_plant_step_batch.argtypes = [vp, PL, C.c_int64] + [vp] * 7 + [C.c_uint32]
    L.mpcq_session_enable_plant.argtypes = [vp, PL]
    L.mpcq_session_disable_plant.argtypes = [vp]
    L.mpcq_default_weights.argtypes = [PP, C.POINTER(Weights)]
    L.mpcq_default_weights.restype = None
    L.mpcq_set_weights.argtypes = [vp, C.c_int64, vp, C.c_uint32]
    L.mpcq_session_set_weights.argtypes = [vp, vp, C.c_uint32]
    L.mpcq_session_get_weights.argtypes = [vp, vp, C.c_uint32]
    for name in ("mpcq_set_weights", "mpcq_session_set_weights", "mpcq_session_get_weights"):
        getattr(L, name).restype = C.c_int
    L.mpcq_set_disturbance.argtypes = [vp, C.c_int64, vp, C.c_uint32]
    L.mpcq_session_set_disturbance.argtypes = [vp, vp, C.c_uint32]
    L.mpcq_session_get_disturbance.argtypes = [vp, vp, C.c_uint32]
    for name in ("mpcq_set_disturbance", "mpcq_session_set_disturbance", "mpcq_session_get_disturbance"):
        getattr(L, name).restype = C.c_int
    DP = C.POINTER(DisturbParams)
    L.mpcq_default_disturb_params.argtypes = [DP]
    L.mpcq_default_disturb_params.restype = None
    L.mpcq_disturb_step_batch.argtypes = [vp, DP, C.c_int64, vp, C.c_int] + [vp] * 8 + [C.c_uint32]
    L.mpcq_session_enable_disturb.argtypes = [vp, DP]
    L.mpcq_session_disable_disturb.argtypes = [vp]
    L.mpcq_session_disturb_read.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_disturb_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    for name in ("mpcq_disturb_step_batch", "mpcq_session_enable_disturb", "mpcq_session_disable_disturb",
                 "mpcq_session_disturb_read", "mpcq_session_disturb_device_ptr"):
        getattr(L, name).restype = C.c_int
    L.mpcq_session_set_plant_robots.argtypes = [vp, vp, C.c_uint32]
    L.mpcq_session_set_wrench.argtypes = [vp, vp, C.c_uint32]
    L.mpcq_session_plant_read.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_plant_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    for name in ("mpcq_plant_step_batch", "mpcq_session_enable_plant", "mpcq_session_disable_plant",
                 "mpcq_session_set_plant_robots", "mpcq_session_set_wrench", "mpcq_session_plant_read",
                 "mpcq_session_plant_device_ptr"):
        getattr(L, name).restype = C.c_int
    MP = C.POINTER(MonitorParams)
    L.mpcq_default_monitor_params.argtypes = [MP]
    L.mpcq_default_monitor_params.restype = None
    L.mpcq_monitor_step_batch.argtypes = [vp, MP, C.c_int64] + [vp] * 14 + [C.c_uint32]
    L.mpcq_session_enable_monitor.argtypes = [vp, MP]
    L.mpcq_session_disable_monitor.argtypes = [vp]
    L.mpcq_session_monitor_read.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_monitor_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.mpcq_session_run.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_uint32]
    for name in ("mpcq_monitor_step_batch", "mpcq_session_enable_monitor", "mpcq_session_disable_monitor",
                 "mpcq_session_monitor_read", "mpcq_session_monitor_device_ptr", "mpcq_session_run"):
        getattr(L, name).restype = C.c_int
    CP = C.POINTER(ScenarioParams)
    L.mpcq_default_scenario_params.argtypes = [CP]
    L.mpcq_default_scenario_params.restype = None
    L.mpcq_scenario_step_batch.argtypes = [vp, CP, C.c_int64, vp, C.c_int] + [vp] * 9 + [C.c_uint32]
    L.mpcq_session_enable_scenario.argtypes = [vp, CP]
    L.mpcq_session_disable_scenario.argtypes = [vp]
    L.mpcq_session_scenario_read.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_scenario_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    for name in ("mpcq_scenario_step_batch", "mpcq_session_enable_scenario", "mpcq_session_disable_scenario",
                 "mpcq_session_scenario_read", "mpcq_session_scenario_device_ptr"):
        getattr(L, name).restype = C.c_int
    HP = C.POINTER(ChannelParams)
    L.mpcq_default_channel_params.argtypes = [HP]
    L.mpcq_default_channel_params.restype = None
    L.mpcq_channel_observe_batch.argtypes = [vp, HP, C.c_int64, vp, C.c_int] + [vp] * 6 + [C.c_uint32]
    L.mpcq_channel_actuate_batch.argtypes = [vp, HP, C.c_int64] + [vp] * 5 + [C.c_uint32]
    L.mpcq_session_enable_channel.argtypes = [vp, HP]
    L.mpcq_session_disable_channel.argtypes = [vp]
    L.mpcq_session_channel_read.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_channel_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    for name in ("mpcq_channel_observe_batch", "mpcq_channel_actuate_batch", "mpcq_session_enable_channel",
                 "mpcq_session_disable_channel", "mpcq_session_channel_read", "mpcq_session_channel_device_ptr"):
        getattr(L, name).restype = C.c_int
    EP = C.POINTER(EstimatorParams)
    L.mpcq_default_estimator_params.argtypes = [EP]
    L.mpcq_default_estimator_params.restype = None
    L.mpcq_estimator_step_batch.argtypes = [vp, EP, C.c_int64, vp, C.c_int] + [vp] * 7 + [C.c_uint32]
    L.mpcq_session_enable_estimator.argtypes = [vp, EP]
    L.mpcq_session_disable_estimator.argtypes = [vp]
    L.mpcq_session_estimator_read.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_estimator_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    for name in ("mpcq_estimator_step_batch", "mpcq_session_enable_estimator", "mpcq_session_disable_estimator",
                 "mpcq_session_estimator_read", "mpcq_session_estimator_device_ptr"):
        getattr(L, name).restype = C.c_int
    GP = C.POINTER(GaitParams)
    L.mpcq_default_gait_params.argtypes = [GP]
    L.mpcq_default_gait_params.restype = None
    L.mpcq_gait_roll_batch.argtypes = [vp, GP, vp, C.c_int64, vp, vp, vp, C.c_uint32]
    L.mpcq_session_enable_gait.argtypes = [vp, GP, vp]
    L.mpcq_session_disable_gait.argtypes = [vp]
    L.mpcq_session_set_gait.argtypes = [vp, vp, C.c_uint32]
    L.mpcq_session_gait_read.argtypes = [vp, C.c_int, vp, C.c_uint32]
    L.mpcq_session_gait_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    for name in ("mpcq_gait_roll_batch", "mpcq_session_enable_gait", "mpcq_session_disable_gait",
                 "mpcq_session_set_gait", "mpcq_session_gait_read", "mpcq_session_gait_device_ptr"):
        getattr(L, name).restype = C.c_int
    L.mpcq_session_snapshot_create.argtypes = [vp, C.POINTER(vp)]
    L.mpcq_session_snapshot_destroy.argtypes = [vp]
    L.mpcq_session_snapshot_save.argtypes = [vp, vp, C.c_uint32]
    L.mpcq_session_snapshot_restore.argtypes = [vp, vp, vp, C.c_uint32]
    L.mpcq_session_fork.argtypes = [vp, vp, C.c_uint32]
    L.mpcq_session_snapshot_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.mpcq_session_snapshot_export.argtypes = [vp, vp, C.c_int64]
    L.mpcq_session_snapshot_import.argtypes = [vp, vp, vp, C.c_int64]
    L.mpcq_debug_gather_rows.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int64, C.c_int64, vp, C.c_uint32]
    for name in ("mpcq_session_snapshot_create", "mpcq_session_snapshot_destroy", "mpcq_session_snapshot_save",
                 "mpcq_session_snapshot_restore", "mpcq_session_fork", "mpcq_session_snapshot_bytes",
                 "mpcq_session_snapshot_export", "mpcq_session_snapshot_import", "mpcq_debug_gather_rows"):
        getattr(L, name).restype = C.c_int
    for name in ("mpcq_debug_class_table_read", "mpcq_debug_class_table_write", "mpcq_debug_class_order",
                 "mpcq_debug_class_learn", "mpcq_debug_suspended", "mpcq_debug_session_order",
                 "mpcq_debug_last_dispatch"):
        getattr(L, name).restype = C.c_int
    for name in ("mpcq_dims", "mpcq_pattern", "mpcq_supported_horizons", "mpcq_create",
                 "mpcq_destroy", "mpcq_set_stream", "mpcq_set_slice", "mpcq_last_kernel_ms", "mpcq_formulate_batch",
                 "mpcq_qp_solve_batch", "mpcq_solve_batch", "mpcq_default_planner_params",
           "mpcq_plan_batch", "mpcq_session_create", "mpcq_session_destroy", "mpcq_session_tick",
           "mpcq_session_read", "mpcq_session_write", "mpcq_session_device_ptr", "mpcq_debug_set_stamps"):
        getattr(L, name).restype = C.c_int
    if L.mpcq_abi_version() != ABI_VERSION:
        raise MpcqError(E_UNSUPPORTED, f"{LIB_PATH} has ABI {L.mpcq_abi_version()}, these bindings ABI {ABI_VERSION}: "
                        f"rebuild it (`make -C {CSRC}`)")
    _lib = L
    return L


def check(rc: int):
    if rc != OK:
        msg = lib().mpcq_last_error()
        raise MpcqError(rc, msg.decode() if msg else "")
    return rc


def default_params(**overrides) -> Params:
    p = Params()
    lib().mpcq_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown parameter {k}")
        setattr(p, k, v)
    return p


def default_planner_params(**overrides) -> PlannerParams:
    p = PlannerParams()
    lib().mpcq_default_planner_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown planner parameter {k}")
        setattr(p, k, v)
    return p


def default_swing_params(**overrides) -> SwingParams:
    p = SwingParams()
    lib().mpcq_default_swing_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown swing parameter {k}")
        setattr(p, k, v)
    return p


def default_plant_params(**overrides) -> PlantParams:
    p = PlantParams()
    lib().mpcq_default_plant_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown plant parameter {k}")
        setattr(p, k, v)
    return p


def default_monitor_params(**overrides) -> MonitorParams:
    p = MonitorParams()
    lib().mpcq_default_monitor_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown monitor parameter {k}")
        setattr(p, k, v)
    return p


def default_scenario_params(**overrides) -> ScenarioParams:
    """mpcq_default_scenario_params; an array field takes a sequence of its length."""
    p = ScenarioParams()
    lib().mpcq_default_scenario_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown scenario parameter {k}")
        cur = getattr(p, k)
        if hasattr(cur, "__len__"):
            v = list(v)
            if len(v) != len(cur):
                raise ValueError(f"scenario parameter {k} takes {len(cur)} values")
            v = type(cur)(*v)
        setattr(p, k, v)
    return p


def default_weights(params: Params | None = None) -> Weights:
    """mpcq_default_weights: state_weights and force_weight of ``params`` (None: the defaults)."""
    w = Weights()
    lib().mpcq_default_weights(C.byref(params) if params is not None else None, C.byref(w))
    return w


def default_robot(params: Params | None = None) -> Robot:
    """mpcq_default_robot: mass, gI, mu, fz_max of ``params`` (None: the defaults)."""
    r = Robot()
    lib().mpcq_default_robot(C.byref(params) if params is not None else None, C.byref(r))
    return r


def build_info() -> dict:
    """The loaded library's build stamp (mpcq_build_info): {"src_sha256": ..., "arch": ...}."""
    raw = lib().mpcq_build_info().decode()
    return dict(kv.split("=", 1) for kv in raw.split() if "=" in kv)


def source_sha(csrc: str = CSRC) -> str:
    """The stamp a default `make` gives the sources in ``csrc`` (csrc/stamp.py: sha256 over
    the HIP sources, the assembly pass, the Makefile, the headers, the C++ units and the
    Makefile's default flags; first 16 hex digits)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mpcq_stamp", os.path.join(csrc, "stamp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.stamp(csrc)


def supported_horizons():
    buf = (C.c_int32 * 64)()
    n = lib().mpcq_supported_horizons(buf, 64)
    return [buf[i] for i in range(min(n, 64))]


def default_channel_params(**overrides) -> ChannelParams:
    """mpcq_default_channel_params (all zero: a channel that changes nothing); an array field
    takes a sequence of its length, or one number for every entry."""
    p = ChannelParams()
    lib().mpcq_default_channel_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown channel parameter {k}")
        cur = getattr(p, k)
        if hasattr(cur, "__len__"):
            v = [v] * len(cur) if not hasattr(v, "__len__") else list(v)
            if len(v) != len(cur):
                raise ValueError(f"channel parameter {k} takes {len(cur)} values")
            v = type(cur)(*v)
        setattr(p, k, v)
    return p


def default_estimator_params(**overrides) -> EstimatorParams:
    """mpcq_default_estimator_params (lag 0, f_lag 0, skip_repeats 1, p0 1e-2, q 1e-6 / 1e-4,
    r 1e-4: starting values, not tuned); an array field takes a sequence of its length, or one
    number for every entry."""
    p = EstimatorParams()
    lib().mpcq_default_estimator_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown estimator parameter {k}")
        cur = getattr(p, k)
        if hasattr(cur, "__len__"):
            v = [v] * len(cur) if not hasattr(v, "__len__") else list(v)
            if len(v) != len(cur):
                raise ValueError(f"estimator parameter {k} takes {len(cur)} values")
            v = type(cur)(*v)
        setattr(p, k, v)
    return p


def default_disturb_params(**overrides) -> DisturbParams:
    """mpcq_default_disturb_params (alpha 0.2, d_max 5 m/s^2 and 30 rad/s^2, f_lag 0, compensate 1,
    skip_repeats 1: starting values, not tuned); an array field takes a sequence of its length,
    or one number for every entry."""
    p = DisturbParams()
    lib().mpcq_default_disturb_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown disturb parameter {k}")
        cur = getattr(p, k)
        if hasattr(cur, "__len__"):
            v = [v] * len(cur) if not hasattr(v, "__len__") else list(v)
            if len(v) != len(cur):
                raise ValueError(f"disturb parameter {k} takes {len(cur)} values")
            v = type(cur)(*v)
        setattr(p, k, v)
    return p


def default_gait_params(**overrides) -> GaitParams:
    """mpcq_default_gait_params (n_gaits 0: to be set; GAIT_MANUAL, align 1, thresholds all +inf,
    hysteresis 0, yaw_weight = the default shoulders' distance from the centre); ``thresholds``
    takes up to 7 values (the rest stay +inf), ``reserved`` a sequence of its length."""
    p = GaitParams()
    lib().mpcq_default_gait_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"unknown gait parameter {k}")
        cur = getattr(p, k)
        if hasattr(cur, "__len__"):
            v = [v] * len(cur) if not hasattr(v, "__len__") else list(v)
            if k == "thresholds" and len(v) < len(cur):
                v = v + [float("inf")] * (len(cur) - len(v))
            if len(v) != len(cur):
                raise ValueError(f"gait parameter {k} takes {len(cur)} values")
            v = type(cur)(*v)
        setattr(p, k, v)
    return p
