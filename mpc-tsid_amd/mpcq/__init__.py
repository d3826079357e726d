"""mpcq — MI355X-native batched convex-MPC QP engine (the MPC.py hot path of
thomascbrs/mpc-tsid).  See DESIGN.md.

Public surface:
  Engine            batched formulate / qp_solve / solve over libmpcq.so
  default_params    reference constants + OSQP 0.6 settings (MPC.py:25-39, 414-416)
  pattern, dims     CSC pattern / sizes of MPC.create_ML
  Engine.plan       batched FootstepPlanner (roll / compute_footsteps / getRefStates)
  Session           B robots in closed loop, all per-tick state resident in HBM
                    (Session.reset: any subset of them back to their initial state)
  robots            per-robot mass / inertia / friction / force limit tables
                    (Engine.set_robots, Session.set_robots)
  weights           per-instance cost weights, the diagonal of P (Engine.set_weights,
                    Session.set_weights): a tuning sweep in one launch
  disturbances      per-instance constant disturbance accelerations in the model's dynamics
                    (Engine.set_disturbance, Session.set_disturbance): pushes sampled over one
                    state in one launch, a known payload or bias compensated
  Swing             batched swing-foot trajectories between two ticks (Session.enable_swing)
  Plant             batched rigid-body plant under the stance feet's forces: true robots that
                    differ from the model, external pushes (Session.enable_plant)
  Monitor           episodes on the device: per-robot termination, episode statistics, batch
                    totals (Session.enable_monitor: auto-reset; Session.run: whole rollouts
                    with a per-tick trace)
  Scenario          per-episode random commands, pushes and payloads drawn on the device from a
                    counter-based generator (Session.enable_scenario); mpcq.scenario restates
                    the draws on the host, bit for bit
  Channel           what lies between plant and controller, on the device: delayed, biased, noisy
                    state feedback with dropped frames in front of the planner, delayed, scaled,
                    noisy forces in front of the plant (Session.enable_channel); mpcq.channel
                    restates the draws on the host, bit for bit
  Disturb           a per-robot disturbance observer in front of the solve: the acceleration the
                    controller's model lacks (an unknown payload, a steady push), estimated from
                    consecutive states and handed to the solve (Session.enable_disturb)
  Estimator         the controller's side of the channel, on the device: a per-robot Kalman filter
                    on the MPC's own model that compensates the measurement's delay through the
                    recorded forces and footholds (Session.enable_estimator)
  Gait              gait transitions on the device: per-robot target gaits from a small library of
                    gait cycles, switched at phase boundaries by request or by the commanded
                    speed; the step that enters the horizon comes from the desired cycle
                    (Session.enable_gait, Session.set_gait); mpcq.gait.cycle builds the cycles
  Snapshot          a session's robots saved on the device (Session.snapshot): restore them, seed
                    another session from them, branch one robot into many (Session.restore,
                    Session.fork), checkpoint them to the host (Snapshot.tobytes,
                    Session.snapshot_from)
  synth             seeded synthetic inputs shaped like FootstepPlanner's
"""
from . import synth  # noqa: F401
from ._lib import (FLAG_ASYNC, FLAG_DEVICE_PTRS, FLAG_ORDER_BY_CLASS, MODE_SETUP, MODE_UPDATE,  # noqa: F401
                   PLAN_FOOTSTEPS, PLAN_REFSTATES, PLAN_ROLL, PLAN_TICK, PlannerParams,
                   default_planner_params, STATUS_BAD_GAIT, SV_COST, SV_F0, SV_FSTEPS, SV_GAIT,
                   SV_H_ROT, SV_ITERS, SV_ORDER, SV_FIRST, SV_L_FEET, SV_Q_W, SV_RHO, SV_ROT_FLAG, SV_STATE, SV_STATUS, SV_X,
                   SV_X_ROBOT, SV_XREF, SV_Y, STATUS_FACTOR_FAILED, STATUS_MAX_ITER_REACHED,
                   STATUS_NONFINITE, STATUS_SOLVED, STATUS_SOLVED_INACCURATE, STATUS_PRIMAL_INFEASIBLE,
                   STATUS_DUAL_INFEASIBLE, STATUS_PRIMAL_INFEASIBLE_INACCURATE,
                   STATUS_DUAL_INFEASIBLE_INACCURATE, STATUS_BAD_BOUNDS, MpcqError,
                   Params, build, build_info, default_params, lib, source_sha, supported_horizons,
                   SV_FRAME, SV_SWING_REF, SV_SWING_STATE, SWING_STATE, SwingParams, default_swing_params,
                   Robot, default_robot, Weights, default_weights, Disturbance,
                   PLANT_MODEL, PLANT_RIGID, PV_F_EFF, PV_STATE_END, PV_WRENCH, PlantParams, default_plant_params,
                   DONE_HEIGHT, DONE_NONFINITE, DONE_SOLVER, DONE_TILT, DONE_TIMEOUT, MV_DONE, MV_EP, MV_EP_TICKS,
                   MV_EPISODES, MV_LAST, MV_TOTALS, TRACE, MonitorParams, default_monitor_params,
                   CV_DRAW, CV_EPOCH, CV_PUSH, CV_ROBOTS, CV_TICK, CV_V_REF, CV_WRENCH, ScenarioParams,
                   default_scenario_params,
                   HV_CLOCK, HV_DRAW, HV_F_CMD, HV_F_RING, HV_OBS, HV_S_RING, CHANNEL_MAX_DELAY,
                   CHANNEL_MAX_LATENCY, ChannelParams, default_channel_params,
                   EV_EST, EV_ROW, EST_CLOCK, EST_P, EST_POST, EST_PREV, EST_RING, EST_ROW, EST_SLOTS,
                   ESTIMATOR_MAX_F_LAG, ESTIMATOR_MAX_LAG, EstimatorParams, default_estimator_params,
                   DV_DIST, DV_ROW, DV_RESID, DIST_D, DIST_PREV, DIST_CLOCK, DIST_RING, DIST_SLOTS, DIST_ROW,
                   DISTURB_MAX_F_LAG, DisturbParams, default_disturb_params,
                   GV_STATE, GAIT_MAX, GAIT_MANUAL, GAIT_BY_SPEED, GaitParams, default_gait_params)
from . import channel  # noqa: F401
from .channel import Channel  # noqa: F401
from . import estimator  # noqa: F401
from .estimator import Estimator  # noqa: F401
from . import disturb  # noqa: F401
from .disturb import Disturb  # noqa: F401
from . import gait  # noqa: F401
from .gait import Gait  # noqa: F401
from .engine import (DISTURBANCE_DTYPE, ROBOT_DTYPE, WEIGHTS_DTYPE, Engine, dims, disturbances, pattern,  # noqa: F401
                     robots, weights)
from .monitor import Monitor  # noqa: F401
from .plant import Plant  # noqa: F401
from . import scenario  # noqa: F401
from .scenario import Scenario  # noqa: F401
from .session import Session, Snapshot  # noqa: F401
from .swing import Swing  # noqa: F401

__version__ = "0.1.0"
