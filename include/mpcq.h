/*
 * mpcq.h — C ABI of the MI355X-native batched convex-MPC QP engine (libmpcq.so).
 *
 * Drop-in boundary for the hot path of thomascbrs/mpc-tsid: the QP formulation
 * in MPC.py and its OSQP solve.  Every entry point below names the reference
 * interface it replaces (file:line in the reference tree).  Plain C types only:
 * pointers + sizes, no torch / HIP types in the signatures.
 *
 * Problem (per instance, horizon N, MPC.py:98-288):
 *   x = [X_1..X_N (12 each), f_0..f_{N-1} (12 each)]     n = 24N variables
 *   rows: 12N dynamics | 12N swing mask | 20N friction    m = 44N constraints
 *   min 1/2 x'Px   s.t.  l <= A x <= u     (P diagonal, q = 0)
 * A is CSC with the fixed sparsity pattern of MPC.create_ML (nnz = 126N-18).
 *
 * Layouts (all C-order / row-major, float64):
 *   xref    [B][12][N+1]   column 0 = current state (MPC.py:466-467)
 *   fsteps  [B][20][13]    col 0 = phase duration, then foot xyz (NaN = swing)
 *   Ax      [B][nnz]       CSC data, pattern from mpcq_pattern()
 *   l, u    [B][m]
 *   x       [B][n], y [B][m], f0 [B][12]
 *
 * Conventions: functions return 0 on success, a negative MPCQ_E* code on an
 * API error (message via mpcq_last_error()).  Per-instance outcomes are
 * reported through the status array (OSQP codes, see MPCQ_STATUS_*).
 * Inputs are never mutated.  Calls are blocking unless MPCQ_FLAG_ASYNC.
 */
#ifndef MPCQ_H
#define MPCQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI changelog:
 *   2: eps_prim_inf / eps_dual_inf, dual_warm, infeasibility statuses
 *   3: info[b][3] = the ADMM's own exit status (before polish; was always 0),
 *      MPCQ_SV_ORDER added (MPCQ_SV_COUNT 16 -> 17), initialised to the identity
 *   3 (additions, no bump): mpcq_debug_class_table_slots / _read / _write, mpcq_debug_class_order,
 *      mpcq_debug_class_learn, mpcq_debug_suspended_status, mpcq_debug_suspended,
 *      mpcq_debug_session_order, mpcq_debug_last_dispatch (diagnostics);
 *      MPCQ_SLICE16 in the environment no longer slices a library compiled without it
 *   3 (additions, no bump): mpcq_default_swing_params, mpcq_swing_step_batch, mpcq_swing_batch,
 *      mpcq_session_enable_swing; MPCQ_SV_SWING_REF / _SWING_STATE / _FRAME (MPCQ_SV_COUNT
 *      17 -> 20; MPCQ_E_INVALID on a session that has not enabled swing)
 *   3 (additions, no bump): mpcq_robot, mpcq_default_robot, mpcq_set_robots,
 *      mpcq_session_set_robots, mpcq_session_get_robots (per-instance mass, gI, mu, fz_max)
 *   3 (additions, no bump): mpcq_weights, mpcq_default_weights, mpcq_set_weights,
 *      mpcq_session_set_weights, mpcq_session_get_weights (per-instance diagonal of P)
 *   3 (additions, no bump): mpcq_session_reset (any subset of a session's robots back to their
 *      state after create, between two ticks); MPCQ_SV_FIRST (MPCQ_SV_COUNT 20 -> 21, read-only)
 *   3 (additions, no bump): mpcq_plant_params, mpcq_default_plant_params, mpcq_plant_step_batch,
 *      mpcq_session_enable_plant / _disable_plant / _set_plant_robots / _set_wrench /
 *      _plant_read / _plant_device_ptr (a rigid-body plant between two ticks); its arrays have
 *      ids of their own, MPCQ_PV_*: MPCQ_SV_COUNT stays 21
 *   3 (additions, no bump): mpcq_monitor_params, mpcq_default_monitor_params,
 *      mpcq_monitor_step_batch, mpcq_session_enable_monitor / _disable_monitor / _monitor_read /
 *      _monitor_device_ptr, mpcq_session_run (episodes: on-device termination, statistics,
 *      auto-reset, multi-tick rollouts); the monitor's arrays have ids of their own, MPCQ_MV_*:
 *      MPCQ_SV_COUNT stays 21
 *   3 (additions, no bump): mpcq_scenario_params, mpcq_default_scenario_params,
 *      mpcq_scenario_step_batch, mpcq_session_enable_scenario / _disable_scenario /
 *      _scenario_read / _scenario_device_ptr (per-episode random commands, pushes and payloads
 *      drawn on the device); its arrays have ids of their own, MPCQ_CV_*; with a scenario that
 *      commands, mpcq_session_tick and mpcq_session_run accept v_ref == NULL
 *   3 (additions, no bump): mpcq_snapshot, mpcq_session_snapshot_create / _destroy / _save /
 *      _restore / _bytes / _export / _import, mpcq_session_fork, mpcq_debug_gather_rows (save,
 *      restore and branch a session's robots on the device); no new array id: MPCQ_SV_COUNT
 *      stays 21
 *   3 (additions, no bump): mpcq_channel_params, mpcq_default_channel_params,
 *      mpcq_channel_observe_batch, mpcq_channel_actuate_batch, mpcq_session_enable_channel /
 *      _disable_channel / _channel_read / _channel_device_ptr (noisy, delayed, biased state
 *      feedback in front of the planner; delayed, scaled, noisy forces in front of the plant);
 *      its arrays have ids of their own, MPCQ_HV_*: MPCQ_SV_COUNT stays 21.  A snapshot of a
 *      session with a channel writes blob format version 2 (one more part); one without writes
 *      version 1 as before, and import reads both
 *   3 (additions, no bump): mpcq_gait_params, mpcq_default_gait_params, mpcq_gait_roll_batch,
 *      mpcq_session_enable_gait / _disable_gait / _set_gait / _gait_read / _gait_device_ptr
 *      (per-robot target gaits: the step that enters the horizon comes from a desired gait
 *      cycle); its array has an id of its own, MPCQ_GV_STATE: MPCQ_SV_COUNT stays 21.  A
 *      snapshot of a session with the gait array writes blob format version 4 (a 144-byte
 *      header, one more part); one without writes what it wrote before, and import reads all
 *   3 (additions, no bump): mpcq_disturbance, mpcq_set_disturbance,
 *      mpcq_session_set_disturbance, mpcq_session_get_disturbance (a per-instance constant
 *      disturbance acceleration in the model's dynamics)
 *   3 (additions, no bump): mpcq_disturb_params, mpcq_default_disturb_params,
 *      mpcq_disturb_step_batch, mpcq_session_enable_disturb / _disable_disturb / _disturb_read /
 *      _disturb_device_ptr (a disturbance observer in front of the solve); its arrays have ids
 *      of their own, MPCQ_DV_*: MPCQ_SV_COUNT stays 21.  A snapshot of a session with those
 *      arrays writes blob format version 5 (a 160-byte header, one more part); one without
 *      writes what it wrote before, and import reads all */
#define MPCQ_ABI_VERSION 3

/* error codes (return values) */
#define MPCQ_OK 0
#define MPCQ_E_INVALID (-1)   /* bad argument */
#define MPCQ_E_DEVICE (-2)    /* HIP runtime error */
#define MPCQ_E_NOMEM (-3)     /* allocation failed */
#define MPCQ_E_UNSUPPORTED (-4) /* horizon N not compiled in */

/* per-instance status (OSQP 0.6 status values, plus formulation errors) */
#define MPCQ_STATUS_SOLVED 1
#define MPCQ_STATUS_SOLVED_INACCURATE 2
#define MPCQ_STATUS_PRIMAL_INFEASIBLE_INACCURATE 3
#define MPCQ_STATUS_DUAL_INFEASIBLE_INACCURATE 4
#define MPCQ_STATUS_MAX_ITER_REACHED (-2)
#define MPCQ_STATUS_PRIMAL_INFEASIBLE (-3)  /* OSQP 0.6 is_primal_infeasible: x, y, f0 are NaN */
#define MPCQ_STATUS_DUAL_INFEASIBLE (-4)    /* OSQP 0.6 is_dual_infeasible: x, y, f0 are NaN */
#define MPCQ_STATUS_NONFINITE (-10)      /* NaN/Inf reached the solver */
#define MPCQ_STATUS_BAD_GAIT (-11)       /* fsteps durations: no terminator / sum != N / NaN */
#define MPCQ_STATUS_FACTOR_FAILED (-12)  /* KKT block lost positive definiteness */
#define MPCQ_STATUS_BAD_BOUNDS (-13)     /* some l > u: osqp's setup / update reject the data
                                            (the python wrapper raises ValueError); no solve */

/* flags */
#define MPCQ_FLAG_DEVICE_PTRS 1u  /* every array argument is a device pointer on ctx's device */
#define MPCQ_FLAG_ASYNC 2u        /* do not synchronise the stream before returning (device ptrs only) */
/* mpcq_solve_batch only: dispatch the instances in the order of the mean iteration count
 * their gait class (the set of contact masks of their fsteps phases) has shown in this
 * context's earlier launches with this flag, the most expensive first (index order inside
 * a class and before any launch); the launch then adds its own counts.  Scheduling only:
 * every result is bit-identical with and without it.  No reference counterpart (the
 * reference solves one QP per tick). */
#define MPCQ_FLAG_ORDER_BY_CLASS 4u

/* formulation mode (MPC.py:491-494) */
#define MPCQ_MODE_UPDATE 0  /* k > 0: update_ML/update_NK with fsteps footholds */
#define MPCQ_MODE_SETUP 1   /* k == 0: create_ML/create_NK with the default footholds */

/*
 * Parameters.  mpcq_default_params() fills the reference constants:
 * dt 0.02, mass 2.50000279 (MPC.py:28), inertia gI (MPC.py:35-37), mu 0.9
 * (MPC.py:39), fz_max 25 (MPC.py:228), g 9.81 (MPC.py:201), state weights
 * (MPC.py:255-266), force weight 1e-5 (MPC.py:273-275), default footholds
 * (MPC.py:67-70) and the OSQP 0.6 settings used by MPC.py:414-416
 * (eps_abs = eps_rel = 1e-7, every other setting at the library default).
 */
typedef struct mpcq_params {
  /* --- formulation --- */
  double dt;
  double mass;
  double gI[9];             /* row-major 3x3 body inertia */
  double mu;
  double fz_max;
  double gravity;
  double state_weights[12]; /* P diagonal for [pos, rpy, linvel, angvel] */
  double force_weight;      /* P diagonal for every force component */
  double footholds[12];     /* default footholds, row-major 3x4 (setup mode) */
  /* --- OSQP settings --- */
  double rho;               /* 0.1 */
  double sigma;             /* 1e-6 */
  double alpha;             /* 1.6 */
  double eps_abs;           /* 1e-7 */
  double eps_rel;           /* 1e-7 */
  double adaptive_rho_tolerance; /* 5 */
  double delta;             /* polish regularisation 1e-6 */
  double eps_prim_inf;      /* 1e-4: primal infeasibility tolerance (OSQP 0.6 default) */
  double eps_dual_inf;      /* 1e-4: dual infeasibility tolerance (OSQP 0.6 default) */
  int32_t max_iter;         /* 4000 */
  int32_t check_termination;/* 25 */
  int32_t adaptive_rho;     /* 1 */
  int32_t adaptive_rho_interval; /* 100 = OSQP's non-timed rule (4 x check_termination) */
  int32_t scaling;          /* 10 Ruiz iterations */
  int32_t polish;           /* 0 off (OSQP default); 1 after SOLVED (OSQP); 2 also after
                               SOLVED_INACCURATE / MAX_ITER (status upgraded if it then meets eps) */
  int32_t polish_refine_iter; /* 3 */
  int32_t polish_rounds;    /* 1 = OSQP's single active-set guess; >1 iterates the
                               guess (primal-dual active set) until it repeats */
  int32_t dual_warm;        /* how warm_y / y are read and written (MPC.py:419-420):
                               0: osqp's unscaled duals (warm_start(y=) in, results.y out);
                               1: the solver's scaled workspace y, carried as is across the
                                  re-scaled update(Ax=) + warm_start(x=) of the next tick --
                                  what osqp 0.6 does between the reference's ticks */
  int32_t reserved[7];
} mpcq_params;

typedef struct mpcq_ctx mpcq_ctx;

/* ---- metadata / pattern -------------------------------------------------- */
int mpcq_abi_version(void);
void mpcq_default_params(mpcq_params* p);
/* Dimensions for horizon N: n = 24N, m = 44N, nnz = 126N - 18. */
int mpcq_dims(int n_steps, int32_t* n, int32_t* m, int32_t* nnz);
/* CSC pattern of MPC.create_ML (MPC.py:98-151): indptr[n+1], indices[nnz]. */
int mpcq_pattern(int n_steps, int32_t* indptr, int32_t* indices);
/* Horizons compiled into the HIP engine (writes up to cap values). */
int mpcq_supported_horizons(int32_t* out, int cap);
const char* mpcq_last_error(void);
/* Build stamp of this library (no reference counterpart: provenance for profiles):
 * "src_sha256=<16 hex> arch=gfx950", the hex the first 16 of sha256 over the csrc .hip files,
 * the assembly pass, the Makefile, the headers, the .cpp units and the effective compiler
 * flags (csrc/stamp.py); the stamps build appends "+stamps", an experiment variant
 * "+exp:<name>:<hash>" (tools/build_variant.sh).  bench.py drops a committed PMC figure
 * whose stamp differs from the running library's. */
const char* mpcq_build_info(void);

/* ---- context --------------------------------------------------------------
 * Replaces MPC.MPC(dt, n_steps, T_gait) (MPC.py:22-82) + osqp.OSQP() (MPC.py:73).
 * One context per (device, host thread).  The context owns device scratch. */
int mpcq_create(int device, int n_steps, const mpcq_params* params, mpcq_ctx** out);
int mpcq_destroy(mpcq_ctx* ctx);
/* HIP stream (hipStream_t passed as void*) for subsequent launches; NULL = ctx's own stream. */
int mpcq_set_stream(mpcq_ctx* ctx, void* stream);
/* Device time of the last launch of each kernel (ms, hipEvent timing on ctx's stream; a
 * sliced solve: from its first slice's start to its last slice's end). */
int mpcq_last_kernel_ms(mpcq_ctx* ctx, double* formulate_ms, double* solve_ms);
/* Sliced batch solves (no reference counterpart: a dispatch policy, no result changes).
 * slice_iters > 0: beyond 16 stages, the batch solves of this context (mpcq_solve_batch,
 * mpcq_qp_solve_batch) run as two launches: the first suspends every instance still iterating
 * at the first ADMM segment end (check / adaptive-rho / max_iter boundary) after slice_iters
 * iterations and saves its iterate in device scratch; the second resumes the suspended ones
 * (formulation, scaling and the factorisation at the saved rho recomputed), the farthest from
 * convergence (the iterations left, extrapolated from the residuals' decay) first, to their
 * end.  Every output is bit-identical to the unsliced solve's; long instances no longer hold a CU slot
 * past the others and start first once known, so a batch whose instances fill the CUs in
 * several rounds ends sooner.  No host synchronisation: the second
 * launch reads its workgroup count on the device (MPCQ_FLAG_ASYNC holds).  0 (the default), a
 * slice of max_iter or more, and horizons up to 16: one launch. */
int mpcq_set_slice(mpcq_ctx* ctx, int32_t slice_iters);

/* ---- per-robot constants ----------------------------------------------------
 * No reference counterpart (the reference is one robot): the four physical constants of
 * mpcq_params that may differ between the instances of one batch.  The diagonal of P
 * (state_weights, force_weight) has a table of its own, mpcq_weights below.  Every other
 * field (dt, gravity, footholds, OSQP settings) shapes the horizon's meaning, the scaling or
 * the loop counters and stays per context. */
typedef struct mpcq_robot {      /* 16 doubles = 128 bytes */
  double mass;      /* > 0 */
  double gI[9];     /* row-major 3x3, as mpcq_params.gI */
  double mu;        /* > 0 */
  double fz_max;    /* > 0 */
  double reserved[4];            /* zero */
} mpcq_robot;
#ifdef __cplusplus
static_assert(sizeof(mpcq_robot) == 128, "mpcq_robot is 16 doubles");
#else
_Static_assert(sizeof(mpcq_robot) == 128, "mpcq_robot is 16 doubles");
#endif
/* mass, gI, mu, fz_max of p (NULL = mpcq_default_params), reserved zero. */
void mpcq_default_robot(const mpcq_params* p, mpcq_robot* r);
/* Copies robots [count] into memory the context owns: from a host pointer the call blocks;
 * with MPCQ_FLAG_DEVICE_PTRS the copy is device to device on ctx's stream.  In every later
 * mpcq_formulate_batch and mpcq_solve_batch of ctx (both formulation modes, sliced and
 * class-ordered solves included) instance b takes those four quantities from robots[b] --
 * b is the instance index, whatever order the workgroups are dispatched in -- and everything
 * else from ctx's mpcq_params.  count == 0 or robots == NULL clears the table (the context's
 * mpcq_params again).  While a table is set, a launch with batch > count returns
 * MPCQ_E_INVALID and launches nothing.
 * A host table is validated: mass, mu, fz_max finite and > 0, every gI entry finite, reserved
 * zero; otherwise MPCQ_E_INVALID (the message names the first offending index and field) and
 * the table in force stays, as it does when the memory for a larger table cannot be
 * allocated (MPCQ_E_NOMEM).  A device table is not validated: its values are the caller's
 * responsibility; a NaN among them reaches the constraint values and ends as
 * MPCQ_STATUS_NONFINITE through the solver's non-finite check.
 * mpcq_qp_solve_batch is untouched by the table: its caller has formulated already, and P
 * comes from the context. */
int mpcq_set_robots(mpcq_ctx* ctx, int64_t count, const mpcq_robot* robots, uint32_t flags);

/* ---- per-instance cost weights ------------------------------------------------
 * No reference counterpart (the reference is one controller): the 13 numbers of P's diagonal,
 * so that every instance of a batch, and every robot of a session, may carry its own tuning. */
typedef struct mpcq_weights {    /* 16 doubles = 128 bytes */
  double state[12];  /* as mpcq_params.state_weights, each > 0 */
  double force;      /* as mpcq_params.force_weight, > 0 */
  double reserved[3];            /* zero */
} mpcq_weights;
#ifdef __cplusplus
static_assert(sizeof(mpcq_weights) == 128, "mpcq_weights is 16 doubles");
#else
_Static_assert(sizeof(mpcq_weights) == 128, "mpcq_weights is 16 doubles");
#endif
/* state_weights and force_weight of p (NULL = mpcq_default_params), reserved zero.  A NULL w
 * is ignored. */
void mpcq_default_weights(const mpcq_params* p, mpcq_weights* w);
/* Copies weights [count] into memory the context owns: from a host pointer the call blocks;
 * with MPCQ_FLAG_DEVICE_PTRS the copy is device to device on ctx's stream, behind the
 * launches that still read the table it replaces.  In every later mpcq_solve_batch of ctx
 * (both formulation modes, polish, sliced and class-ordered solves included) instance b takes
 * the diagonal of P from weights[b] -- b is the instance index, whatever order the workgroups
 * are dispatched in -- and with it q = -P xref, the scaling and the KKT diagonal; everything
 * else comes from ctx's mpcq_params, or from the robots table where one is set (the two
 * tables are independent).  count == 0 or weights == NULL clears the table (the context's
 * mpcq_params again: a context that never sets one launches exactly what it did before).
 * While a table is set, a launch with batch > count returns MPCQ_E_INVALID and launches
 * nothing.
 * A host table is validated: every state weight and the force weight finite and > 0, reserved
 * zero; otherwise MPCQ_E_INVALID (the message names the first offending index and field) and
 * the table in force stays, as it does when the memory for a larger table cannot be
 * allocated (MPCQ_E_NOMEM).  A device table is not validated: a NaN or Inf among the values
 * of a row is caught by the solver's non-finite data check and ends as MPCQ_STATUS_NONFINITE
 * on that instance alone.
 * mpcq_formulate_batch does not look at the table: Ax, l, u hold no entry of P.
 * mpcq_qp_solve_batch does not look at it either, as with the robots table: its P comes
 * from the context's mpcq_params. */
int mpcq_set_weights(mpcq_ctx* ctx, int64_t count, const mpcq_weights* weights, uint32_t flags);

/* ---- per-instance disturbance -------------------------------------------------
 * No reference counterpart (the reference's model knows gravity only): a constant acceleration
 * that the model of instance b carries through every stage of its horizon, beside gravity --
 * an unmodelled payload's sag, a steady push, a bias the caller has estimated.  The frame is
 * the instance's xref frame (in a session: the tick's local frame).  With it
 *   X_{k+1}[6+i] = (the model as it was) + dt * a[i],   i = 0..5, every stage k,
 * in MPC.py's terms g[6+i] += dt * a[i]: the constant of dynamics row 6+i becomes
 * v + (-(dt * a[i])) (v: gravity * dt on row 8, -0.0 elsewhere), added before the xref terms,
 * so a row of +0.0 changes no bit of l, u, x or f0.  Ax and P do not move. */
typedef struct mpcq_disturbance {   /* 8 doubles = 64 bytes */
  double a[6];        /* linear acceleration [m/s^2], then angular acceleration [rad/s^2] */
  double reserved[2];            /* zero */
} mpcq_disturbance;
#ifdef __cplusplus
static_assert(sizeof(mpcq_disturbance) == 64, "mpcq_disturbance is 8 doubles");
#else
_Static_assert(sizeof(mpcq_disturbance) == 64, "mpcq_disturbance is 8 doubles");
#endif
/* Copies table [count] into memory the context owns, with mpcq_set_robots' and
 * mpcq_set_weights' rules word for word: from a host pointer the call blocks; with
 * MPCQ_FLAG_DEVICE_PTRS the copy is device to device on ctx's stream.  In every later
 * mpcq_formulate_batch and mpcq_solve_batch of ctx (both formulation modes, polish, sliced and
 * class-ordered solves included; a sliced solve's resumed launch re-formulates from the same
 * row) instance b takes its disturbance from table[b] -- b is the instance index, whatever
 * order the workgroups are dispatched in.  The three tables are independent.  count == 0 or
 * table == NULL clears the table (no disturbance: a context that never sets one launches
 * exactly what it did before).  While a table is set, a launch with batch > count returns
 * MPCQ_E_INVALID and launches nothing.
 * A host table is validated: every a[i] finite, reserved zero; otherwise MPCQ_E_INVALID (the
 * message names the first offending index and field) and the table in force stays, as it does
 * when the memory for a larger table cannot be allocated (MPCQ_E_NOMEM).  A device table is
 * not validated: a NaN or Inf among the six values of a row ends as MPCQ_STATUS_NONFINITE on
 * that instance alone (in mpcq_formulate_batch it reaches l and u as it is).
 * mpcq_qp_solve_batch does not look at the table: its caller's l and u hold what they hold. */
int mpcq_set_disturbance(mpcq_ctx* ctx, int64_t count, const mpcq_disturbance* table, uint32_t flags);

/* ---- formulation -----------------------------------------------------------
 * Replaces MPC.construct_gait + update_matrices (MPC.py:635-652, 290-378) in
 * MODE_UPDATE, and construct_gait + create_matrices (MPC.py:84-234) in
 * MODE_SETUP: writes A.data (CSC order), l and u for each instance.
 * status[b] = 0 or MPCQ_STATUS_BAD_GAIT. */
int mpcq_formulate_batch(mpcq_ctx* ctx, int64_t batch, const double* xref,
                         const double* fsteps, int mode, double* Ax, double* l,
                         double* u, int32_t* status, uint32_t flags);

/* ---- QP solve --------------------------------------------------------------
 * Replaces osqp.OSQP.update(Ax=, l=, u=) + warm_start(x=) + solve()
 * (MPC.py:419-428; osqp 0.6 ADMM).  P, q come from params (constant).
 * warm_x [B][n], warm_y [B][m], rho_in [B] are optional (NULL = cold start,
 * rho = params.rho).  x, y, rho_out, iters optional outputs (NULL = skip).
 * info [B][4] (optional): rho updates (refactorisations after the first),
 * polish result (0 not run, 1 accepted, -1 rejected), polish rounds run, and
 * the ADMM's own exit status before polish (with polish = 2 a MAX_ITER /
 * SOLVED_INACCURATE exit that polish upgrades reports SOLVED in status and the
 * ADMM's code here). */
int mpcq_qp_solve_batch(mpcq_ctx* ctx, int64_t batch, const double* Ax,
                        const double* l, const double* u, const double* warm_x,
                        const double* warm_y, const double* rho_in, double* x,
                        double* y, int32_t* status, int32_t* iters,
                        double* rho_out, int32_t* info, uint32_t flags);

/* ---- fused hot path --------------------------------------------------------
 * Replaces MPC.run(k, xref, fsteps) (MPC.py:460-514) for a batch: formulation
 * + OSQP solve (with the osqp workspace carried between ticks: warm_x, warm_y,
 * rho_in, as mpcq_qp_solve_batch) + retrieve_result (MPC.py:432-458) in one
 * launch.  f0 [B][12] = f_applied; x [B][n], y [B][m], rho_out [B] optional. */
int mpcq_solve_batch(mpcq_ctx* ctx, int64_t batch, const double* xref,
                     const double* fsteps, int mode, const double* warm_x,
                     const double* warm_y, const double* rho_in, double* f0, double* x,
                     double* y, double* rho_out, int32_t* status, int32_t* iters,
                     int32_t* info, uint32_t flags);

/* ---- footstep planner ------------------------------------------------------
 * The producer of (xref, fsteps): FootstepPlanner.py.  Per instance the
 * planner keeps the reference object's mutable state — the gait table
 * gait [20][5] (durations + contact bits, FootstepPlanner.py:58-62,193-213),
 * the rotation-command state machine (flag_rotation_command,
 * h_rotation_command, FootstepPlanner.py:67-68,130-154) and xref itself
 * (getRefStates only rewrites some rows in some states, so xref is in/out).
 *
 * Parameters (mpcq_default_planner_params): FootstepPlanner.py:18-52,321,352. */
typedef struct mpcq_planner_params {
  double dt;            /* MPC time step, 0.02 */
  double T_gait;        /* 0.32 (FootstepPlanner.py:51); getRefStates' linspace end points */
  double h_ref;         /* 0.2027682 (processing.py:131 passes it to getRefStates) */
  double k_feedback;    /* 0.03 */
  double L;             /* 0.12: bound on the (x, y) deviation from the shoulders */
  double g;             /* 9.81 */
  double t_stance;      /* 0.16 (compute_next_footstep) */
  double cmd_threshold; /* 0.05: joystick dead band of the height command */
  double shoulders[8];  /* row-major 2x4: x of FL FR HL HR, then y */
  double reduced_offset[8]; /* row-major 2x4 subtracted when reduced (FootstepPlanner.py:320-322) */
  int32_t reserved[8];
} mpcq_planner_params;

/* operations of mpcq_plan_batch, applied in this order */
#define MPCQ_PLAN_ROLL 1u       /* FootstepPlanner.roll (FootstepPlanner.py:401-425) */
#define MPCQ_PLAN_FOOTSTEPS 2u  /* compute_footsteps (FootstepPlanner.py:284-361) */
#define MPCQ_PLAN_REFSTATES 4u  /* getRefStates (FootstepPlanner.py:76-159) */
/* update_fsteps(k > 0) + getRefStates: the once-per-tick sequence of processing.py:81-131 */
#define MPCQ_PLAN_TICK (MPCQ_PLAN_ROLL | MPCQ_PLAN_FOOTSTEPS | MPCQ_PLAN_REFSTATES)

void mpcq_default_planner_params(mpcq_planner_params* pp);

/*
 * Replaces FootstepPlanner.update_fsteps(k, l_feet, v_cur, v_ref, h, oMl, _, reduced)
 * (FootstepPlanner.py:427-459, minus its viewer code) and getRefStates(k, T_gait,
 * lC, abg, lV, lW, v_ref, h_ref) (FootstepPlanner.py:76-159) for a batch.
 *   ops       MPCQ_PLAN_* bits
 *   k         getRefStates' k (only k == 0 is distinguished, FootstepPlanner.py:105)
 *   state     [B][12] lC, abg, lV, lW (local frame)             REFSTATES
 *   v_cur     [B][6]  compute_footsteps' v_cur; NULL = state[6:12] (processing.py:81)
 *   h         [B]     compute_footsteps' h;    NULL = state[2]   (processing.py:82)
 *   l_feet    [B][3][4] feet positions, local frame                FOOTSTEPS
 *   v_ref     [B][6]
 *   reduced   [B] int32, NULL = 0
 *   gait      [B][20][5]  in/out
 *   rot_flag  [B] int32 in/out, h_rot [B] in/out   (REFSTATES; 0 / 0.2 initially)
 *   xref      [B][12][N+1] in/out                                  REFSTATES
 *   fsteps    [B][20][13] out                                      FOOTSTEPS
 *   status    [B] out (optional): 0, or MPCQ_STATUS_BAD_GAIT where the reference
 *             raises (gait table without a zero-duration terminator / empty); the
 *             instance's buffers are then left unchanged.  Otherwise the table
 *             is followed exactly as the reference indexes it (an empty first row
 *             makes roll() look at row -1 = row 19, as Python does). */
int mpcq_plan_batch(mpcq_ctx* ctx, const mpcq_planner_params* pp, int64_t batch, uint32_t ops,
                    int k, const double* state, const double* v_cur, const double* h,
                    const double* l_feet, const double* v_ref, const int32_t* reduced,
                    double* gait, int32_t* rot_flag, double* h_rot, double* xref, double* fsteps,
                    int32_t* status, uint32_t flags);

/* ---- closed-loop session ---------------------------------------------------
 * B robots, each running the reference's once-per-tick MPC sequence
 * (processing.py:81-131 + MPC.run, MPC.py:460-514) with every piece of state
 * the reference keeps between ticks resident in HBM:
 *   FootstepPlanner: gait table, rotation state machine, xref, fsteps;
 *   MPC / osqp workspace: x (the next tick's warm start is x shifted by one
 *   stage, MPC.py:403-406), y and rho (kept by osqp across solves), q_w.
 * A tick is three launches on the context's stream, no host round trip:
 *   planner (roll + compute_footsteps + getRefStates; at k == 0 the extra
 *   compute_footsteps of processing.py:80-82 first) -> fused formulation + OSQP
 *   solve (k == 0: create_matrices, cold start; k > 0: update_matrices, warm) ->
 *   retrieve (f_applied, x_robot, q_next / v_next, q_w, the Logger's cost
 *   components, the next warm start, the virtual robot's next state).
 *
 * Virtual robot (optional): passing state == NULL / l_feet == NULL to a tick
 * takes the robot's state from the previous tick's prediction x_robot[:, 0],
 * re-expressed in the new local frame (origin under the base, yaw removed,
 * Interface.py:100-138), and the stance feet from the previous fsteps — the
 * "MPC future state as the robot state" path of processing.py:33-38.  It makes
 * a closed loop run entirely on the device (tests, benchmarks). */
typedef struct mpcq_session mpcq_session;

/* gait0 [B][20][5] (NULL: create_walking_trot for this ctx's horizon, FootstepPlanner.py:193-214).
 * pp NULL = mpcq_default_planner_params.  The session keeps ctx (and its stream). */
int mpcq_session_create(mpcq_ctx* ctx, int64_t batch, const mpcq_planner_params* pp,
                        const double* gait0, mpcq_session** out);
int mpcq_session_destroy(mpcq_session* s);

/* One tick for every robot.  state [B][12] (lC, abg, lV, lW), l_feet [B][3][4],
 * v_ref [B][6], reduced [B] (NULL = 0); host pointers, or device pointers with
 * MPCQ_FLAG_DEVICE_PTRS.  state / l_feet NULL = the virtual robot (above).
 * k = MPC tick index (k == 0: first tick, MPC.py:491).  Blocking unless
 * MPCQ_FLAG_ASYNC together with MPCQ_FLAG_DEVICE_PTRS.
 * From the second tick on, the solve dispatches the robots longest-first by the
 * previous tick's iteration counts (a fourth, one-workgroup launch after the
 * retrieve builds the order); results do not depend on it.  The environment
 * variable MPCQ_DISPATCH_ORDER=0, read at mpcq_session_create, keeps index order
 * (timing comparisons only). */
int mpcq_session_tick(mpcq_session* s, int k, const double* state, const double* l_feet,
                      const double* v_ref, const int32_t* reduced, uint32_t flags);

/* Per-robot arrays a session holds (mpcq_session_read / mpcq_session_device_ptr). */
#define MPCQ_SV_F0 0        /* [B][12]     f_applied (MPC.py:441-444) */
#define MPCQ_SV_X 1         /* [B][24N]    QP solution x */
#define MPCQ_SV_X_ROBOT 2   /* [B][12][N]  x_robot = x states + xref[:, 1:] (MPC.py:437-449) */
#define MPCQ_SV_Q_W 3       /* [B][6]      world pose (MPC.py:503-510) */
#define MPCQ_SV_COST 4      /* [B][13]     Logger.log_cost_function (Logger.py:406-418) */
#define MPCQ_SV_XREF 5      /* [B][12][N+1] */
#define MPCQ_SV_FSTEPS 6    /* [B][20][13] */
#define MPCQ_SV_GAIT 7      /* [B][20][5] */
#define MPCQ_SV_STATUS 8    /* [B] int32: OSQP status, or MPCQ_STATUS_BAD_GAIT from the planner */
#define MPCQ_SV_ITERS 9     /* [B] int32 */
#define MPCQ_SV_RHO 10      /* [B] */
#define MPCQ_SV_Y 11        /* [B][44N] */
#define MPCQ_SV_STATE 12    /* [B][12]     the virtual robot's next state */
#define MPCQ_SV_L_FEET 13   /* [B][3][4]   the virtual robot's next feet */
#define MPCQ_SV_ROT_FLAG 14 /* [B] int32 */
#define MPCQ_SV_H_ROT 15    /* [B] */
#define MPCQ_SV_ORDER 16    /* [B] int32: the next tick's dispatch order (read-only: a permutation of
                               0..B-1, longest previous solve first, buckets of 16 iterations; the
                               identity until the first tick) */
/* Only on a session with mpcq_session_enable_swing (otherwise MPCQ_E_INVALID): */
#define MPCQ_SV_SWING_REF 17   /* [B][k_mpc][4][9] the tick's swing-foot references (read-only) */
#define MPCQ_SV_SWING_STATE 18 /* [B][4][MPCQ_SWING_STATE] the foot trajectory generators */
#define MPCQ_SV_FRAME 19    /* [B][3] x, y, yaw of MPCQ_SV_Q_W as they stood before this tick's
                               update: the frame of the tick's fsteps (read-only) */
#define MPCQ_SV_FIRST 20    /* [B] int32: 1 = a reset is pending, the robot's next tick runs as a first
                               tick whatever k says (read-only: mpcq_session_reset sets it, the tick's
                               retrieve clears it; 0 after create) */
#define MPCQ_SV_COUNT 21
/* Copy array `what` to dst (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking. */
int mpcq_session_read(mpcq_session* s, int what, void* dst, uint32_t flags);
/* Overwrite array `what` from src (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking.
 * MPCQ_SV_ORDER and MPCQ_SV_FIRST are read-only (MPCQ_E_INVALID). */
int mpcq_session_write(mpcq_session* s, int what, const void* src, uint32_t flags);
/* Device address of array `what` (valid until mpcq_session_destroy).  The engine reads
 * MPCQ_SV_ORDER as its workgroup -> robot map: writing through its device address is not
 * allowed (a non-permutation would solve some robots twice and others not at all). */
int mpcq_session_device_ptr(mpcq_session* s, int what, void** out);
/* The session's own table of per-robot constants, robots [B] (mpcq_set_robots: the same
 * copy, validation and flags); independent of the context's table, so a batch solve on the
 * same context does not disturb the session, nor the session a batch solve.  May be called
 * between any two ticks: the ticks after it use the new table.  NULL clears it.  A session
 * that never sets one launches exactly what it did before. */
int mpcq_session_set_robots(mpcq_session* s, const mpcq_robot* robots, uint32_t flags);
/* The table in force, robots [B] (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking.
 * Without a table: mpcq_default_robot(the context's params) for every robot. */
int mpcq_session_get_robots(mpcq_session* s, mpcq_robot* robots, uint32_t flags);
/* The session's own table of cost weights, weights [B] (mpcq_set_weights: the same copy,
 * validation and flags); independent of the context's table.  The ticks after the call solve
 * robot b under weights[b], and MPCQ_SV_COST is robot b's cost under weights[b].  NULL clears
 * it.  The table persists across mpcq_session_reset and the monitor's auto-reset.  It is the
 * controller's tuning, not the robot's state: snapshots do not carry it, and restore,
 * restore_map and fork leave the table in force untouched -- fork(r) followed by
 * mpcq_session_set_weights is a tuning sweep from one state. */
int mpcq_session_set_weights(mpcq_session* s, const mpcq_weights* weights, uint32_t flags);
/* The table in force, weights [B] (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking.
 * Without a table: mpcq_default_weights(the context's params) for every robot. */
int mpcq_session_get_weights(mpcq_session* s, mpcq_weights* weights, uint32_t flags);
/* The session's own table of disturbances, table [B] (mpcq_set_disturbance: the same copy,
 * validation and flags); independent of the context's table.  The ticks after the call solve
 * robot b with table[b] in its model, in the tick's local frame.  NULL clears it.  The table
 * persists across mpcq_session_reset and the monitor's auto-reset.  Like the weights it is the
 * controller's, not the robot's state: snapshots do not carry it (the blob of a session with a
 * table is byte for byte the blob without one), and restore, restore_map and fork leave the
 * table in force untouched. */
int mpcq_session_set_disturbance(mpcq_session* s, const mpcq_disturbance* table, uint32_t flags);
/* The table in force, table [B] (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking.
 * Without a table: zeros for every robot. */
int mpcq_session_get_disturbance(mpcq_session* s, mpcq_disturbance* table, uint32_t flags);
/* Restart a subset of the robots between two ticks; the others are not written at all.
 *   mask  [B] int32, nonzero = reset this robot; NULL = every robot
 *   gait0 [B][20][5] or NULL (the table the session was created with, of which it keeps a
 *         device copy); q_w0 [B][6] or NULL ((0, 0, 0.2027682, 0, 0, 0), MPC.py:53-56).
 *         Only the rows of masked robots are read.
 * Host pointers (blocking, as mpcq_session_tick), or device pointers with
 * MPCQ_FLAG_DEVICE_PTRS; with MPCQ_FLAG_DEVICE_PTRS | MPCQ_FLAG_ASYNC the call enqueues on
 * the context's stream and returns: a mask computed on the device never visits the host.
 * Every per-robot array of a masked robot goes back to what mpcq_session_create leaves
 * (GAIT: the gait0 row or the creation table; ROT_FLAG 0, H_ROT 0.20, XREF 0, FSTEPS NaN,
 * Q_W: q_w0 or the default; STATE / L_FEET: the virtual robot standing at h_ref, feet under
 * the shoulders; RHO params.rho; Y, the warm start, X, F0, X_ROBOT, COST, STATUS, ITERS 0;
 * with swing enabled SWING_STATE, SWING_REF, FRAME 0), and its MPCQ_SV_FIRST is set: its next
 * tick is a first tick whatever k the call passes (the extra compute_footsteps, h_ref in
 * getRefStates, create_matrices, a cold solve at params.rho that reads no warm x or y), while
 * every other robot runs as k says (k == 0 still makes every robot first).  The tick's
 * retrieve clears the flag.  Robots with a pending reset go to the front of MPCQ_SV_ORDER (a
 * cold solve is a robot's longest).  The session's robots table is kept.  Nothing but s is
 * validated: a malformed gait0 row shows as MPCQ_STATUS_BAD_GAIT on the robot's next tick,
 * as at create.  A session on which this was never called launches exactly what it did
 * before. */
int mpcq_session_reset(mpcq_session* s, const int32_t* mask, const double* gait0,
                       const double* q_w0, uint32_t flags);

/* ---- swing-foot trajectories ----------------------------------------------
 * The consumer of (gait, fsteps) between two MPC ticks: the position, velocity and
 * acceleration references of the swing feet that the reference's whole-body controller
 * derives every dt (update_feet_tasks / update_footsteps,
 * TSID_Debug_controller_four_legs_fb_vel.py:247-327, 471-487) with
 * Foot_trajectory_generator.get_next_foot (FootTrajectoryGenerator.py:184-380): a 5th-order
 * polynomial in x and y, a 6th-order one in z, re-targeted every step until t_lock before
 * touchdown.  pinocchio and the TSID solver stay out of scope. */
typedef struct mpcq_swing_params {
  double dt;          /* 0.001  TSID:107 */
  double max_height;  /* 0.05   TSID:96  */
  double t_lock;      /* 0.05   TSID:97  */
  double feet_z;      /* 0.0    Interface.py:91 */
  int32_t k_mpc;      /* 20     main.py:21 */
  int32_t reserved[7];
} mpcq_swing_params;
void mpcq_default_swing_params(mpcq_swing_params* sp);
/* doubles per foot; a generator's state is [B][4][MPCQ_SWING_STATE], all-zero = a new generator:
 *   0..23  lastCoeffs in the reference's order (cx5..cx0, dx5..dx0, cy5..cy0, dy5..dy0,
 *          FootTrajectoryGenerator.py:308-309)
 *   24,25  x1, y1         26..31  mgoals (x, dx, ddx, y, dy, ddy)
 *   32     t_swing         33      the last t0
 *   34     the last mode (1 adaptive, 0 locked)
 *   35,36  the foot's last world x, y            37..39  zero */
#define MPCQ_SWING_STATE 40

/* One get_next_foot(x0, dx0, ddx0, y0, dy0, ddy0, x1, y1, t0, t1, dt) per (robot, foot).
 *   in    [B][4][10]  the ten arguments above (dt from sp)
 *   state [B][4][MPCQ_SWING_STATE] in/out (slots 0..25 and 34 are used)
 *   out   [B][4][11]  the reference's return list: x0, dx0, ddx0, y0, dy0, ddy0, z0, dz0,
 *                     ddz0, gx1, gy1
 * A foot whose t0 is NaN is skipped: its outputs are NaN and its state is untouched. */
int mpcq_swing_step_batch(mpcq_ctx* ctx, const mpcq_swing_params* sp, int64_t batch,
                          const double* in, double* state, double* out, uint32_t flags);

/* Substeps k_sub0 .. k_sub0 + n_sub - 1 (k_loop % k_mpc in the reference) of
 * update_footsteps + update_feet_tasks for a batch.
 *   gait    [B][20][5], fsteps [B][20][13]   the tick's tables
 *   frame   [B][3]  x, y, yaw of the local frame in the world (the reference's oMl), held
 *                   for the whole call.  The reference moves oMl every substep: a call with
 *                   n_sub = 1 reproduces that exactly; a call over a whole tick holds the
 *                   frame, which is exact for the session's virtual robot.
 *   feet0   [B][4][6] or NULL: the measured foot (x, dx, ddx, y, dy, ddy, world frame) a
 *                   swing starts from at lift-off (t0 == 0, TSID:290-295).  NULL: the
 *                   foot's last world position kept in the state, at rest (the virtual
 *                   robot's rule; no reference counterpart).
 *   state   [B][4][MPCQ_SWING_STATE] in/out
 *   ref     [B][n_sub][4][9] out: pos xyz, vel xyz, acc xyz (feet_z added to z); NaN for a
 *                   stance foot (no tracking task, TSID:524-549)
 *   t0_out  [B][n_sub][4] out, optional; NaN for stance feet
 *   status  [B] out, optional: 0, or MPCQ_STATUS_BAD_GAIT for a robot with a swing foot that
 *                   has no stance row in its gait column (the reference raises IndexError);
 *                   its state is left unchanged and its outputs are NaN.
 * k_sub0 < 0, n_sub < 1, k_sub0 + n_sub > k_mpc or a NULL required pointer: MPCQ_E_INVALID. */
int mpcq_swing_batch(mpcq_ctx* ctx, const mpcq_swing_params* sp, int64_t batch, int k_sub0,
                     int n_sub, const double* gait, const double* fsteps, const double* frame,
                     const double* feet0, double* state, double* ref, double* t0_out,
                     int32_t* status, uint32_t flags);

/* Opt-in (sp NULL = mpcq_default_swing_params): every later mpcq_session_tick appends one
 * swing launch after its last launch, over substeps 0..k_mpc-1 of the tick's resident gait /
 * fsteps with feet0 = NULL and the frame MPCQ_SV_FRAME.  A session that never calls it
 * launches exactly what it did before. */
int mpcq_session_enable_swing(mpcq_session* s, const mpcq_swing_params* sp);

/* ---- rigid-body plant ------------------------------------------------------
 * No reference counterpart (the reference closes its loop with PyBullet and TSID): the object
 * the MPC is a discretisation of, a single rigid body under the forces of its stance feet,
 * integrated on the device over one MPC tick, with constants of its own and an external
 * wrench -- so that the robot a session moves can disagree with the controller's model
 * (an unknown payload, another friction, a push).  FP64, one thread per robot.
 *
 * Everything of one robot is expressed in one inertial frame (in a session: the tick's local
 * frame).  Effective forces, once per tick: a swing foot (any NaN coordinate) applies none;
 * with clamp != 0 a stance foot's fz is limited to [0, fz_max] and its tangential part, if
 * t = sqrt(fx^2 + fy^2) > mu fz, scaled by mu fz / t onto the Coulomb cone (the model's
 * friction pyramid admits sqrt(2) mu, so the clamp bites even with the model's own mu).
 * F = sum f_i + wrench[0:3], tau = sum (p_i - c0) x f_i + wrench[3:6]: the lever arms are
 * taken at the tick's start and held, as the MPC holds them.
 *   MPCQ_PLANT_MODEL  the MPC's own discrete step (MPC.py:110-119, 171-178, 201) with the
 *                     plant's constants: c += dt v0, rpy += dt w0, v += dt F / m - dt g e_z,
 *                     w += dt inv(Rz(yaw0) gI) tau (the reference's Rz gI, not Rz gI Rz');
 *                     n_sub is ignored
 *   MPCQ_PLANT_RIGID  n_sub semi-implicit Euler substeps of h = dt / n_sub: R = Rz(yaw)
 *                     Ry(pitch) Rx(roll), Iw = R gI R', a = F / m - g e_z, alpha = inv(Iw)
 *                     (tau - w x Iw w), v += h a, w += h alpha, c += h v, rpy += h E w (new v
 *                     and w, the substep's old angles; E maps the world-frame angular
 *                     velocity to ZYX angle rates)
 * 3x3 inverses by the adjugate; sums left to right in foot order; no contraction, so a host
 * restatement in the same order (tests/plant_model.py) differs by the sin / cos only.  A NaN
 * among a robot's inputs spreads through that robot's arithmetic and to no other robot. */
#define MPCQ_PLANT_MODEL 0
#define MPCQ_PLANT_RIGID 1
typedef struct mpcq_plant_params {   /* 48 bytes */
  double dt;          /* 0.02: one MPC tick */
  double gravity;     /* 9.81 */
  int32_t n_sub;      /* 20 (k_mpc, main.py:21); >= 1 */
  int32_t integrator; /* MPCQ_PLANT_RIGID */
  int32_t clamp;      /* 1 */
  int32_t reserved[5];
} mpcq_plant_params;
#ifdef __cplusplus
static_assert(sizeof(mpcq_plant_params) == 48, "mpcq_plant_params is 48 bytes");
#else
_Static_assert(sizeof(mpcq_plant_params) == 48, "mpcq_plant_params is 48 bytes");
#endif
void mpcq_default_plant_params(mpcq_plant_params* pl);
/* One tick of the plant for a batch.
 *   state     [B][12] c, rpy, v, w
 *   feet      [B][3][4] foot positions, laid out as l_feet; NaN = swing
 *   f         [B][12] foot-major fx, fy, fz per foot, as f_applied
 *   wrench    [B][6] force, then torque about the centre of mass; NULL = none
 *   robots    [B] mass, gI, mu, fz_max per robot; NULL = ctx's mpcq_params (a host table is
 *             validated as in mpcq_set_robots, a device table is not)
 *   state_out [B][12]; may be state itself
 *   f_eff     [B][12] the effective forces; NULL = not wanted
 * pl NULL = mpcq_default_plant_params.  Host pointers, or device pointers with
 * MPCQ_FLAG_DEVICE_PTRS (then MPCQ_FLAG_ASYNC does not wait for the stream).  dt <= 0, n_sub < 1,
 * an unknown integrator or a NULL required pointer: MPCQ_E_INVALID, nothing is launched. */
int mpcq_plant_step_batch(mpcq_ctx* ctx, const mpcq_plant_params* pl, int64_t batch,
                          const double* state, const double* feet, const double* f,
                          const double* wrench, const mpcq_robot* robots, double* state_out,
                          double* f_eff, uint32_t flags);

/* Opt-in (pl NULL = mpcq_default_plant_params with ctx's dt; a dt other than ctx's is
 * MPCQ_E_INVALID): while enabled, every mpcq_session_tick runs one plant launch directly after
 * its retrieve, on the context's stream, no host synchronisation.  Per robot it integrates the
 * state the tick's planner read, under MPCQ_SV_F0 at the stance feet of row 0 of the tick's
 * fsteps, the session's wrench, and the plant's table of robots (without one the session's
 * model table, without that ctx's params), and rewrites MPCQ_SV_Q_W, MPCQ_SV_STATE and
 * MPCQ_SV_L_FEET by the retrieve's own formulas with the plant's end state in place of the
 * prediction x_robot[:, 0], from MPCQ_SV_Q_W as it stood before the tick.  MPCQ_SV_X_ROBOT,
 * the warm start and every other array stay the MPC's: x_robot[:, 0] - MPCQ_PV_STATE_END is
 * the tracking error.  A robot the retrieve treats as failed (status not SOLVED,
 * SOLVED_INACCURATE or MAX_ITER_REACHED) keeps what the retrieve left; its MPCQ_PV_STATE_END
 * and MPCQ_PV_F_EFF rows are NaN.  The swing launch and the dispatch order are unaffected.
 * Calling it again replaces the parameters.  A session that never enables it launches exactly
 * what it did before. */
int mpcq_session_enable_plant(mpcq_session* s, const mpcq_plant_params* pl);
/* The ticks after it run without the plant launch; the wrench and the plant's table stay. */
int mpcq_session_disable_plant(mpcq_session* s);
/* The true robots, robots [B] (mpcq_session_set_robots: the same copy, validation and flags),
 * distinct from the model's table; NULL clears it.  Kept across mpcq_session_reset. */
int mpcq_session_set_plant_robots(mpcq_session* s, const mpcq_robot* robots, uint32_t flags);
/* The external wrench, wrench [B][6]: force, then torque about the centre of mass, in the
 * WORLD frame; each tick rotates force and torque separately by Rz(-yaw) into its local frame,
 * yaw = MPCQ_SV_Q_W[5] as it stood before the tick.  NULL = zero.  Host pointer (the call
 * blocks), or device pointer with MPCQ_FLAG_DEVICE_PTRS (copied on the context's stream;
 * MPCQ_FLAG_ASYNC does not wait).  It persists until changed, across mpcq_session_reset too,
 * and may be set before the plant is enabled. */
int mpcq_session_set_wrench(mpcq_session* s, const double* wrench, uint32_t flags);
/* The plant's arrays; they exist from the first mpcq_session_enable_plant or
 * mpcq_session_set_wrench on (before: MPCQ_E_INVALID), zero until written. */
#define MPCQ_PV_STATE_END 0  /* [B][12] plant state at the tick's end, in the tick's frame */
#define MPCQ_PV_F_EFF 1      /* [B][12] the effective forces of the tick */
#define MPCQ_PV_WRENCH 2     /* [B][6]  the wrench as set (world frame) */
#define MPCQ_PV_COUNT 3
/* Copy array `what` to dst (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking. */
int mpcq_session_plant_read(mpcq_session* s, int what, void* dst, uint32_t flags);
/* Device address of array `what` (valid until mpcq_session_destroy). */
int mpcq_session_plant_device_ptr(mpcq_session* s, int what, void** out);

/* ---- episode monitor -------------------------------------------------------
 * No reference counterpart (the reference runs one robot until its script ends): what turns a
 * session into a batch of episodes.  After a tick, one thread per robot decides whether the
 * robot's episode ended, keeps the episode's statistics, and leaves the done bits as an int32
 * mask on the device -- the mask mpcq_session_reset takes.  FP64, no contraction, every sum
 * left to right in index order: tests/monitor_model.py restates it in numpy, bit for bit.
 *
 * Done bits of a tick (0 = the episode goes on): */
#define MPCQ_DONE_NONFINITE 1 /* some q_w[0..5] is NaN or infinite */
#define MPCQ_DONE_TILT 2      /* fabs(q_w[3]) > max_tilt or fabs(q_w[4]) > max_tilt */
#define MPCQ_DONE_HEIGHT 4    /* q_w[2] < min_height */
#define MPCQ_DONE_SOLVER 8    /* status none of SOLVED, SOLVED_INACCURATE, MAX_ITER_REACHED: the
                                 retrieve's own test, so MPCQ_STATUS_BAD_GAIT sets it */
#define MPCQ_DONE_TIMEOUT 16  /* max_ticks > 0 and the episode has run max_ticks ticks, this one
                                 included */
/* TILT and HEIGHT are comparisons, false on NaN: a NaN pose sets NONFINITE only.  A value equal
 * to its threshold is not a violation.
 *
 * Episode accumulators ep [B][8], updated every tick:
 *   0  sum of the tick's cost: the 13 entries of MPCQ_SV_COST summed left to right, then added
 *   1  sum of f0 . f0 (the 12 squares summed left to right)
 *   2  sum of iters
 *   3  max over the ticks of max(fabs(roll), fabs(pitch))
 *   4  min over the ticks of z (+inf before the first tick)
 *   5  sum of (state[6] - v_ref[0])^2 + (state[7] - v_ref[1])^2 + (state[11] - v_ref[5])^2.
 *      Frame caveat: state is the virtual robot's NEXT state, its velocity expressed in the next
 *      tick's local frame, while v_ref is this tick's command in this tick's frame; the two
 *      differ by the yaw the robot turned during the tick (a rotation of the x, y components).
 *   6, 7  zero
 * A tick with the SOLVER bit adds nothing to 0, 1 and 5 (a failed solve's f0 and cost are not
 * the controller's); a tick with the NONFINITE bit leaves 3 and 4 alone.  ep_ticks [B] int32
 * counts the episode's ticks.
 * On a tick with done != 0: last [B][16] = ep[0..7] with this tick in, the tick count, the done
 * bits, q_w[0..5]; episodes [B] int32 is incremented; ep and ep_ticks restart (ep[3] = 0,
 * ep[4] = +inf).
 * totals [8] uint64, cumulative, never cleared by a tick: 0 robot-ticks monitored, 1 episodes
 * ended, 2..6 how often each done bit was set (NONFINITE .. TIMEOUT), 7 zero.
 * trace [B][MPCQ_TRACE] (optional), all doubles: 0..5 q_w, 6 done bits, 7 status, 8 iters,
 * 9 the episode's ticks with this one in and before any restart, 10 the tick's cost sum,
 * 11 f0 . f0, 12..15 zero. */
#define MPCQ_TRACE 16
typedef struct mpcq_monitor_params {  /* 64 bytes */
  double max_tilt;     /* 0.5 rad; > 0, +inf switches the test off */
  double min_height;   /* 0.10 (half of h_ref); finite, or -inf to switch the test off */
  int32_t max_ticks;   /* 0 = no limit; >= 0 */
  int32_t auto_reset;  /* 0; 1: a session's tick restarts the robots whose episode ended */
  int32_t reserved[10];
} mpcq_monitor_params;
#ifdef __cplusplus
static_assert(sizeof(mpcq_monitor_params) == 64, "mpcq_monitor_params is 64 bytes");
#else
_Static_assert(sizeof(mpcq_monitor_params) == 64, "mpcq_monitor_params is 64 bytes");
#endif
void mpcq_default_monitor_params(mpcq_monitor_params* mp);
/* The monitor on its own, one tick for a batch.
 *   q_w [B][6], status [B], iters [B], f0 [B][12], cost [B][13], state [B][12], v_ref [B][6]: in
 *   ep [B][8], ep_ticks [B], done [B]: in/out (done: out)
 *   episodes [B], last [B][16], totals [8], trace [B][MPCQ_TRACE]: in/out, each optional (NULL)
 * mp NULL = mpcq_default_monitor_params (auto_reset is ignored here).  Host pointers, or device
 * pointers with MPCQ_FLAG_DEVICE_PTRS (then MPCQ_FLAG_ASYNC does not wait for the stream).  A
 * NaN or out-of-range field of mp or a NULL required pointer: MPCQ_E_INVALID, nothing is
 * launched. */
int mpcq_monitor_step_batch(mpcq_ctx* ctx, const mpcq_monitor_params* mp, int64_t batch,
                            const double* q_w, const int32_t* status, const int32_t* iters,
                            const double* f0, const double* cost, const double* state,
                            const double* v_ref, double* ep, int32_t* ep_ticks, int32_t* episodes,
                            double* last, int32_t* done, uint64_t* totals, double* trace,
                            uint32_t flags);

/* Opt-in (mp NULL = mpcq_default_monitor_params): while enabled, every mpcq_session_tick runs one
 * monitor launch directly after its plant launch (without a plant: after its retrieve), on the
 * context's stream, over MPCQ_SV_Q_W, _STATUS, _ITERS, _F0, _COST, _STATE as the tick leaves
 * them and the tick's v_ref.  The monitor's arrays are made by the first enable, zero then
 * (ep[4] = +inf); calling it again replaces the parameters and keeps the arrays.
 * With auto_reset = 1 the tick ends, after its last launch (the swing launch included, which
 * still sees the tick's gait and fsteps), by enqueueing exactly what mpcq_session_reset(s,
 * MPCQ_MV_DONE's device address, NULL, NULL, MPCQ_FLAG_DEVICE_PTRS | MPCQ_FLAG_ASYNC) enqueues:
 * the robots whose episode ended start their next tick as a first tick from the creation table
 * and the default pose; their terminal pose survives in MPCQ_MV_LAST and in the trace.
 * An explicit mpcq_session_reset of a robot discards its running episode (ep and ep_ticks
 * restart, no episode is counted, last is kept).  A session that never enables the monitor
 * launches exactly what it did before. */
int mpcq_session_enable_monitor(mpcq_session* s, const mpcq_monitor_params* mp);
/* The ticks after it run without the monitor launch and the auto-reset; the arrays stay. */
int mpcq_session_disable_monitor(mpcq_session* s);
/* The monitor's arrays; they exist from the first mpcq_session_enable_monitor on (before:
 * MPCQ_E_INVALID). */
#define MPCQ_MV_DONE 0      /* [B] int32   the last tick's done bits */
#define MPCQ_MV_EP 1        /* [B][8]      the running episode's accumulators */
#define MPCQ_MV_EP_TICKS 2  /* [B] int32   the running episode's ticks */
#define MPCQ_MV_EPISODES 3  /* [B] int32   episodes ended */
#define MPCQ_MV_LAST 4      /* [B][16]     the last ended episode */
#define MPCQ_MV_TOTALS 5    /* [8] uint64  batch totals */
#define MPCQ_MV_COUNT 6
/* Copy array `what` to dst (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking. */
int mpcq_session_monitor_read(mpcq_session* s, int what, void* dst, uint32_t flags);
/* Device address of array `what` (valid until mpcq_session_destroy). */
int mpcq_session_monitor_device_ptr(mpcq_session* s, int what, void** out);

/* n_ticks ticks of the virtual robot (or the plant) enqueued in one call: tick t runs as
 * mpcq_session_tick(s, k0 + t, NULL, NULL, v_ref row min(t, v_ref_ticks - 1), NULL, ...) and
 * leaves every array as that sequence of calls does.
 *   v_ref [v_ref_ticks][B][6] device; trace [n_ticks][B][MPCQ_TRACE] device or NULL: tick t's
 *   monitor writes row t (a trace on a session whose monitor is not enabled: MPCQ_E_INVALID)
 * flags must include MPCQ_FLAG_DEVICE_PTRS; the call blocks unless MPCQ_FLAG_ASYNC.  k0 < 0,
 * n_ticks < 1, v_ref_ticks < 1, a NULL v_ref or host pointers: MPCQ_E_INVALID, nothing is
 * launched. */
int mpcq_session_run(mpcq_session* s, int k0, int n_ticks, const double* v_ref, int v_ref_ticks,
                     double* trace, uint32_t flags);

/* ---- scenarios -------------------------------------------------------------
 * The producer of v_ref, and of what disturbs a robot, on the device: per robot and per episode
 * a command profile relative to the episode's start (the reference's one command source in use,
 * Joystick.update_v_ref_predefined, Joystick.py:70-83, is its default), push windows, and the
 * true mass and friction of the plant's robot.  One thread per robot, stateless but for two
 * integers per robot (the episode's number `epoch` and the episode's tick `tau`); every draw
 * comes from a counter-based generator, so a host restatement (mpcq/scenario.py in the Python
 * package) reproduces any episode from (seed, robot, epoch), bit for bit.
 *
 * Generator: Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85, called as philox(counter = (b, epoch, index, stream), key = (seed & 0xffffffff,
 * seed >> 32)) -> w0..w3; streams: 0 the episode's constants, 1 commands, 2 pushes.
 *   u(wa, wb)        = ((wa >> 5) * 67108864.0 + (wb >> 6)) * 2^-53      a double in [0, 1)
 *   range(lo, hi, u) = lo + (hi - lo) * u                                no contraction
 *   int(a, n, w)     = a + (int)(((uint64)w * n) >> 32)                  in [a, a + n - 1]
 *   prob(w, p)       = (double)w * 2^-32 < p
 *
 * A robot-tick.  On a tick where the robot is first, epoch += 1 and tau = 0; otherwise tau is
 * the stored tick.  After the tick's computation the stored tick is tau + 1.
 *   Constants (a first tick only): philox(b, epoch, 0, 0): mass_scale = range(mass_scale_lo,
 *     mass_scale_hi, u(w0, w1)), mu = range(mu_lo, mu_hi, u(w2, w3)).  robots_out[b] = the base
 *     row, with (robots & 1) mass and the nine gI entries times mass_scale, with (robots & 2) mu
 *     replaced.  draw[b] = mass_scale, mu, (double)epoch, five zeros.
 *   Commands (commands != 0): segment j = cmd_period > 0 ? tau / cmd_period : 0; its target:
 *     philox(b, epoch, 2j, 1) -> vx = range(v_lo[0], v_hi[0], u(w0, w1)), vy = range(v_lo[1],
 *     v_hi[1], u(w2, w3)); philox(b, epoch, 2j + 1, 1) -> wyaw = range(v_lo[2], v_hi[2],
 *     u(w0, w1)).  prev = the target of segment j - 1, zero for j = 0 (a start from rest).
 *     t = tau - j * cmd_period - (j == 0 ? cmd_start : 0); alpha = cmd_ramp > 0 ?
 *     clamp((double)t / (double)cmd_ramp, 0, 1) : (t >= 0 ? 1 : 0).  v_ref[b][0, 1, 5] = target
 *     when alpha == 1, prev when alpha == 0, else prev + (target - prev) * alpha; v_ref[b][2, 3,
 *     4] = 0.  With commands == 0 v_ref[b] is written as zeros.
 *   Pushes (pushes != 0): none while tau < push_first; else window j = push_period > 0 ?
 *     (tau - push_first) / push_period : 0; philox(b, epoch, 4j, 2): jitter = int(0,
 *     push_jitter + 1, w0), occurs = prob(w1, push_prob), w2 = the flip bits; the window starts
 *     at s = push_first + j * push_period + jitter and is active iff occurs and s <= tau <
 *     s + push_ticks.  Its wrench: philox(b, epoch, 4j + 1 + i / 2, 2) for i = 0..5 gives
 *     range(wrench_lo[i], wrench_hi[i], u) with u = u(w0, w1) for even i, u(w2, w3) for odd i,
 *     negated when bit i of push_flip and bit i of w2 are both set.  push[b] = that wrench while
 *     active, else zeros; wrench_out[b] = wrench_in[b] (zeros if NULL) + push[b] component by
 *     component while active, else a plain copy of wrench_in[b].  With pushes == 0 push[b] is
 *     zeros and wrench_out[b] the copy. */
typedef struct mpcq_scenario_params {   /* 256 bytes */
  uint64_t seed;
  double v_lo[3], v_hi[3];              /* vx, vy, wyaw */
  double wrench_lo[6], wrench_hi[6];    /* force, then torque (a session: world frame) */
  double push_prob;                     /* in [0, 1] */
  double mass_scale_lo, mass_scale_hi, mu_lo, mu_hi;
  int32_t commands, cmd_start, cmd_ramp, cmd_period;
  int32_t pushes, push_first, push_period, push_jitter, push_ticks, push_flip;
  int32_t robots;                       /* bit 1: mass and gI scale, bit 2: mu */
  int32_t reserved[5];
} mpcq_scenario_params;
#ifdef __cplusplus
static_assert(sizeof(mpcq_scenario_params) == 256, "mpcq_scenario_params is 256 bytes");
#else
_Static_assert(sizeof(mpcq_scenario_params) == 256, "mpcq_scenario_params is 256 bytes");
#endif
/* The reference's predefined joystick at MPC ticks (Joystick.py:82 evaluates (k_loop - 960) /
 * 3500 at k_loop = 20 tau, the same rational as (tau - 48) / 175): seed 0, commands 1, v_lo =
 * v_hi = (1, 0, 0), cmd_start 48, cmd_ramp 175, cmd_period 0; pushes 0, push_prob 1, push_ticks
 * 10, the other push fields and both wrench bounds 0; mass_scale 1..1, mu 0.9..0.9, robots 0. */
void mpcq_default_scenario_params(mpcq_scenario_params* sc);
/* The scenario on its own, one tick for a batch.
 *   first      [B] int32 or NULL: nonzero = a first tick for this robot; all_first != 0: for all
 *   epoch, tick [B] int32 in/out
 *   base       [B] the rows the constants are applied to; NULL = ctx's mpcq_params (a host table
 *              is validated as in mpcq_set_robots, a device table is not)
 *   wrench_in  [B][6] or NULL (zeros)
 *   v_ref, push, wrench_out [B][6] out
 *   robots_out [B] or NULL, draw [B][8] or NULL: in/out, written on a robot's first tick only
 * sc NULL = mpcq_default_scenario_params.  Host pointers, or device pointers with
 * MPCQ_FLAG_DEVICE_PTRS (then MPCQ_FLAG_ASYNC does not wait for the stream).
 * MPCQ_E_INVALID, nothing launched: a NULL required pointer; a non-finite bound or lo > hi;
 * mass_scale_lo <= 0 with (robots & 1), mu_lo <= 0 with (robots & 2); push_prob outside [0, 1];
 * a negative integer field; push_ticks < 1 with pushes; cmd_period != 0 and cmd_period <
 * cmd_start + cmd_ramp, or push_period != 0 and push_jitter + push_ticks > push_period (the
 * two rules that keep a tick a function of one or two segments); robots beyond 3, push_flip
 * beyond 63; reserved not zero.  The parameters are checked before anything else. */
int mpcq_scenario_step_batch(mpcq_ctx* ctx, const mpcq_scenario_params* sc, int64_t batch,
                             const int32_t* first, int all_first, int32_t* epoch, int32_t* tick,
                             const mpcq_robot* base, const double* wrench_in, double* v_ref,
                             double* push, double* wrench_out, mpcq_robot* robots_out,
                             double* draw, uint32_t flags);

/* Opt-in (sc NULL = mpcq_default_scenario_params; invalid parameters: MPCQ_E_INVALID, nothing is
 * launched and the parameters in force stay): while enabled, every tick starts with one
 * scenario launch, before its planner, on the context's stream.  A robot is first there exactly
 * where the planner takes it as first (k == 0, or its MPCQ_SV_FIRST set by a reset or an
 * auto-reset).  The base rows of the constants: the plant's table if set, else the model's
 * table, else ctx's params, as they stand at the tick; the user's tables are never written.
 * wrench_in is MPCQ_PV_WRENCH (zeros before any mpcq_session_set_wrench).
 *   commands != 0: mpcq_session_tick and mpcq_session_run accept v_ref == NULL (v_ref_ticks is
 *     then ignored): planner and monitor take MPCQ_CV_V_REF.  A non-NULL v_ref wins;
 *     MPCQ_CV_V_REF is written all the same.  Without a scenario, or with commands == 0, a NULL
 *     v_ref stays MPCQ_E_INVALID.
 *   pushes != 0: the tick's plant launch takes MPCQ_CV_WRENCH in place of MPCQ_PV_WRENCH.
 *   robots != 0: the tick's plant launch takes MPCQ_CV_ROBOTS as its table.
 * Pushes and robots act only through an enabled plant; without one they are computed and unused.
 * The first call makes the MPCQ_CV_* arrays (zero, MPCQ_CV_ROBOTS the base rows) and enqueues
 * one launch that, for every robot, draws the constants of epoch 0 into MPCQ_CV_ROBOTS and
 * MPCQ_CV_DRAW and evaluates commands and pushes at tau = 0 without advancing MPCQ_CV_TICK: a
 * session enabled in mid-episode runs epoch 0 with tau counting from the enable; one enabled
 * before its first tick starts epoch 1 there.  Calling it again replaces the parameters and
 * keeps the arrays (the constants in force change at each robot's next first tick).  With
 * auto-reset alone, the n-th ended episode of robot b (MPCQ_MV_EPISODES) ran under epoch n.
 * A session that never enables it launches exactly what it did before. */
int mpcq_session_enable_scenario(mpcq_session* s, const mpcq_scenario_params* sc);
/* The ticks after it run without the scenario launch: the plant is back on the user's wrench
 * and tables, a NULL v_ref is MPCQ_E_INVALID again; the arrays stay. */
int mpcq_session_disable_scenario(mpcq_session* s);
/* The scenario's arrays; they exist from the first mpcq_session_enable_scenario on (before:
 * MPCQ_E_INVALID). */
#define MPCQ_CV_EPOCH 0     /* [B] int32   the running episode's number */
#define MPCQ_CV_TICK 1      /* [B] int32   the next tick's tau, unless that tick is a first one */
#define MPCQ_CV_V_REF 2     /* [B][6]      the last tick's command */
#define MPCQ_CV_PUSH 3      /* [B][6]      the last tick's push (zeros outside a window) */
#define MPCQ_CV_WRENCH 4    /* [B][6]      MPCQ_PV_WRENCH + MPCQ_CV_PUSH (world frame) */
#define MPCQ_CV_ROBOTS 5    /* [B] mpcq_robot  the running episode's true robots */
#define MPCQ_CV_DRAW 6      /* [B][8]      mass_scale, mu, (double)epoch, five zeros */
#define MPCQ_CV_COUNT 7
/* Copy array `what` to dst (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking. */
int mpcq_session_scenario_read(mpcq_session* s, int what, void* dst, uint32_t flags);
/* Device address of array `what` (valid until mpcq_session_destroy). */
int mpcq_session_scenario_device_ptr(mpcq_session* s, int what, void** out);

/* ---- channel: noisy, delayed state feedback and delayed forces ---------------
 * What lies between the plant and the controller, on the device: a measurement model in front
 * of the planner (delay, per-episode bias, per-tick noise, dropped frames) and an actuation
 * model in front of the plant (latency, per-episode leg gain, per-tick force noise).  One tick
 * of latency is the reference's asynchronous mode, where get_latest_result hands back the
 * previous solve and, on the first call, [0, 0, 8] * 4 (MPC_Wrapper.py:57-78; processing.py:
 * 133-145).  Everything else has no reference counterpart.  Every draw is a pure function of
 * (seed, robot, epoch, tau): a host restatement (mpcq/channel.py) agrees bit for bit.
 *
 * Clock [B][2] int32: the episode's number `epoch` and the next tick's `tau`, the channel's own
 * (no scenario needed) under the scenario's rule: on a tick where the robot is first, epoch += 1
 * and tau = 0; otherwise tau is the stored value; after the observe stage the stored value is
 * tau + 1.  A scenario enabled before the first tick has the same clock by construction.
 * A NEGATIVE stored tau is the bitwise complement of the tau to continue from and says that the
 * robot's rings are not filled yet: the next observe stage `primes` it (below).
 *
 * Generator: the scenario's Philox4x32-10 under the channel's seed, philox((b, epoch, c2,
 * stream), key), u(wa, wb) and prob(w, p) as above.  Streams (none shared with the scenario's):
 *   0x100 + i  state noise of component i             c2 = tau
 *   0x110      hold decision (w1)                     c2 = tau
 *   0x120 + j  force noise of force component j < 12  c2 = tau
 *   0x200 + i  episode bias of component i            c2 = 0
 *   0x210 + q  episode gain of leg q                  c2 = 0
 * Draw shapes:
 *   n(w)   = (double)((int64)(w0 + w1 + w2 + w3) - 8589934590) * (1.7320508075688772 * 2^-32)
 *   sym(w) = 2 * u(w0, w1) - 1
 * n is the centred sum of the four words at unit variance (Irwin-Hall of order 4: near-Gaussian,
 * |n| <= 2 sqrt(3)), exact up to one rounding; it needs no log / cos of a device library.  sym
 * is exact, in [-1, 1).
 *
 * Observe stage (per robot; truth [12] = the state the tick would have handed the planner).
 *   init = first or priming.  On an init tick: draw[i] = bias[i] * sym(stream 0x200 + i) for
 *     i < 12 and gain_q = 1 + f_gain * sym(stream 0x210 + q) for the epoch; every slot of the
 *     state ring <- truth; on a FIRST tick every slot of the force ring <- [0, 0, 8] * 4 and
 *     draw[12 + q] = gain_q; on a priming tick that is not first the force ring is left to the
 *     actuate stage, which fills it with that tick's own f0: until then draw[12] holds -gain_0
 *     (the gains are positive: the sign of draw[12] is that pending mark, nothing else).
 *   delayed = truth if delay == 0, else ring slot tau % delay read before truth is written into
 *     it: the truth of tick tau - delay, or the episode's (or the priming tick's) first truth
 *     before that.  The record is reported as it was written, in that tick's yaw-free local
 *     frame: it is not re-expressed in the current one.
 *   obs_i = (delayed_i + draw_i) + sigma[i] * n(stream 0x100 + i), no contraction.  A term whose
 *     amplitude (bias[i], sigma[i]) is exactly 0 is not added at all: -0.0 and NaN pass through,
 *     and a zero channel is a bitwise pass-through.
 *   hold: with hold_prob > 0, on a tick that is not init, prob(w1 of stream 0x110, hold_prob)
 *     makes obs the previous obs row (a dropped frame); the ring is advanced all the same.
 *   obs is written; the clock becomes (epoch, tau + 1).
 * Actuate stage (per robot; tau = stored - 1, taken as 0 where no observe stage has run).
 *   cmd = f0 if latency == 0, else force-ring slot tau % latency read before this tick's f0 is
 *     written there: the f0 of tick tau - latency, applied in the current local frame as
 *     commanded (as the reference applies a late result); before that the initial result above.
 *     With the pending mark set, every slot <- f0 first (so cmd = f0) and the mark is cleared.
 *   f_cmd[3q + a] = cmd * gain_q + f_sigma[a] * n(stream 0x120 + 3q + a), no contraction, the
 *     same zero-amplitude rule (f_gain == 0: no product; f_sigma[a] == 0: no sum). */
typedef struct mpcq_channel_params {   /* 256 bytes */
  uint64_t seed;                        /* the channel's own */
  int32_t delay;                        /* 0..8 ticks between a state and its observation */
  int32_t latency;                      /* 0..4 ticks between a solve and its forces */
  double hold_prob;                     /* in [0, 1]: a tick repeats the previous observation */
  double sigma[12];                     /* per-tick noise amplitude per state component */
  double bias[12];                      /* per-episode bias amplitude per state component */
  double f_sigma[3];                    /* per-tick force noise, x / y / z of every foot */
  double f_gain;                        /* per-episode leg gain amplitude, 0 <= f_gain < 1 */
  int32_t reserved[2];
} mpcq_channel_params;
#define MPCQ_CHANNEL_MAX_DELAY 8
#define MPCQ_CHANNEL_MAX_LATENCY 4
#ifdef __cplusplus
static_assert(sizeof(mpcq_channel_params) == 256, "mpcq_channel_params is 256 bytes");
#else
_Static_assert(sizeof(mpcq_channel_params) == 256, "mpcq_channel_params is 256 bytes");
#endif
/* Everything zero: a channel that changes nothing. */
void mpcq_default_channel_params(mpcq_channel_params* ch);
/* The observe stage on its own, one tick for a batch.
 *   first   [B] int32 or NULL: nonzero = a first tick for this robot; all_first != 0: for all
 *   truth   [B][12]
 *   clock   [B][2] int32 in/out;  obs [B][12] in/out (a held tick reads it);  draw [B][16]
 *   in/out;  s_ring [B][8][12] in/out;  f_ring [B][4][12] in/out (written on a first tick only)
 * All are required but first.  ch NULL = mpcq_default_channel_params.  Host pointers, or device
 * pointers with MPCQ_FLAG_DEVICE_PTRS (then MPCQ_FLAG_ASYNC does not wait for the stream).
 * MPCQ_E_INVALID, nothing launched, the message naming the field: delay outside 0..8, latency
 * outside 0..4, hold_prob outside [0, 1] or NaN, a negative, NaN or infinite sigma, bias,
 * f_sigma or f_gain, f_gain >= 1, reserved not zero; a NULL required pointer.  The parameters
 * are checked before anything else. */
int mpcq_channel_observe_batch(mpcq_ctx* ctx, const mpcq_channel_params* ch, int64_t batch,
                               const int32_t* first, int all_first, const double* truth,
                               int32_t* clock, double* obs, double* draw, double* s_ring,
                               double* f_ring, uint32_t flags);
/* The actuate stage on its own, after the observe stage of the same tick.
 *   f0 [B][12];  clock [B][2] int32 (read);  draw [B][16] in/out (the pending mark);
 *   f_ring [B][4][12] in/out;  f_cmd [B][12] out.  All required; flags and errors as above. */
int mpcq_channel_actuate_batch(mpcq_ctx* ctx, const mpcq_channel_params* ch, int64_t batch,
                               const double* f0, const int32_t* clock, double* draw,
                               double* f_ring, double* f_cmd, uint32_t flags);

/* Opt-in (ch NULL = mpcq_default_channel_params; invalid parameters: MPCQ_E_INVALID naming the
 * field, nothing is launched and the parameters in force stay).  While enabled a tick runs
 *   - the observe stage after its scenario stage and the staging of its inputs, before the
 *     planner: truth = the staged copy of MPCQ_SV_STATE, or the caller's state; a robot is
 *     first exactly where the planner takes it as first (k == 0, or its MPCQ_SV_FIRST set).
 *     The planner takes MPCQ_HV_OBS as its state: column 0 of MPCQ_SV_XREF is the observation,
 *     bit for bit.  l_feet is not disturbed.  Whatever else reads the tick's state, the plant,
 *     keeps reading the truth;
 *   - the actuate stage directly before the plant launch, only in ticks that run the plant:
 *     the plant takes MPCQ_HV_F_CMD in place of MPCQ_SV_F0, and its own rules then apply (a
 *     swing foot applies none, clamp to the true robot's cone): MPCQ_PV_F_EFF is what acted,
 *     MPCQ_SV_F0 stays the MPC's.
 * Without a plant the retrieve makes the prediction from the OBSERVATION the next state, so
 * measurement error enters the virtual robot's state and accumulates; that is allowed.
 * The first call makes the MPCQ_HV_* arrays, zero.  Whenever the channel was not enabled, or
 * delay or latency differ from those in force, the call enqueues one small launch that
 * complements every non-negative stored tau (on new arrays: -1), so the next observe stage
 * primes every robot: rings filled, draw drawn for the stored epoch, tau continuing; a robot
 * that is first there starts its new epoch as usual.  Calling it again with the same delay and
 * latency only replaces the amplitudes (a bias or gain in force changes at the robot's next
 * first tick).  A reset or an auto-reset needs nothing of its own: the first flags carry it.
 * A session that never enables it launches exactly what it did before. */
int mpcq_session_enable_channel(mpcq_session* s, const mpcq_channel_params* ch);
/* The ticks after it run without the two launches; the arrays stay. */
int mpcq_session_disable_channel(mpcq_session* s);
/* The channel's arrays; they exist from the first mpcq_session_enable_channel on (before:
 * MPCQ_E_INVALID).  The ring depths are the maxima whatever delay and latency are. */
#define MPCQ_HV_CLOCK 0     /* [B][2] int32  epoch, the next tick's tau (negative: see above) */
#define MPCQ_HV_OBS 1       /* [B][12]       the last tick's observation */
#define MPCQ_HV_F_CMD 2     /* [B][12]       the last plant tick's commanded forces */
#define MPCQ_HV_DRAW 3      /* [B][16]       the episode's 12 biases and 4 leg gains */
#define MPCQ_HV_S_RING 4    /* [B][8][12]    the last truths, slot tau % delay */
#define MPCQ_HV_F_RING 5    /* [B][4][12]    the last f0, slot tau % latency */
#define MPCQ_HV_COUNT 6
/* Copy array `what` to dst (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking. */
int mpcq_session_channel_read(mpcq_session* s, int what, void* dst, uint32_t flags);
/* Device address of array `what` (valid until mpcq_session_destroy). */
int mpcq_session_channel_device_ptr(mpcq_session* s, int what, void** out);

/* ---- estimator: a delay-compensating state estimator in front of the planner --
 * The controller's side of the channel, on the device: per robot a Kalman filter on the MPC's
 * own discrete model that keeps its posterior at the time the measurement was taken (`lag`
 * ticks ago) and predicts forward to now through the forces the MPC commanded and the
 * footholds it planned.  No reference counterpart (the reference reads the simulator's ground
 * truth); tests/estimator_model.py restates every rule below on the host.
 *
 * Model step M(x, feet, f): the plant's MPCQ_PLANT_MODEL step (mpcq_plant_step_batch above)
 * without clamp and without wrench, with dt and gravity of the context's mpcq_params and the
 * robot row the CONTROLLER believes (the robots argument / the session's mpcq_session_set_robots
 * table, else the context's params; never the plant's table), followed by the state part of
 * the tick's frame change: x, y and yaw <- 0, (vx, vy) and (wx, wy) rotated by Rz(-yaw_end).
 * The operation order is that of those two, no contraction, sums over feet left to right in
 * foot order; a foot with any NaN coordinate is a swing foot and applies no force.
 *
 * Filter state, one row of MPCQ_EST_ROW doubles per robot (nothing in it depends on a
 * parameter: no launch arms it, a snapshot needs no depth fields):
 *   [MPCQ_EST_POST  .. +12)  the posterior mean at filter time s
 *   [MPCQ_EST_PREV  .. +12)  the previous tick's observation row
 *   [MPCQ_EST_P     .. +18)  six symmetric 2x2 blocks (p_pp, p_pv, p_vv): block i couples
 *                            components i and i + 6 (a pose and its rate)
 *   [MPCQ_EST_CLOCK .. +2)   four int32: valid, s, tau_next, zero
 *   [MPCQ_EST_RING  .. +288) 12 slots of 24 doubles: slot j % 12 holds tick j's f0 [12] and
 *                            stance feet [3][4] (laid out as l_feet, NaN = swing)
 * tau is the filter's own count of ticks since its last initialisation.
 *
 * One robot-tick (obs [12] the measurement; f_prev, feet_prev the PREVIOUS tick's f0 and feet):
 *  1. Init, when any of: the robot is first; valid == 0; the previous tick failed; the stored
 *     s is not max(tau_next - 1 - lag, 0) (the lag changed under it).  Then post = obs, block
 *     P_i = diag(p0[i], p0[i + 6]), s = 0, tau = 0, valid = 1, est = obs bit for bit; the ring is
 *     not read before it is written.
 *  2. Otherwise tau = tau_next, and in this order:
 *     time update, with s* = max(tau - lag, 0): if s* == s + 1, post <- M(post, feet of tick s,
 *       force of tick s) and every block <- A P A^T + diag(q[i], q[i + 6]), A = [[1, dt], [0, 1]]
 *       (the MPC's own A): t = p_pv + dt p_vv; p_pp = ((p_pp + dt p_pv) + dt t) + q[i]; p_pv = t;
 *       p_vv = p_vv + q[i + 6]; for i in {0, 1, 5} the frame change pins the pose: p_pp = q[i],
 *       p_pv = 0.  The covariance ignores the small rotation of (vx, vy) and (wx, wy).  Its ring
 *       slots are read BEFORE the record below (at lag 8, f_lag 4 the force of tick tau - 13
 *       shares its slot with tick tau - 1).
 *     record: slot (tau - 1) % 12 <- f_prev, feet_prev.
 *     measurement update, skipped on a missing frame (a row with any non-finite component;
 *       with skip_repeats a row equal bit for bit to the previous tick's row: the channel's
 *       hold): per block S = P + diag(r[i], r[i + 6]), det = s00 s11 - s01 s01,
 *       K = P S^-1 (k00 = (p_pp s11 - p_pv s01) / det, k01 = (p_pv s00 - p_pp s01) / det,
 *       k10 = (p_pv s11 - p_vv s01) / det, k11 = (p_vv s00 - p_pv s01) / det), e = obs - post,
 *       post_i += k00 e_i + k01 e_{i+6}, post_{i+6} += k10 e_i + k11 e_{i+6}, and P -= K P
 *       (p_pp -= k00 p_pp + k01 p_pv; p_pv -= k00 p_pv + k01 p_vv; p_vv -= k10 p_pv + k11 p_vv).
 *     forecast: est = post taken tau - s* times (at most 8) through M over ticks s* .. tau - 1.
 *     `The force of tick j` is the f0 recorded for tick j - f_lag, and before that tick 0 the
 *     reference's initial result [0, 0, 8] * 4 (MPC_Wrapper.py:78).
 *  3. prev = obs, s = s*, tau_next = tau + 1 are stored.
 * With p0 = q = 0 every gain is exactly 0 (a pure model rollout from the first observation);
 * with an exact model and exact measurements every innovation is exactly 0 and est is the
 * truth.  A bias is unobservable with H = I and is not estimated. */
#define MPCQ_ESTIMATOR_MAX_LAG 8
#define MPCQ_ESTIMATOR_MAX_F_LAG 4
#define MPCQ_EST_POST 0
#define MPCQ_EST_PREV 12
#define MPCQ_EST_P 24
#define MPCQ_EST_CLOCK 42
#define MPCQ_EST_RING 44
#define MPCQ_EST_SLOTS 12   /* MPCQ_ESTIMATOR_MAX_LAG + MPCQ_ESTIMATOR_MAX_F_LAG */
#define MPCQ_EST_ROW 332    /* doubles: 2656 bytes, a multiple of 16 */
typedef struct mpcq_estimator_params {   /* 320 bytes */
  int32_t lag;                          /* 0..8: the age in ticks of a measurement (the channel's delay) */
  int32_t f_lag;                        /* 0..4: ticks between a solve and its forces (the channel's latency) */
  int32_t skip_repeats;                 /* nonzero: a repeated observation row is a missing frame */
  int32_t reserved[5];                  /* zero */
  double q[12];                         /* process variance per state component (c, rpy, v, w) */
  double r[12];                         /* measurement variance, > 0 */
  double p0[12];                        /* initial variance */
} mpcq_estimator_params;
#ifdef __cplusplus
static_assert(sizeof(mpcq_estimator_params) == 320, "mpcq_estimator_params is 320 bytes");
#else
_Static_assert(sizeof(mpcq_estimator_params) == 320, "mpcq_estimator_params is 320 bytes");
#endif
/* lag 0, f_lag 0, skip_repeats 1, p0 = 1e-2, q = 1e-6 (components 0..5) and 1e-4 (6..11),
 * r = 1e-4: starting values, not tuned; set r to the channel's sigma^2. */
void mpcq_default_estimator_params(mpcq_estimator_params* ep);
/* One tick of the filter for a batch, on its own.
 *   first       [B] int32 or NULL: nonzero = a first tick for this robot; all_first != 0: all
 *   obs         [B][12]
 *   f_prev      [B][12], feet_prev [B][3][4]: the previous tick's f0 and feet (not read by a
 *               robot that initialises)
 *   failed_prev [B] int32 or NULL: nonzero = the previous tick failed
 *   robots      [B] mpcq_robot or NULL (the context's params); a host table is validated as in
 *               mpcq_set_robots
 *   row         [B][MPCQ_EST_ROW] in/out (all zero: a new filter);  est [B][12] out
 * ep NULL = the defaults.  Host pointers, or device pointers with MPCQ_FLAG_DEVICE_PTRS (then
 * MPCQ_FLAG_ASYNC does not wait for the stream).  MPCQ_E_INVALID, nothing launched, the message
 * naming the field: lag outside 0..8, f_lag outside 0..4, r[i] <= 0, a negative q[i] or p0[i],
 * any NaN or infinity, reserved not zero; a NULL obs, f_prev, feet_prev, row or est.  The
 * parameters are checked before anything else. */
int mpcq_estimator_step_batch(mpcq_ctx* ctx, const mpcq_estimator_params* ep, int64_t batch,
                              const int32_t* first, int all_first, const double* obs,
                              const double* f_prev, const double* feet_prev,
                              const int32_t* failed_prev, const mpcq_robot* robots, double* row,
                              double* est, uint32_t flags);
/* Opt-in (ep NULL = the defaults; invalid parameters: MPCQ_E_INVALID naming the field, nothing
 * is launched and the parameters in force stay).  While enabled a tick runs the estimate stage
 * after its observe stage (or, without a channel, after the staging of its inputs) and before
 * the planner: obs = what the planner would have taken as its state (MPCQ_HV_OBS, or the staged
 * state); f_prev = MPCQ_SV_F0 and feet_prev = row 0 of MPCQ_SV_FSTEPS as they stand before this
 * tick's planner; the previous tick failed by the plant's rule (MPCQ_SV_STATUS none of SOLVED,
 * SOLVED_INACCURATE, MAX_ITER_REACHED, or a planner status); a robot is first exactly where the
 * planner takes it as first.  The planner takes MPCQ_EV_EST as its state: column 0 of
 * MPCQ_SV_XREF is the estimate, bit for bit.  The plant and the monitor keep reading the truth.
 * It works without a channel and without a plant.  A reset or an auto-reset needs nothing of its
 * own: the first flags carry it.
 * The first call makes the MPCQ_EV_* arrays, zero (valid = 0).  Enabling while not enabled
 * zeroes the rows again (a ring that missed ticks is stale).  Calling it while enabled only
 * replaces the parameters; a changed lag re-initialises each robot at its next tick by rule 1.
 * A session that never enables it launches exactly what it did before. */
int mpcq_session_enable_estimator(mpcq_session* s, const mpcq_estimator_params* ep);
/* The ticks after it run without the launch; the arrays stay. */
int mpcq_session_disable_estimator(mpcq_session* s);
/* The estimator's arrays; they exist from the first mpcq_session_enable_estimator on (before:
 * MPCQ_E_INVALID). */
#define MPCQ_EV_EST 0       /* [B][12]            the last tick's estimate (derived: not in snapshots) */
#define MPCQ_EV_ROW 1       /* [B][MPCQ_EST_ROW]  the filter state */
#define MPCQ_EV_COUNT 2
/* Copy array `what` to dst (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking. */
int mpcq_session_estimator_read(mpcq_session* s, int what, void* dst, uint32_t flags);
/* Device address of array `what` (valid until mpcq_session_destroy). */
int mpcq_session_estimator_device_ptr(mpcq_session* s, int what, void** out);

/* ---- gait transitions: per-robot target gaits through the roll ----------------
 * The reference's roll (FootstepPlanner.py:401-425) appends to the end of the horizon a copy of
 * the step it consumes at the front, so a gait table repeats itself for ever.  The gait stage
 * replaces that roll: the step that enters the horizon comes from a desired gait cycle, per
 * robot (mpcq_gait.hip).  tests/gait_model.py restates every rule below on the host; all
 * quantities are small integers, every comparison against it is exact.
 *
 * Library: n_gaits cycles (1..MPCQ_GAIT_MAX), each a [20][5] table in the gait table's own
 * format -- rows [count, c0, c1, c2, c3], ended by a row whose count is 0 -- holding ONE period
 * of a gait (its period P_g = the sum of its counts; no relation to N).  A valid cycle has 1 to
 * 19 rows, every count an integer in 1..64, every contact exactly 0.0 or 1.0, and everything
 * after the terminator row zero.  The one-row cycle [1, 1,1,1,1] is "stand".
 *
 * Per-robot state, [B][4] int32 (want, active, phase, switches); (-1, -1, 0, 0) after enable and
 * after any reset of the robot.  want: the requested library entry (-1: none).  active: the
 * entry whose cycle is being appended (-1: the table repeats itself, the reference's roll).
 * phase: the next step of that cycle, in [0, P_active).  switches: how many switches were taken.
 * The kernel is defensive about what it reads: an active or a want outside [-1, n_gaits) is read
 * as -1, and phase is taken mod P_active, so a restored or hand-written row cannot index outside
 * a cycle.
 *
 * One call per robot (a session: once per tick, tick 0 included):
 * 1. selection, with select = MPCQ_GAIT_BY_SPEED only: s = sqrt(vx vx + vy vy) + yaw_weight |wz|
 *    of this call's v_ref (no contraction).  want < 0 (and s not NaN): want = the number of
 *    thresholds[i], i < n_gaits - 1, with s >= thresholds[i].  Otherwise want moves up while
 *    want < n_gaits - 1 and s > thresholds[want] + hysteresis; if it did not move up, it moves
 *    down while want > 0 and s < thresholds[want - 1] - hysteresis.  A NaN s leaves want alone.
 * 2. switch: index = the first row whose count is 0, last = index - 1 (row 19 for index 0, as
 *    the reference's gait[index - 1] wraps).  A table without a zero row: NOTHING is written,
 *    neither table nor state (the planner's own test then ends the tick as
 *    MPCQ_STATUS_BAD_GAIT).  With want >= 0 and want != active: boundary = (active >= 0) ? phase
 *    is the first step of a row of the active cycle : the contacts of row 0 differ from those
 *    of row last (the reference's "create a new phase" branch: the step about to be appended
 *    starts a phase of the running gait), or index == 1.  If boundary, or align == 0: active =
 *    want, phase = 0, switches += 1.
 * 3. roll: the new contacts are step `phase` of cycle `active`, then phase = (phase + 1) mod
 *    P_active; with active = -1 they are the contacts of row 0.  The rest is the reference's
 *    roll: equal to row last's contacts: that row's count += 1, else row index = [1, contacts];
 *    then the front row's count is decremented where it is > 1, else the rows shift up and row
 *    19 is zeroed.  The sum of the counts never changes.
 * With align = 1 the running gait contributes only whole phases to the horizon and the new one
 * starts at the start of its cycle: no swing phase is cut short at the seam (one may be
 * lengthened). */
#define MPCQ_GAIT_MAX 8
#define MPCQ_GAIT_MANUAL 0     /* want is what mpcq_session_set_gait last wrote */
#define MPCQ_GAIT_BY_SPEED 1   /* the kernel picks want from the commanded speed */
typedef struct mpcq_gait_params {        /* 128 bytes */
  int32_t n_gaits;                      /* 1..MPCQ_GAIT_MAX: the library's entries */
  int32_t select;                       /* MPCQ_GAIT_MANUAL or MPCQ_GAIT_BY_SPEED */
  int32_t align;                        /* 1: switch only at a phase boundary; 0: at once */
  int32_t reserved0;                    /* zero */
  double thresholds[7];                 /* speed bands: the first n_gaits - 1, non-decreasing, +inf allowed */
  double hysteresis;                    /* >= 0 */
  double yaw_weight;                    /* >= 0, metres per rad/s */
  double reserved[5];                   /* zero */
} mpcq_gait_params;
#ifdef __cplusplus
static_assert(sizeof(mpcq_gait_params) == 128, "mpcq_gait_params is 128 bytes");
#else
_Static_assert(sizeof(mpcq_gait_params) == 128, "mpcq_gait_params is 128 bytes");
#endif
/* n_gaits 0 (to be set), MPCQ_GAIT_MANUAL, align 1, thresholds all +inf, hysteresis 0,
 * yaw_weight 0.2421053541332781 = sqrt(0.19^2 + 0.15005^2): the distance of the default
 * planner's shoulders from the centre, the speed of a foot under a pure turn of 1 rad/s. */
void mpcq_default_gait_params(mpcq_gait_params* gp);
/* The gait kernel on its own: one call of the rules above for every robot of a batch.
 *   gp      the parameters (host, required);  cycles [n_gaits][20][5] doubles (host, required)
 *   v_ref   [B][6], read with MPCQ_GAIT_BY_SPEED only (may be NULL with MPCQ_GAIT_MANUAL)
 *   gait    [B][20][5] in/out;  gstate [B][4] int32 in/out
 * v_ref, gait and gstate are host pointers, or device pointers with MPCQ_FLAG_DEVICE_PTRS (then
 * MPCQ_FLAG_ASYNC does not wait for the stream).  MPCQ_E_INVALID, nothing launched, the message
 * naming the field: n_gaits outside 1..8; select or align not 0 or 1; one of the first
 * n_gaits - 1 thresholds NaN or below its predecessor; hysteresis or yaw_weight negative or not
 * finite; a reserved field not zero; a cycle that breaks the library rules (the message names
 * the gait, the row and the field).  The parameters and cycles are checked before anything else. */
int mpcq_gait_roll_batch(mpcq_ctx* ctx, const mpcq_gait_params* gp, const double* cycles, int64_t batch,
                         const double* v_ref, double* gait, int32_t* gstate, uint32_t flags);
/* Opt-in (invalid parameters or cycles: MPCQ_E_INVALID, nothing is launched and the settings in
 * force stay).  While enabled a tick runs the gait stage between its first tick's
 * footsteps-only planner pass and its main planner pass, on MPCQ_SV_GAIT, MPCQ_GV_STATE and the
 * v_ref the planner reads (the scenario's or the staged command), and launches the main pass
 * without its own roll (MPCQ_PLAN_FOOTSTEPS | MPCQ_PLAN_REFSTATES).  A reset or an auto-reset
 * puts the robot's row back to (-1, -1, 0, 0).  The first call makes MPCQ_GV_STATE, every row
 * (-1, -1, 0, 0); calling it again replaces library and parameters, and the rows stay (under
 * the defensive reads above).  A session that never enables it launches exactly what it did
 * before.  One difference to the planner's own roll shows with the stage enabled: a roll that
 * fills row 19 without a shift is written (the planner discards it), and the planner's test
 * then ends that tick as MPCQ_STATUS_BAD_GAIT, as it would end the next one. */
int mpcq_session_enable_gait(mpcq_session* s, const mpcq_gait_params* gp, const double* cycles);
/* The ticks after it run the planner's own roll again; the array stays. */
int mpcq_session_disable_gait(mpcq_session* s);
/* Requests: want[b] = ids[b], ids [B] int32, each in [-1, n_gaits); host, or device with
 * MPCQ_FLAG_DEVICE_PTRS (| MPCQ_FLAG_ASYNC: not blocking).  A host array is validated (the
 * message names the first offending index); a device array is copied on the stream and covered
 * by the kernel's defensive read.  Only want is written: -1 withdraws a request that has not
 * been taken yet, a gait that is already active stays active.  MPCQ_E_INVALID under
 * MPCQ_GAIT_BY_SPEED (the kernel owns want) and before mpcq_session_enable_gait. */
int mpcq_session_set_gait(mpcq_session* s, const int32_t* ids, uint32_t flags);
/* The gait array; it exists from the first mpcq_session_enable_gait on (before: MPCQ_E_INVALID). */
#define MPCQ_GV_STATE 0     /* [B][4] int32     want, active, phase, switches */
#define MPCQ_GV_COUNT 1
/* Copy array `what` to dst (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking. */
int mpcq_session_gait_read(mpcq_session* s, int what, void* dst, uint32_t flags);
/* Device address of array `what` (valid until mpcq_session_destroy). */
int mpcq_session_gait_device_ptr(mpcq_session* s, int what, void** out);

/* ---- disturb: a disturbance observer in front of the solve ---------------------
 * The one piece of a session that did not react to a payload the controller does not know or
 * to a steady push was the controller's own model.  This stage estimates, on the device, the
 * constant acceleration the model lacks from consecutive states and the model itself, and hands
 * it to the solve as each robot's mpcq_disturbance row (mpcq_disturb.hip).  (`observe` is the
 * channel's stage; this one is `disturb`.)  No reference counterpart; tests/disturb_model.py
 * restates every rule below on the host.
 *
 * Row, MPCQ_DIST_ROW doubles per robot (nothing in it depends on a parameter: no launch arms
 * it, a snapshot needs no depth fields):
 *   [MPCQ_DIST_D     .. +6)   d, the estimate, in the frame of the last tick that ran
 *   [MPCQ_DIST_PREV  .. +12)  the previous tick's measurement
 *   [MPCQ_DIST_CLOCK .. +2)   four int32: valid, tau_next, zero, zero
 *   [MPCQ_DIST_RING  .. +60)  5 slots of 12 doubles: slot j % 5 holds tick j's f0
 * tau is the stage's own count of ticks since its last first tick.
 *
 * One robot-tick (meas [12] what the planner is about to take as its state; f_prev, feet_prev
 * the PREVIOUS tick's f0 and stance feet; M the estimator's model step above, with the robot
 * the CONTROLLER believes, never the plant's):
 *  1. First tick, when the robot is first, valid == 0, or the stored tau_next < 1.  Then d = 0,
 *     prev = meas, tau_next = 1, valid = 1, the output row is zero, the ring is neither read nor
 *     written (a new episode may have drawn a new payload).
 *  2. Otherwise tau = tau_next, and in this order:
 *     record: slot (tau - 1) % 5 <- f_prev.
 *     acting force: the f0 recorded for tick tau - 1 - f_lag, and before tick 0 the reference's
 *       [0, 0, 8] * 4 (MPC_Wrapper.py:78): the estimator's rule.
 *     frame change: psi = prev[5] + dt * prev[11] (the bits of M's yaw at the end of the tick);
 *       with c = cos psi, s = sin psi, (d0, d1) and (d3, d4) become (c d0 + s d1, -s d0 + c d1);
 *       d2 and d5 stay.  A psi that is not finite leaves d as it is.
 *     sample, unless: the previous tick failed (the plant's rule, as in the estimator); meas or
 *       prev has a non-finite component; with skip_repeats, meas equals prev bit for bit (the
 *       channel's hold).  pred = M(prev, feet_prev, acting force); r[i] = (meas[6+i] -
 *       pred[6+i]) / dt.  The plant's physics do not care what the MPC believed, so r samples
 *       the whole lumped disturbance whether or not the last solve compensated: the update
 *       carries no "previously applied" term.
 *     update: with a sample whose six r are finite, d[i] = d[i] + alpha[i] * (r[i] - d[i]).
 *     clip: d[i] to [-d_max[i], d_max[i]].
 *  3. prev = meas and tau_next = tau + 1 are stored; the output row's a = d, reserved zero; the
 *     diagnostic row = r (NaN where no sample was taken).
 * With alpha = 0 the estimate stays zero exactly; with alpha = 1 it follows the last sample.
 * Known limit: the estimator's forecast model does not include the disturbance, so behind a
 * channel with lag > 0 its estimate carries a near-constant rate offset, which largely cancels
 * in the difference of consecutive estimates that this stage samples. */
#define MPCQ_DISTURB_MAX_F_LAG 4
#define MPCQ_DIST_D 0
#define MPCQ_DIST_PREV 6
#define MPCQ_DIST_CLOCK 18
#define MPCQ_DIST_RING 20
#define MPCQ_DIST_SLOTS 5   /* MPCQ_DISTURB_MAX_F_LAG + 1 */
#define MPCQ_DIST_ROW 80    /* doubles: 640 bytes, a multiple of 16 */
typedef struct mpcq_disturb_params {     /* 128 bytes */
  double alpha[6];                      /* the filter's gain per component, each in [0, 1] */
  double d_max[6];                      /* > 0: the estimate is clipped to +-d_max[i] */
  int32_t f_lag;                        /* 0..4: ticks between a solve and its forces (the channel's latency) */
  int32_t compensate;                   /* nonzero: a session's solve takes MPCQ_DV_DIST as its disturbance table */
  int32_t skip_repeats;                 /* nonzero: a repeated measurement row yields no sample */
  int32_t reserved[5];                  /* zero */
} mpcq_disturb_params;
#ifdef __cplusplus
static_assert(sizeof(mpcq_disturb_params) == 128, "mpcq_disturb_params is 128 bytes");
#else
_Static_assert(sizeof(mpcq_disturb_params) == 128, "mpcq_disturb_params is 128 bytes");
#endif
/* alpha = 0.2, d_max = 5 m/s^2 (linear) and 30 rad/s^2 (angular), f_lag 0, compensate 1,
 * skip_repeats 1: starting values, not tuned. */
void mpcq_default_disturb_params(mpcq_disturb_params* dp);
/* One tick of the stage for a batch, on its own.
 *   first       [B] int32 or NULL: nonzero = a first tick for this robot; all_first != 0: all
 *   meas        [B][12]
 *   f_prev      [B][12], feet_prev [B][3][4]: the previous tick's f0 and feet (not read by a
 *               robot that runs a first tick)
 *   failed_prev [B] int32 or NULL: nonzero = the previous tick failed
 *   robots      [B] mpcq_robot or NULL (the context's params); a host table is validated as in
 *               mpcq_set_robots
 *   row         [B][MPCQ_DIST_ROW] in/out (all zero: a new stage)
 *   dist        [B] mpcq_disturbance out;  resid [B][6] out or NULL
 * dp NULL = the defaults.  Host pointers, or device pointers with MPCQ_FLAG_DEVICE_PTRS (then
 * MPCQ_FLAG_ASYNC does not wait for the stream).  MPCQ_E_INVALID, nothing launched, the message
 * naming the field: an alpha[i] outside [0, 1], a d_max[i] <= 0, f_lag outside 0..4, any NaN or
 * infinity, reserved not zero; a NULL meas, f_prev, feet_prev, row or dist.  The parameters are
 * checked before anything else. */
int mpcq_disturb_step_batch(mpcq_ctx* ctx, const mpcq_disturb_params* dp, int64_t batch,
                            const int32_t* first, int all_first, const double* meas,
                            const double* f_prev, const double* feet_prev,
                            const int32_t* failed_prev, const mpcq_robot* robots, double* row,
                            mpcq_disturbance* dist, double* resid, uint32_t flags);
/* Opt-in (dp NULL = the defaults; invalid parameters: MPCQ_E_INVALID naming the field, nothing
 * is launched and the parameters in force stay).  While enabled a tick runs the stage after its
 * estimate stage and before the planner ([scenario] -> inputs -> [observe] -> [estimate] ->
 * [disturb] -> planner -> solve -> ...): meas = what the planner is about to take as its state
 * (MPCQ_EV_EST, MPCQ_HV_OBS, or the staged state; the stage does not change it); f_prev =
 * MPCQ_SV_F0 and feet_prev = row 0 of MPCQ_SV_FSTEPS as they stand before this tick's planner;
 * failed and first as in the estimator; the robot is the session's mpcq_session_set_robots
 * table, else the context's params.  With compensate the tick's solve takes MPCQ_DV_DIST as its
 * disturbance table: it then takes precedence over the table of mpcq_session_set_disturbance.
 * With compensate == 0 the stage only estimates, and the solve takes the user's table if there
 * is one.  One more small launch per tick, nothing on the host.  It works without plant,
 * channel or estimator.  A reset or an auto-reset needs nothing of its own: the first flags
 * carry it.
 * The first call makes the MPCQ_DV_* arrays, zero (valid = 0).  Enabling while not enabled
 * zeroes the rows again (a ring that missed ticks is stale).  Calling it while enabled only
 * replaces the parameters.  A session that never enables it launches exactly what it did
 * before. */
int mpcq_session_enable_disturb(mpcq_session* s, const mpcq_disturb_params* dp);
/* The ticks after it run without the launch (and the solve takes the user's table again); the
 * arrays stay. */
int mpcq_session_disable_disturb(mpcq_session* s);
/* The stage's arrays; they exist from the first mpcq_session_enable_disturb on (before:
 * MPCQ_E_INVALID). */
#define MPCQ_DV_DIST 0      /* [B] mpcq_disturbance   what the solve reads (derived: not in snapshots) */
#define MPCQ_DV_ROW 1       /* [B][MPCQ_DIST_ROW]     the stage's state */
#define MPCQ_DV_RESID 2     /* [B][6]                 the last tick's raw sample, NaN where none was taken
                                                      (derived, for diagnostics: not in snapshots) */
#define MPCQ_DV_COUNT 3
/* Copy array `what` to dst (host, or device with MPCQ_FLAG_DEVICE_PTRS); blocking. */
int mpcq_session_disturb_read(mpcq_session* s, int what, void* dst, uint32_t flags);
/* Device address of array `what` (valid until mpcq_session_destroy). */
int mpcq_session_disturb_device_ptr(mpcq_session* s, int what, void** out);

/* ---- snapshots: save, restore and branch robots on the device ---------------
 * A snapshot is a device-resident copy of everything per-robot that a session holds, plus the
 * few host flags that decide what the next tick launches.  Every call below runs on the
 * context's stream: behind the ticks already queued, ahead of later ones.  No reference
 * counterpart (the reference runs one robot forward).
 *
 * What a snapshot holds: every array of every group the session has allocated when it is
 * saved -- the main group (MPCQ_SV_F0 .. _H_ROT, MPCQ_SV_FIRST, the warm start, the planner's
 * status, the engine's info, the creation gait table), the swing arrays (after
 * mpcq_session_enable_swing), MPCQ_PV_* (after _enable_plant / _set_wrench), MPCQ_MV_* (after
 * _enable_monitor), MPCQ_CV_* (after _enable_scenario), MPCQ_HV_* (after _enable_channel), MPCQ_EV_ROW (after
 * _enable_estimator; the row is self-describing, so a restore into a session with another lag is
 * legal and re-initialises by the filter's rule 1; MPCQ_EV_EST is derived, rewritten by every
 * tick before anything reads it, and left out: after a restore it shows the session's last tick
 * until the next one), MPCQ_GV_STATE (after _enable_gait; the gait library and parameters are the controller's
 * configuration and are not held, so a restore needs a session whose library has as many
 * cycles), MPCQ_DV_ROW (after _enable_disturb; self-describing like the estimator's row;
 * MPCQ_DV_DIST and MPCQ_DV_RESID are derived, rewritten by every tick of the stage before
 * anything reads them, and left out), and the tables of mpcq_session_set_robots / _set_plant_robots where in force -- and its shape: N,
 * B, which of these exist, the swing k_mpc, the channel's delay and latency in force at the
 * save (the rings mean nothing under others: a restore into a session whose values differ is
 * MPCQ_E_INVALID); and whether a tick has run since create and whether a reset was ever called.  Not held: the staging of host inputs and the plant's copy of q_w (every
 * tick rewrites them before reading), and MPCQ_SV_ORDER (a permutation, not a per-robot row;
 * the restore rebuilds it, and results do not depend on it).  Parameters and enable flags
 * (swing, plant, monitor, scenario parameters; _enable_* / _disable_*) are configuration, not
 * robots' state: the session's own, never touched.  So is the table of
 * mpcq_session_set_weights, the controller's tuning, and the table of
 * mpcq_session_set_disturbance: a snapshot holds neither (the blob of a session with a table is
 * byte for byte the blob without one) and no restore touches them.
 *
 * create: no device memory until the first save.  The snapshot belongs to s's context (hence
 * its N and stream) and may be restored into any session of that context.  A snapshot may be
 * destroyed after its session; one whose session is gone is good for _destroy, _bytes and
 * _export, and for a restore into another session of the context.  Destroy every snapshot
 * before mpcq_destroy of the context.  destroy(NULL) is MPCQ_OK. */
typedef struct mpcq_snapshot mpcq_snapshot;
int mpcq_session_snapshot_create(mpcq_session* s, mpcq_snapshot** out);
int mpcq_session_snapshot_destroy(mpcq_snapshot* snap);
/* Capture s as it stands behind the queued ticks: whole-array device-to-device copies.
 * Saving again re-captures, and reallocates when the shape changed (one allocation per group;
 * a failed one leaves the snapshot as it was).  Blocking unless flags has MPCQ_FLAG_ASYNC (a
 * save that has to allocate blocks all the same). */
int mpcq_session_snapshot_save(mpcq_session* s, mpcq_snapshot* snap, uint32_t flags);
/* Robot b of s takes row map[b] of snap; map [B_session] int32, -1 = leave this robot alone
 * (not one byte of it is written).  The same row may appear any number of times (branching);
 * the snapshot's batch may differ from the session's (seeding).  map == NULL: the identity
 * over every robot; it needs B_snapshot == B_session and also restores the batch-wide
 * MPCQ_MV_TOTALS, which a mapped restore leaves alone.
 * Requirements, else MPCQ_E_INVALID naming the first difference, with nothing launched and
 * the session as it was: snap saved; the same context; the same shape as at the save (the same
 * groups allocated, the same swing k_mpc, each table in force or not as then); a host map's
 * entries -1 or in [0, B_snapshot) (the message names the first offending index); and a mapped
 * restore of ticked state into a session that has not ticked yet covers every robot (no -1;
 * the others would run a warm tick on creation state), from a host map.
 * map is a host pointer (the call blocks) or, with MPCQ_FLAG_DEVICE_PTRS, a device pointer
 * (with | MPCQ_FLAG_ASYNC the call enqueues and returns, as mpcq_session_reset).  A device
 * map cannot be validated: an entry outside [0, B_snapshot) acts as -1.
 * A restored robot gets its row of every array the snapshot holds, in ONE launch
 * (gather_rows_kernel) up to 48 arrays, in two beyond (a session with every group enabled has
 * 50), each on the stream.  After it, where the session or the snapshot has a dispatch order in
 * use, MPCQ_SV_ORDER is rebuilt from the restored iteration counts and pending resets.  A
 * reset recorded in the snapshot stays recorded in the session.
 * A snapshot saved before any tick holds creation state, which only a first tick may consume:
 * its rows come with MPCQ_SV_FIRST[b] = 1, so restoring such a row is exactly a pending
 * mpcq_session_reset of that robot.
 * k stays the caller's: after restoring ticked state, call the next tick with k > 0 (the
 * planner and the engine read k only as zero or non-zero).
 * Scenarios: the draws are a function of (seed, slot b, epoch, tau).  A robot restored into
 * slot b inherits the source's MPCQ_CV_EPOCH, _TICK and the running episode's true robot
 * (MPCQ_CV_ROBOTS, MPCQ_CV_DRAW); from the next tick on it draws slot b's own commands and
 * pushes at that (epoch, tau): branches of one robot live through different futures from one
 * state.  On the host a branch's constants are those of (map[b], epoch) for the running
 * episode and of (b, epoch) from its next restart on. */
int mpcq_session_snapshot_restore(mpcq_session* s, const mpcq_snapshot* snap, const int32_t* map,
                                  uint32_t flags);
/* Save into a snapshot the session owns (made on first use, freed by mpcq_session_destroy),
 * then restore from it with map (not NULL): the one-call form of branching inside a live
 * session.  The source is never the live arrays: map may be any mapping. */
int mpcq_session_fork(mpcq_session* s, const int32_t* map, uint32_t flags);
/* Checkpoint to the host.  One blob = a 128-byte header, then the groups' arrays unpadded, in
 * the order main, swing, plant, monitor, scenario, robots table, plant robots table, channel,
 * estimator, gait, disturb, inside a group by array id (the private main arrays behind the named ones).  The
 * header, little endian: char magic[8] "MPCQSNP1"; uint32 version (3 with an estimator part, else
 * 2 with a channel part, else 1: a session without either writes the version-1 blob byte for
 * byte, one with a channel and no estimator the version-2 blob; import reads all three); int32
 * N; int64 B; int32 k_mpc (0: no swing arrays); uint32 flags (bit 0 a tick had run, 1 a reset
 * was recorded, 2 swing, 3 plant, 4 monitor, 5 scenario, 6 robots table, 7 plant robots table,
 * 8 channel, 9 estimator); int64 group_bytes[7]; int64 total (header included); int64 user (0; for the
 * caller, ignored by import); at offset 104 int64 bytes of the channel part; at 112 int32
 * delay, latency in force at the save; at 120 int64 bytes of the estimator part (MPCQ_EV_ROW).
 * Format version 4 (a session with MPCQ_GV_STATE; flags bit 10) has a 144-byte header: at 128
 * int64 bytes of the gait part, at 136 int32 n_gaits, at 140 int32 zero.
 * Format version 5 (a session with MPCQ_DV_ROW; flags bit 11) has a 160-byte header: the
 * version-4 header (its gait fields zero without a gait part), at 144 int64 bytes of the disturb
 * part (MPCQ_DV_ROW), at 152 int64 zero.
 * _bytes: the size of snap's blob (snap saved).  _export: dst is a host buffer of exactly
 * that many bytes; blocking.  _import: makes snap the snapshot the blob describes, for s's
 * context; before it touches the device it checks the magic, the version, N against the
 * context, and that the group byte counts follow from the header's shape and sum to `bytes`: a
 * truncated or foreign blob is MPCQ_E_INVALID and snap stays as it was. */
int mpcq_session_snapshot_bytes(const mpcq_snapshot* snap, int64_t* bytes);
int mpcq_session_snapshot_export(const mpcq_snapshot* snap, void* dst, int64_t bytes);
int mpcq_session_snapshot_import(mpcq_session* s, mpcq_snapshot* snap, const void* src, int64_t bytes);

/* ---- diagnostics -----------------------------------------------------------
 * Device buffer [B][16] (uint64) that a diagnostic build of the library
 * (compiled with -DMPCQ_STAMPS, libmpcq_stamps.so) fills with per-phase
 * s_memtime cycle counts of thread 0; ignored by the shipped build. */
int mpcq_debug_set_stamps(mpcq_ctx* ctx, void* device_buffer);

/* The dispatch-order layer on its own (no reference counterpart; tests/test_gpu_dispatch.py
 * pins these kernels to a host model).  Every pointer is a host pointer, every call blocks,
 * none launches the engine or adds work to a solve.
 *
 * The class table of MPCQ_FLAG_ORDER_BY_CLASS: mpcq_debug_class_table_slots() slots, per slot
 * the sum of the iteration counts learned and their number (uint64 each).  A context that has
 * not solved with the flag yet holds the all-zero table. */
int mpcq_debug_class_table_slots(void);
int mpcq_debug_class_table_read(mpcq_ctx* ctx, uint64_t* sum, uint64_t* cnt);
int mpcq_debug_class_table_write(mpcq_ctx* ctx, const uint64_t* sum, const uint64_t* cnt);
/* The class order of fsteps [B][20][13] on ctx's table as it stands: cls [B] = each instance's
 * slot, order [B] = the dispatch order (what a solve with the flag would use now). */
int mpcq_debug_class_order(mpcq_ctx* ctx, int64_t batch, const double* fsteps, int32_t* cls,
                           int32_t* order);
/* Adds iters [B] to the slots cls [B] of ctx's table (entries with iters <= 0 are not counted);
 * a slot outside the table is MPCQ_E_INVALID. */
int mpcq_debug_class_learn(mpcq_ctx* ctx, int64_t batch, const int32_t* cls, const int32_t* iters);
/* The status value a sliced solve's first launch leaves on a suspended instance (internal:
 * no caller of a solve ever sees it). */
int mpcq_debug_suspended_status(void);
/* The resumed launch's list: of prev [n] (NULL: 0..n-1; instance indices below n_inst, else
 * MPCQ_E_INVALID) the instances whose status [n_inst] is the suspended one, the largest
 * key [n_inst][2] (element 0) first in buckets of 1/8 octave, prev's order inside a bucket.
 * list [n]: *count entries are written. */
int mpcq_debug_suspended(mpcq_ctx* ctx, int64_t n, int64_t n_inst, const int32_t* prev,
                         const int32_t* status, const double* key, int32_t* list, int32_t* count);
/* The session's order of its next tick (MPCQ_SV_ORDER) from iters [B]. */
int mpcq_debug_session_order(mpcq_ctx* ctx, int64_t batch, const int32_t* iters, int32_t* order);
/* What the last mpcq_solve_batch / mpcq_qp_solve_batch of ctx dispatched by, read from the
 * scratch the context keeps (so before the next solve).  Every output is optional (NULL).
 * batch: its batch B (0: no solve yet); sliced: whether it ran as two launches; by_class:
 * whether it used the class order; cls [B], order [B]: the slots and the first launch's order
 * (by_class only; otherwise untouched); list [B], count: the resumed launch's instances, in its
 * order (list[*count..B) = -1; sliced only, otherwise *count = 0); key [B][2]: element 0 of a
 * listed instance is the key it was ranked by (sliced only; otherwise untouched). */
int mpcq_debug_last_dispatch(mpcq_ctx* ctx, int64_t* batch, int32_t* sliced, int32_t* by_class,
                             int32_t* cls, int32_t* order, int32_t* list, int32_t* count, double* key);

/* The restore's gather kernel on its own (tests/test_gpu_snapshot.py pins it to numpy's fancy
 * indexing): n arrays (at most 48); array i has rows of row_bytes[i] bytes (a multiple of 4),
 * src[i] rows_src of them, dst[i] rows_dst; dst row b <- src row map[b] for every i, in one
 * launch; an entry outside [0, rows_src) leaves row b alone; map NULL = the identity.  src,
 * dst and row_bytes are host tables; what src[i], dst[i] and map point to is host memory, or
 * device memory (4-byte aligned) with MPCQ_FLAG_DEVICE_PTRS (| MPCQ_FLAG_ASYNC: not blocking). */
int mpcq_debug_gather_rows(mpcq_ctx* ctx, int n, const void* const* src, void* const* dst,
                           const int64_t* row_bytes, int64_t rows_src, int64_t rows_dst,
                           const int32_t* map, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* MPCQ_H */
