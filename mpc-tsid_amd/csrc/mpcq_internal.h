// mpcq_internal.h — shared between the HIP kernels and the host C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mpcq.h"

namespace mpcq {

// Per-launch arguments.  Every pointer is a device pointer.  Optional arrays
// may be null.  Layouts are the ones documented in include/mpcq.h.
struct LaunchArgs {
  int64_t batch;
  int mode;            // formulation mode (fused path)
  const double* xref;  // [B][12][N+1]   (fused / formulate)
  const double* fsteps;// [B][20][13]    (fused / formulate)
  const double* Ax;    // [B][nnz]       (qp path)
  const double* l;     // [B][m]         (qp path)
  const double* u;     // [B][m]         (qp path)
  const double* warm_x;// [B][n]
  const double* warm_y;// [B][m]
  const double* rho_in;// [B]
  double* Ax_out;      // [B][nnz]       (formulate)
  double* l_out;       // [B][m]
  double* u_out;       // [B][m]
  double* f0;          // [B][12]
  double* x;           // [B][n]
  double* y;           // [B][m]
  int32_t* status;     // [B]
  int32_t* iters;      // [B]
  double* rho_out;     // [B]
  int32_t* info;       // [B][4]: rho updates, polish status, polish rounds, reserved
  uint64_t* stamps;    // [B][16] diagnostic build only (MPCQ_STAMPS): cycles per phase
  double* work;        // [B][work_doubles(N)] engine workspace (N > 32)
  const int32_t* order; // [B] instance solved by workgroup i (a permutation of 0..B-1), or null: i
  // sliced solves (mpcq_set_slice): slice_iters > 0 suspends an instance at the first segment
  // end (a check / adaptive-rho / max_iter boundary of the ADMM loop) after slice_iters more
  // iterations: its iterate and loop counters to res / res_rho / res_i, status
  // kStatusSuspended, no other output.  resume != 0: every instance of this launch starts from
  // its saved iterate (the formulation, scaling and factorisation at the saved rho recomputed:
  // the same bits) instead of the cold point.
  int32_t slice_iters;
  int32_t resume;
  const int32_t* batch_dev;  // (the resumed launch) the count of workgroups with work, on the device:
                             // the launch is sized for the whole batch, workgroups past it return
  double* res;          // [B][8][res_lanes(N)]: xf, xX, z[3], y[3] of every lane
  double* res_rho;      // [B]
  double* res_key;      // [B][2]: the primal / dual residual over its tolerance half way through the
                        // slice, then (at suspension) [b][0] = the iterations left, extrapolated from
                        // their decay since -- the resumed launch's order
  int32_t* res_i;       // [B][8]: next iteration, to the next check, to the next adaptation, rho
                        // updates, the half-way sample's iteration, 3 spare
  // [B] per-instance mass, gI, mu, fz_max (mpcq_set_robots), or null: the launch's mpcq_params.
  // Indexed by the instance (after the order[] mapping), never by the workgroup; read by the
  // formulation only: not null selects the engine's ROB instantiations.
  const mpcq_robot* robots;
  // [B] or null (a session after mpcq_session_reset): nonzero = this instance (after the
  // order[] mapping) runs a first tick -- MPCQ_MODE_SETUP and a cold start that reads none of
  // warm_x, warm_y, rho_in -- whatever mode and the warm pointers say.  Batch solves: null.
  const int32_t* first;
  // [B] per-instance diagonal of P (mpcq_set_weights, mpcq_session_set_weights), indexed by the
  // instance like robots.  The ROB instantiations read both tables, so the host passes both or
  // neither: where one table is set and the other is not, the missing one is a device table of
  // the context's values (mpcq_api.cpp launch_tables).  Null with robots null.
  const mpcq_weights* weights;
  // [B] per-instance constant disturbance acceleration (mpcq_set_disturbance,
  // mpcq_session_set_disturbance), indexed by the instance like robots; read by the formulation
  // (dyn_bound) of the ROB instantiations, the formulation-only one included.  Passed with the
  // other two tables or not at all; a table that is not set is one of zeros.
  // (Last, so that the other arguments keep their offsets.)
  const mpcq_disturbance* disturb;
};
constexpr int32_t kStatusSuspended = 100;  // (internal: the host loop resumes these)
// The plant's rule, which every stage of a session shares: a robot whose solve ended in none of
// SOLVED, SOLVED_INACCURATE, MAX_ITER_REACHED, or whose planner failed (where the reference
// raises), failed its tick.
__host__ __device__ inline bool solve_failed(int status, int plan_status) {
  return !(status == MPCQ_STATUS_SOLVED || status == MPCQ_STATUS_SOLVED_INACCURATE ||
           status == MPCQ_STATUS_MAX_ITER_REACHED) || plan_status != 0;
}
constexpr int64_t res_lanes(int N) { return 16 * (int64_t)((N + 3) & ~3); }

// Doubles of engine workspace per instance: 0 up to 32 stages (everything in LDS);
// beyond, a 288-double pad, S^{-1} (N x 144 + 2), F W (N x 72), R^{-1} Q (N x 36),
// a zero block (72), beyond 49 stages the scaled constraint values (126 N - 18,
// rounded up to even), beyond 48 every lane's row of F_k (12 x 16 x the stage rows, N
// rounded up to 4); the F W block stays reserved (F W lives in LDS since round 3)
// (One formula: the layouts that had their own -- three or four 16-stage instances per CU, the
// nested-dissection solve -- were measured slower and removed; their code is kept as
// tools/attic/engine_variants_round6.patch, their measurements in DESIGN.md sections 8b item 4
// and 8 item 1.)
constexpr int64_t work_doubles(int N) {
  return N > 32 ? 288 + (int64_t)N * (144 + 72 + 36) + 2 + 72 + (N > 49 ? ((126 * N - 18 + 1) & ~1) : 0) +
                      (N > 48 ? (int64_t)12 * 16 * ((N + 3) & ~3) : 0)
                : 0;
}
static_assert(work_doubles(16) == 0 && work_doubles(32) == 0 && work_doubles(33) == 8678 && work_doubles(48) == 12458 &&
                  work_doubles(49) == 22694 && work_doubles(50) == 29228 && work_doubles(64) == 36824,
              "the engine workspace per instance (doubles)");
// Sliced solves (LaunchArgs::slice_iters / resume): the engine holds the suspend / resume code
// beyond 16 stages only (mpcq_engine.hip kSlice), and the host takes its two-launch path only
// there: a unit without the code ignores slice_iters, resume and batch_dev.
constexpr bool slice_supported(int N) { return N > 16; }
static_assert(!slice_supported(16) && slice_supported(17), "slicing starts at 17 stages");

// Planner launch (mpcq_planner.hip); layouts in include/mpcq.h (mpcq_plan_batch).
struct PlanArgs {
  int64_t batch;
  int N;
  unsigned ops;        // MPCQ_PLAN_* bits
  int k;
  const double* state; // [B][12]
  const double* v_cur; // [B][6] or null (state[6:12])
  const double* h;     // [B] or null (state[2])
  const double* l_feet;// [B][3][4]
  const double* v_ref; // [B][6]
  const int32_t* reduced; // [B] or null
  double* gait;        // [B][20][5] in/out
  int32_t* rot_flag;   // [B] in/out
  double* h_rot;       // [B] in/out
  double* xref;        // [B][12][N+1] in/out
  double* fsteps;      // [B][20][13] out
  int32_t* status;     // [B] or null
  // [B] or null (a session after mpcq_session_reset): instance b plans with k = 0 where
  // first[b] != 0, else with k; a launch of MPCQ_PLAN_FOOTSTEPS alone (the first tick's
  // extra pass) then touches only the instances with first[b] != 0
  const int32_t* first;
};

hipError_t launch_plan(const mpcq_planner_params& pp, const PlanArgs& a, hipStream_t s);

// Session epilogue (mpcq_session.hip): one robot per wave64.
struct SessionArgs {
  int64_t batch;
  const double* x;       // [B][24N] solution of this tick
  const double* xref;    // [B][12][N+1]
  const double* fsteps;  // [B][20][13]
  const double* gait;    // [B][20][5]
  int32_t* status;       // [B] engine status, overridden by a planner failure
  const int32_t* plan_status;  // [B]
  double* x_robot;       // [B][12][N]
  double* warm_x;        // [B][24N] next tick's warm start
  double* y;             // [B][44N] reset to 0 after a failed solve
  double* rho;           // [B]      reset to rho0 after a failed solve
  double rho0;
  double* cost;          // [B][13]
  double* q_w;           // [B][6]
  double* next_state;    // [B][12]
  double* next_l_feet;   // [B][3][4]
  double state_weights[12];
  double force_weight;
  const mpcq_weights* weights;  // [B] or null: the two by-value fields above (mpcq_session_set_weights)
  double shoulders[8];
  int32_t* first;        // [B] or null: cleared (the robot's pending reset is served)
};

hipError_t launch_retrieve(int N, const SessionArgs& a, hipStream_t s);
// Dispatch order of the next tick's solve (mpcq_session.hip): the robots sorted by
// this tick's iteration counts, longest first (buckets of 16 iterations); first [B] or
// null: a robot with a pending reset (a cold solve next) goes into the top bucket.
hipError_t launch_order(const int32_t* iters, const int32_t* first, int64_t batch, int32_t* order, hipStream_t s);

// mpcq_session_reset (mpcq_session.hip): the per-robot arrays of the robots with
// mask[b] != 0 (null: all) to the state of a new robot; one wave64 per robot.
// mpcq_session_create launches it too (over its zeroed allocation, first null): the only
// statement of that state.
struct ResetArgs {
  int64_t batch;
  int N;
  const int32_t* mask;   // [B] or null
  const double* gait_src;// [B][20][5]: the caller's gait0 or the session's creation table
  const double* q_w0;    // [B][6] or null: the default pose
  double h_ref, rho0;
  double shoulders[8];
  double* gait;          // [B][20][5]
  int32_t* rot_flag;     // [B]
  double* h_rot;         // [B]
  double* xref;          // [B][12][N+1]
  double* fsteps;        // [B][20][13]
  double* q_w;           // [B][6]
  double* state;         // [B][12]
  double* l_feet;        // [B][3][4]
  double* rho;           // [B]
  double* y;             // [B][44N]
  double* warm_x;        // [B][24N]
  double* x;             // [B][24N]
  double* f0;            // [B][12]
  double* x_robot;       // [B][12][N]
  double* cost;          // [B][13]
  int32_t* status;       // [B]
  int32_t* iters;        // [B]
  int32_t* first;        // [B] set to 1 (a reset is pending), or null: not marked
  // the swing arrays, or null on a session without them
  double* swing_ref;     // [B][swing_ref_doubles]
  int64_t swing_ref_doubles;
  double* swing_state;   // [B][4][MPCQ_SWING_STATE]
  double* frame;         // [B][3]
  // the monitor's running episode, or null on a session without a monitor: discarded
  double* ep;            // [B][8]
  int32_t* ep_ticks;     // [B]
  // the gait stage's rows, or null on a session that never enabled it: back to (-1, -1, 0, 0)
  int32_t* gstate;       // [B][4]
};
hipError_t launch_reset(const ResetArgs& a, hipStream_t s);

// Dispatch order of a batch solve by gait class (mpcq_order.hip, MPCQ_FLAG_ORDER_BY_CLASS):
// cls[B] = each instance's class slot, order[B] = the instances by the expected cost their
// class has shown on this context (sum / cnt: class_table_slots() entries), the most
// expensive first, index order inside a cost bucket; launch_class_learn adds a launch's
// iteration counts to the table.
int class_table_slots();
hipError_t launch_class_order(const double* fsteps, int64_t batch, int32_t* cls, const uint64_t* sum,
                              const uint64_t* cnt, int32_t* order, hipStream_t s);
hipError_t launch_class_learn(const int32_t* cls, const int32_t* iters, int64_t batch, uint64_t* sum,
                              uint64_t* cnt, hipStream_t s);
// Sliced solves: list[*count] = the instances of prev[0..n) (null: 0..n-1) whose status is
// kStatusSuspended, the largest key (key[2 id]: the iterations left, extrapolated) first, in
// prev's order inside a key bucket (one workgroup; buckets of 1/8 octave).  res_i (LaunchArgs::res_i
// of the launch just ended, or null): the half-way sample's iteration of every instance of prev
// is reset to 0 (none) for the next sliced call.
hipError_t launch_suspended(const int32_t* prev, int64_t n, const int32_t* status, const double* key,
                            int32_t* list, int32_t* count, int32_t* res_i, hipStream_t s);

// Swing-foot trajectories (mpcq_swing.hip); layouts in include/mpcq.h (mpcq_swing_batch).
struct SwingArgs {
  int64_t batch;
  int k_sub0, n_sub;
  const double* gait;   // [B][20][5]
  const double* fsteps; // [B][20][13]
  const double* frame;  // [B][3]
  const double* feet0;  // [B][4][6] or null
  double* state;        // [B][4][40] in/out
  double* ref;          // [B][n_sub][4][9]
  double* t0_out;       // [B][n_sub][4] or null
  int32_t* status;      // [B] or null
};
hipError_t launch_swing(const mpcq_swing_params& sp, const SwingArgs& a, hipStream_t s);
// one get_next_foot per (robot, foot): in [B][4][10], state [B][4][40], out [B][4][11]
hipError_t launch_swing_step(const mpcq_swing_params& sp, int64_t batch, const double* in, double* state,
                             double* out, hipStream_t s);

// Rigid-body plant (mpcq_plant.hip); layouts and equations in include/mpcq.h
// (mpcq_plant_step_batch, mpcq_session_enable_plant).  One thread per robot.
struct PlantArgs {
  int64_t batch;
  const double* state;     // [B][12]
  const double* feet;      // [B][3][4], or null with fsteps
  const double* fsteps;    // [B][20][13] (a session's tick): the feet are row 0's
  const double* f;         // [B][12]
  const double* wrench;    // [B][6] or null
  const mpcq_robot* robots;// [B] or null: dflt
  mpcq_robot dflt;
  double* state_out;       // [B][12]
  double* f_eff;           // [B][12] or null
  // a session's tick only (tail != 0): the wrench is a world-frame one, rotated by
  // Rz(-q_w_prev[5]); a failed robot gets NaN rows and nothing else; the others' world pose
  // and virtual robot are rewritten from the plant's end state (mpcq_virtual.h)
  int tail;
  const int32_t* status;      // [B] after the retrieve
  const int32_t* plan_status; // [B]
  const double* gait;         // [B][20][5]
  const double* q_w_prev;     // [B][6] the world pose before the tick
  double* q_w;                // [B][6]
  double* next_state;         // [B][12]
  double* next_l_feet;        // [B][3][4]
  double shoulders[8];
};
hipError_t launch_plant(const mpcq_plant_params& pl, const PlantArgs& a, hipStream_t s);

// Episode monitor (mpcq_monitor.hip); semantics and layouts in include/mpcq.h
// (mpcq_monitor_step_batch, mpcq_session_enable_monitor).  One thread per robot.
struct MonitorArgs {
  int64_t batch;
  const double* q_w;       // [B][6]
  const int32_t* status;   // [B]
  const int32_t* iters;    // [B]
  const double* f0;        // [B][12]
  const double* cost;      // [B][13]
  const double* state;     // [B][12]
  const double* v_ref;     // [B][6]
  double* ep;              // [B][8] in/out
  int32_t* ep_ticks;       // [B] in/out
  int32_t* episodes;       // [B] in/out, or null
  double* last;            // [B][16] or null
  int32_t* done;           // [B] out
  unsigned long long* totals;  // [8] or null
  double* trace;           // [B][MPCQ_TRACE] or null
};
hipError_t launch_monitor(const mpcq_monitor_params& mp, const MonitorArgs& a, hipStream_t s);

// Scenario stage (mpcq_scenario.hip); semantics and layouts in include/mpcq.h
// (mpcq_scenario_step_batch, mpcq_session_enable_scenario).  One thread per robot.
struct ScenarioArgs {
  int64_t batch;
  const int32_t* first;    // [B] or null: nonzero = a first tick
  int all_first;           // every robot runs a first tick
  // mpcq_session_enable_scenario's launch: the constants of the stored epoch and the tick's
  // values at the stored tau, neither advanced
  int init;
  int32_t* epoch;          // [B] in/out
  int32_t* tick;           // [B] in/out
  const mpcq_robot* base;  // [B] or null: dflt
  mpcq_robot dflt;
  const double* wrench_in; // [B][6] or null: zeros
  double* v_ref;           // [B][6]
  double* push;            // [B][6]
  double* wrench_out;      // [B][6]
  mpcq_robot* robots_out;  // [B] or null
  double* draw;            // [B][8] or null
};
hipError_t launch_scenario(const mpcq_scenario_params& sc, const ScenarioArgs& a, hipStream_t s);

// Channel stages (mpcq_channel.hip); semantics and layouts in include/mpcq.h
// (mpcq_channel_observe_batch / _actuate_batch, mpcq_session_enable_channel).  Sixteen lanes
// per robot, lane c < 12 owns component c.
struct ObserveArgs {
  int64_t batch;
  const int32_t* first;  // [B] or null: nonzero = a first tick
  int all_first;         // every robot runs a first tick
  const double* truth;   // [B][12]
  int32_t* clock;        // [B][2] in/out
  double* obs;           // [B][12] in/out
  double* draw;          // [B][16] in/out
  double* s_ring;        // [B][8][12] in/out
  double* f_ring;        // [B][4][12]: written on a first tick
};
struct ActuateArgs {
  int64_t batch;
  const double* f0;      // [B][12]
  const int32_t* clock;  // [B][2]
  double* draw;          // [B][16]: the pending mark in the sign of draw[12]
  double* f_ring;        // [B][4][12] in/out
  double* f_cmd;         // [B][12] out
};
hipError_t launch_observe(const mpcq_channel_params& ch, const ObserveArgs& a, hipStream_t s);
hipError_t launch_actuate(const mpcq_channel_params& ch, const ActuateArgs& a, hipStream_t s);
// mpcq_session_enable_channel's launch: every non-negative stored tau to its complement
hipError_t launch_channel_arm(int32_t* clock, int64_t batch, hipStream_t s);

// What the stages that run the controller's model read, alone (mpcq_*_step_batch) or in a
// session's tick: the measurement, the previous tick's forces, feet and failure, the robot the
// controller believes.
struct ModelInputs {
  int64_t batch;
  const int32_t* first;    // [B] or null: nonzero = a first tick
  int all_first;           // every robot runs a first tick
  const double* meas;      // [B][12]
  const double* f_prev;    // [B][12]
  const double* feet_prev; // [B][3][4], or null with fsteps
  const double* fsteps;    // [B][20][13] (a session's tick): the feet are row 0's
  const int32_t* failed;   // [B] or null: nonzero = the previous tick failed
  // a session's tick: the previous tick's statuses, failed by solve_failed (failed null)
  const int32_t* status;      // [B] or null
  const int32_t* plan_status; // [B]
  const mpcq_robot* robots;// [B] or null: dflt
  mpcq_robot dflt;
  double dt, gravity;      // the context's
};

// Estimate stage (mpcq_estimator.hip); semantics and layouts in include/mpcq.h
// (mpcq_estimator_step_batch, mpcq_session_enable_estimator).  Sixteen lanes per robot.
struct EstimateArgs : ModelInputs {
  double* row;             // [B][MPCQ_EST_ROW] in/out
  double* est;             // [B][12] out
};
hipError_t launch_estimate(const mpcq_estimator_params& ep, const EstimateArgs& a, hipStream_t s);

// Disturbance stage (mpcq_disturb.hip); semantics and layouts in include/mpcq.h
// (mpcq_disturb_step_batch, mpcq_session_enable_disturb).  Sixteen lanes per robot.
struct DisturbArgs : ModelInputs {
  double* row;             // [B][MPCQ_DIST_ROW] in/out
  mpcq_disturbance* dist;  // [B] out
  double* resid;           // [B][6] out, or null
};
hipError_t launch_disturb(const mpcq_disturb_params& dp, const DisturbArgs& a, hipStream_t s);

// Gait stage (mpcq_gait.hip); semantics and layouts in include/mpcq.h (mpcq_gait_roll_batch,
// mpcq_session_enable_gait).  Thirty-two lanes per robot, lane r < 20 owns row r of its table.
// The library travels in the kernel arguments: one word per cycle row (gait_pack), the
// periods beside it (1 for the entries past n_gaits: never a divisor of zero).
constexpr int32_t gait_pack(int count, int contacts) { return count | (contacts << 8); }  // count 1..64, 4 bits
struct GaitArgs {
  int64_t batch;
  const double* v_ref;   // [B][6], or null with MPCQ_GAIT_MANUAL
  double* gait;          // [B][20][5] in/out
  int32_t* gstate;       // [B][4] in/out
  int32_t period[MPCQ_GAIT_MAX];
  int32_t lib[MPCQ_GAIT_MAX * 20];
};
hipError_t launch_gait(const mpcq_gait_params& gp, const GaitArgs& a, hipStream_t s);

// Row gather of a snapshot restore (mpcq_snapshot.hip; semantics in include/mpcq.h,
// mpcq_session_snapshot_restore / mpcq_debug_gather_rows): row b of every dst array <- row
// map[b] of its src array, in one launch.  The table travels in the kernel arguments.
constexpr int kGatherMax = 48;      // arrays per launch
constexpr int kGatherNarrow = 32;   // rows up to this many bytes: one lane per robot; above: one wave
struct GatherDesc {
  const void* src;    // rows_src rows of row_bytes
  void* dst;          // rows_dst rows of row_bytes
  int32_t row_bytes;  // a multiple of vec
  int32_t vec;        // bytes per access: 16, 8 or 4 (what row_bytes and both bases are aligned to)
};
struct GatherArgs {
  int64_t rows_src, rows_dst;
  const int32_t* map;  // [rows_dst] or null: the identity; an entry outside [0, rows_src) = skip this robot
  int32_t* first;      // [rows_dst] or null: set to 1 for every robot that is written
  // d[0 .. n_wide): row_bytes > kGatherNarrow, sorted by vec: [0, n_wide16) 16, [n_wide16, n_wide8) 8,
  // [n_wide8, n_wide) 4; d[n_wide .. n): the others
  int32_t n_wide16, n_wide8, n_wide, n;
  GatherDesc d[kGatherMax];
};
// The access width for an array: the widest of 16 / 8 / 4 that divides row_bytes and both
// addresses, or 0 (not a multiple of 4).
int gather_vec(const void* src, const void* dst, int64_t row_bytes);
hipError_t launch_gather_rows(const GatherArgs& a, hipStream_t s);

// Launchers (mpcq_engine.hip).  Return hipError_t.
hipError_t launch_formulate(int N, const mpcq_params& p, const LaunchArgs& a, hipStream_t s);
hipError_t launch_solve(int N, bool fused, const mpcq_params& p, const LaunchArgs& a, hipStream_t s);
// the horizons the engine is compiled for (mpcq_dispatch.cpp, Makefile)
#define MPCQ_HORIZONS(X)                                                                                     \
  X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) X(22)  \
  X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32) X(33) X(34) X(35) X(36) X(37) X(38) X(39) X(40)  \
  X(41) X(42) X(43) X(44) X(45) X(46) X(47) X(48) X(49) X(50) X(51) X(52) X(53) X(54) X(55) X(56) X(57) X(58)  \
  X(59) X(60) X(61) X(62) X(63) X(64)
bool horizon_supported(int N);
int supported_horizons(int32_t* out, int cap);

}  // namespace mpcq
