// mpcq_host.h — what the two host units of the C ABI share: mpcq_api.cpp (contexts, batch
// entry points, diagnostics; it defines everything declared here) and mpcq_session_api.cpp
// (closed-loop sessions).
#pragma once
#include "mpcq_internal.h"

// A table of per-instance records on the device -- the robots' constants (mpcq_set_robots,
// mpcq_session_set_robots), the cost weights (mpcq_set_weights, mpcq_session_set_weights) or the
// disturbance accelerations (mpcq_set_disturbance, mpcq_session_set_disturbance):
// count > 0 = in force.
template <class R>
struct Table {
  static_assert(sizeof(R) % 64 == 0, "a table record is 8 or 16 doubles");
  R* dev = nullptr;
  int64_t cap = 0;
  int64_t count = 0;
};
using RobotTable = Table<mpcq_robot>;
using WeightsTable = Table<mpcq_weights>;
using DisturbTable = Table<mpcq_disturbance>;
// The engine's ROB kernels read all three tables.  Where a table is not set beside one that is,
// it is one of these: a device table of the context's own values (the disturbance's: zeros),
// made at the first launch that needs it and grown with the batch (the context's mpcq_params
// never change after mpcq_create).
struct FillTables {
  RobotTable robots;
  WeightsTable weights;
  DisturbTable disturb;
};

struct mpcq_ctx {
  int device = 0;
  int N = 0;
  mpcq_params p{};
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  void* arena = nullptr;
  size_t arena_bytes = 0;
  void* work = nullptr;  // engine workspace (horizons beyond 32 stages)
  size_t work_bytes = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool have_form = false, have_solve = false;
  uint64_t* stamps = nullptr;
  // MPCQ_FLAG_ORDER_BY_CLASS: the class table (sum of iterations, count per slot) and the
  // per-instance scratch (class slot, dispatch order, iteration counts when the caller
  // passes none)
  uint64_t* cls_sum = nullptr;
  uint64_t* cls_cnt = nullptr;
  int32_t* ord_buf = nullptr;
  int64_t ord_cap = 0;
  // what the last batch solve dispatched by (mpcq_debug_last_dispatch): host bookkeeping only
  int64_t last_B = 0;
  bool last_by_class = false, last_sliced = false;
  // sliced solves (mpcq_set_slice): the slice length (0: off), the suspended instances'
  // iterates (mpcq::res_lanes(N) x 8 doubles, rho, key, 4 counters each), the resumed launch's
  // dispatch list (B int32, of 3 B: two once held alternating lists) and a status scratch, the
  // resumed launch's workgroup count (device)
  int32_t slice_iters = 0;
  double* res = nullptr;
  double* res_rho = nullptr;
  double* res_key = nullptr;
  int32_t* res_i = nullptr;
  int32_t* sl_buf = nullptr;
  int64_t sl_cap = 0;
  int32_t* sl_count = nullptr;
  RobotTable robots;  // mpcq_set_robots
  WeightsTable weights;  // mpcq_set_weights
  DisturbTable disturb;  // mpcq_set_disturbance
  FillTables fill;
};

namespace mpcq {

// Sets the calling thread's mpcq_last_error text; returns code.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return mpcq::fail(MPCQ_E_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));  \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != d) (void)hipSetDevice(d);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int check_ctx(mpcq_ctx* c, int64_t batch);
// The engine's per-instance workspace (mpcq::work_doubles(N), zero up to 32 stages).
int ensure_work(mpcq_ctx* c, int64_t B, double** out);
// Replace (count > 0) or clear a table.  The copy runs on the context's stream, behind any
// queued launch that still reads the old values; from a host pointer the call then blocks.
int set_table(mpcq_ctx* c, RobotTable& t, int64_t count, const mpcq_robot* robots, uint32_t flags);
int set_table(mpcq_ctx* c, WeightsTable& t, int64_t count, const mpcq_weights* weights, uint32_t flags);
int set_table(mpcq_ctx* c, DisturbTable& t, int64_t count, const mpcq_disturbance* rows, uint32_t flags);
// The tables a formulating launch of `batch` instances reads, into a->robots / weights /
// disturb: all null where none is set (the kernels of a launch without a table), else all not
// null, the missing ones from `fill`.  MPCQ_E_INVALID, and nothing to launch, where a table in
// force is shorter than the batch.  weights null: a formulation-only launch, which has no P --
// a->weights stays null, and a weights table in force is not looked at.
int launch_tables(mpcq_ctx* c, const RobotTable& robots, const WeightsTable* weights, const DisturbTable& disturb,
                  FillTables& fill, int64_t batch, LaunchArgs* a);
void free_tables(FillTables& fill);
// The caller's parameters (null: the defaults) into *out, or MPCQ_E_INVALID.
int swing_params(const mpcq_swing_params* sp, mpcq_swing_params* out);
int plant_params(const mpcq_plant_params* pl, double dt_default, mpcq_plant_params* out);
int monitor_params(const mpcq_monitor_params* mp, mpcq_monitor_params* out);
int scenario_params(const mpcq_scenario_params* sc, mpcq_scenario_params* out);
int channel_params(const mpcq_channel_params* ch, mpcq_channel_params* out);
int estimator_params(const mpcq_estimator_params* ep, mpcq_estimator_params* out);
int disturb_params(const mpcq_disturb_params* dp, mpcq_disturb_params* out);
// The gait stage's parameters (no defaults: n_gaits is the caller's) and its library, validated:
// *out, and the cycles packed into lib->lib / lib->period (the other fields of *lib zero).
int gait_params(const mpcq_gait_params* gp, const double* cycles, mpcq_gait_params* out, GaitArgs* lib);
}  // namespace mpcq
