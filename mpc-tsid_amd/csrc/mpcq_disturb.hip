// mpcq_disturb.hip — the disturbance stage of a closed-loop session on MI355X, between the
// estimate stage and the planner: per robot an observer that samples, from two consecutive
// states and the controller's own model, the constant acceleration the model lacks (a payload
// it does not know, a steady push), filters it, and hands it to the solve as the robot's
// mpcq_disturbance row (include/mpcq.h, mpcq_disturb_step_batch / mpcq_session_enable_disturb).
// No reference counterpart: the reference's model knows gravity only.
//
// Sixteen lanes per robot (mpcq_stage16.h).  The rows are the measurement, the previous
// measurement, the ring slots and the estimate.  Each lane runs the robot's whole tick, the model
// step included, so the sums over feet run left to right in foot order on every lane and the
// bits are the plant's.  The one word this launch both stores and may need again (the previous
// tick's f0, at f_lag 0) travels in registers, and the ring has MAX_F_LAG + 1 slots, so the slot
// recorded is never the slot read.  One model step per robot: the launch's cost is latency.  FP64
// without contraction: tests/disturb_model.py restates it in numpy and differs by the device
// library's sin / cos.
#include <math.h>

#include "mpcq_internal.h"

#pragma clang fp contract(off)

#include "mpcq_model.h"
#include "mpcq_stage16.h"

namespace mpcq {
namespace {

constexpr int kSlots = MPCQ_DIST_SLOTS;
static_assert(kSlots == MPCQ_DISTURB_MAX_F_LAG + 1, "the ring holds f_lag + 1 ticks");
static_assert(MPCQ_DIST_RING + kSlots * 12 == MPCQ_DIST_ROW && MPCQ_DIST_ROW % 2 == 0, "the stage's row");
static_assert(MPCQ_DIST_PREV == MPCQ_DIST_D + 6 && MPCQ_DIST_CLOCK == MPCQ_DIST_PREV + 12 &&
                  MPCQ_DIST_RING == MPCQ_DIST_CLOCK + 2, "the stage's row");

__global__ __launch_bounds__(64) void disturb_kernel(mpcq_disturb_params dp, DisturbArgs a) {
  const Lane16 ln = lane16();
  const int c = ln.c, cc = ln.cc, c6 = ln.c6;
  const int64_t b = ln.b;
  if (b >= a.batch) return;
  double* row = a.row + b * MPCQ_DIST_ROW;
  int32_t* clk = (int32_t*)(row + MPCQ_DIST_CLOCK);
  const int32_t valid = clk[0], tau_next = clk[1];

  const double y_own = a.meas[b * 12 + cc];
  const double prev_own = row[MPCQ_DIST_PREV + cc];
  const unsigned bad = robot_bits12(!isfinite(y_own) || !isfinite(prev_own), ln.shift);
  const unsigned same = robot_bits12(__double_as_longlong(y_own) == __double_as_longlong(prev_own), ln.shift);

  const bool first = first_tick(a, b);
  // (tau_next < 1 on a valid row is not the stage's own: it initialises too, and every ring
  // index below is then non-negative)
  const bool init = first || valid == 0 || tau_next < 1;

  double d[6], r[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    d[i] = 0.0;
    r[i] = NAN;
  }
  int tau = 0;
  if (!init) {
    tau = tau_next;
    const bool skip = prev_failed(a, b) || bad != 0u || (dp.skip_repeats != 0 && same == 0xfffu);
    double mass, gI[9];
    believed_robot(a, b, mass, gI);
    const double dt = a.dt;
    gather<6>(row[MPCQ_DIST_D + c6], d);
    // the previous tick's inputs: its f0 for the record, its feet and the force that acted
    const double f_last = a.f_prev[b * 12 + cc];
    const double feet_own = prev_feet_own(a.feet_prev, a.fsteps, b, cc);
    const int fj = tau - 1 - dp.f_lag;
    double f_own = f_before_first(cc);
    if (fj >= 0) f_own = row[MPCQ_DIST_RING + (fj % kSlots) * 12 + cc];  // (f_lag 0: replaced below)
    if (dp.f_lag == 0) f_own = f_last;
    if (c < 12) row[MPCQ_DIST_RING + ((tau - 1) % kSlots) * 12 + c] = f_last;  // the record
    double x[12], y[12], feet[12], f[12];
    gather<12>(prev_own, x);
    gather<12>(y_own, y);
    gather<12>(feet_own, feet);
    gather<12>(f_own, f);
    // the frame change of the tick that passed: d into this tick's frame (a yaw that is not
    // finite leaves d as it is)
    const double psi = x[5] + dt * x[11];
    if (isfinite(psi)) {
      const double cs = cos(psi), sn = sin(psi);
      const double d0 = cs * d[0] + sn * d[1], d1 = -sn * d[0] + cs * d[1];
      const double d3 = cs * d[3] + sn * d[4], d4 = -sn * d[3] + cs * d[4];
      d[0] = d0;
      d[1] = d1;
      d[3] = d3;
      d[4] = d4;
    }
    if (!skip) {  // the sample: what the state gained beyond the model's prediction, per second
      model_step(mass, gI, dt, a.gravity, x, feet, f);
      bool fin = true;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        r[i] = (y[6 + i] - x[6 + i]) / dt;
        fin = fin && isfinite(r[i]);
      }
      if (fin) {
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = d[i] + dp.alpha[i] * (r[i] - d[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      d[i] = d[i] > dp.d_max[i] ? dp.d_max[i] : d[i];
      d[i] = d[i] < -dp.d_max[i] ? -dp.d_max[i] : d[i];
    }
  }

  if (c < 12) row[MPCQ_DIST_PREV + c] = y_own;
  if (c < 6) {
    const double dc = pick<6>(d, c);
    row[MPCQ_DIST_D + c] = dc;
    a.dist[b].a[c] = dc;
    if (a.resid) a.resid[b * 6 + c] = pick<6>(r, c);
  } else if (c < 8) {
    a.dist[b].reserved[c - 6] = 0.0;
  }
  if (c == 0) {
    clk[0] = 1;
    clk[1] = tau + 1;
    clk[2] = 0;
    clk[3] = 0;
  }
}

}  // namespace

hipError_t launch_disturb(const mpcq_disturb_params& dp, const DisturbArgs& a, hipStream_t s) {
  return launch16(disturb_kernel, dp, a, s);
}

}  // namespace mpcq
