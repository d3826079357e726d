// mpcq_estimator.hip — the estimate stage of a closed-loop session on MI355X, between the
// observe stage and the planner: per robot a Kalman filter on the MPC's own discrete model that
// keeps its posterior at the time the measurement was taken and predicts forward to now through
// the recorded forces and footholds (include/mpcq.h, mpcq_estimator_step_batch /
// mpcq_session_enable_estimator).  No reference counterpart: the reference reads the
// simulator's ground truth.
//
// Sixteen lanes per robot (mpcq_stage16.h).  The rows are the observation, the posterior, the
// covariance, the ring slots and the estimate: a ring slot is 192 contiguous bytes in two
// accesses of 96.  Each lane runs the robot's whole tick, the model step included, so the sums
// over feet run left to right in foot order on every lane and the bits are the plant's.  Nothing
// that this launch stores is loaded again (the previous tick's inputs travel in registers), and
// every load of a word precedes the store that replaces it in program order.  The forecast's up
// to 8 model steps are a dependent chain: the launch's cost is latency.  FP64 without contraction:
// tests/estimator_model.py restates it in numpy and differs by the device library's sin / cos.
#include <math.h>

#include "mpcq_internal.h"

#pragma clang fp contract(off)

#include "mpcq_model.h"
#include "mpcq_stage16.h"

namespace mpcq {
namespace {

constexpr int kSlots = MPCQ_EST_SLOTS, kSlot = 24;
static_assert(kSlots == MPCQ_ESTIMATOR_MAX_LAG + MPCQ_ESTIMATOR_MAX_F_LAG, "the ring holds lag + f_lag ticks");
static_assert(MPCQ_EST_RING + kSlots * kSlot == MPCQ_EST_ROW && MPCQ_EST_ROW % 2 == 0, "the filter's row");

// Tick j's stance feet and the force acting during it (the f0 of tick j - f_lag; before tick 0
// the result before any solve, MPC_Wrapper.py:78) on every lane of the robot.  Tick `last` was
// recorded by this launch: its values come from the lane's registers, not from the ring.
__device__ __forceinline__ void tick_inputs(const double* ring, int j, int f_lag, int last, int cc, double f_last,
                                            double feet_last, double* feet, double* f) {
  const int fj = j - f_lag;
  double feet_own = ring[(j % kSlots) * kSlot + 12 + cc];
  double f_own = f_before_first(cc);
  if (fj >= 0) f_own = ring[(fj % kSlots) * kSlot + cc];
  if (j == last) feet_own = feet_last;
  if (fj == last) f_own = f_last;
  gather<12>(feet_own, feet);
  gather<12>(f_own, f);
}

__global__ __launch_bounds__(64) void estimate_kernel(mpcq_estimator_params ep, EstimateArgs a) {
  const Lane16 ln = lane16();
  const int c = ln.c, cc = ln.cc;
  const int64_t b = ln.b;
  if (b >= a.batch) return;
  double* row = a.row + b * MPCQ_EST_ROW;
  const double* ring = row + MPCQ_EST_RING;
  int32_t* clk = (int32_t*)(row + MPCQ_EST_CLOCK);
  const int32_t valid = clk[0], s_old = clk[1], tau_next = clk[2];

  const double y_own = a.meas[b * 12 + cc];
  const double prev_own = row[MPCQ_EST_PREV + cc];
  // a missing frame: a non-finite component, or (skip_repeats) the previous row bit for bit
  const unsigned bad = robot_bits12(!isfinite(y_own), ln.shift);
  const unsigned same = robot_bits12(__double_as_longlong(y_own) == __double_as_longlong(prev_own), ln.shift);
  const bool missing = bad != 0u || (ep.skip_repeats != 0 && same == 0xfffu);

  const bool first = first_tick(a, b);
  const bool failed = prev_failed(a, b);
  const int s_want = tau_next - 1 - ep.lag;
  // (tau_next < 1 on a valid row is not the filter's own: it initialises too, and every ring
  // index below is then non-negative)
  const bool init = first || valid == 0 || failed || tau_next < 1 || s_old != (s_want > 0 ? s_want : 0);

  double y[12], x[12], xe[12], P[18];
  gather<12>(y_own, y);
  int tau = 0, s_new = 0;
  if (init) {
#pragma unroll
    for (int i = 0; i < 12; ++i) x[i] = xe[i] = y[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      P[3 * i] = ep.p0[i];
      P[3 * i + 1] = 0.0;
      P[3 * i + 2] = ep.p0[i + 6];
    }
  } else {
    tau = tau_next;
    s_new = tau - ep.lag > 0 ? tau - ep.lag : 0;
    double mass, gI[9];
    believed_robot(a, b, mass, gI);
    const double dt = a.dt;
    gather<12>(row[MPCQ_EST_POST + cc], x);
    gather<16>(row[MPCQ_EST_P + c], P);
    gather<2>(row[MPCQ_EST_P + 16 + (c & 1)], P + 16);
    // the previous tick's inputs, for the record and for the forecast
    const double f_last = a.f_prev[b * 12 + cc];
    const double feet_last = prev_feet_own(a.feet_prev, a.fsteps, b, cc);
    double feet[12], f[12];
    if (s_new == s_old + 1) {  // the time update, its slots read before the record replaces one
      tick_inputs(ring, s_old, ep.f_lag, tau - 1, cc, f_last, feet_last, feet, f);
      model_step(mass, gI, dt, a.gravity, x, feet, f);
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double t = P[3 * i + 1] + dt * P[3 * i + 2];
        P[3 * i] = ((P[3 * i] + dt * P[3 * i + 1]) + dt * t) + ep.q[i];
        P[3 * i + 1] = t;
        P[3 * i + 2] = P[3 * i + 2] + ep.q[i + 6];
        if (i == 0 || i == 1 || i == 5) {  // the frame change pins x, y and yaw
          P[3 * i] = ep.q[i];
          P[3 * i + 1] = 0.0;
        }
      }
    }
    if (c < 12) {  // the record
      double* slot = row + MPCQ_EST_RING + ((tau - 1) % kSlots) * kSlot;
      slot[c] = f_last;
      slot[12 + c] = feet_last;
    }
    if (!missing) {
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double pp = P[3 * i], pv = P[3 * i + 1], vv = P[3 * i + 2];
        const double s00 = pp + ep.r[i], s01 = pv, s11 = vv + ep.r[i + 6];
        const double det = s00 * s11 - s01 * s01;
        const double k00 = (pp * s11 - pv * s01) / det, k01 = (pv * s00 - pp * s01) / det;
        const double k10 = (pv * s11 - vv * s01) / det, k11 = (vv * s00 - pv * s01) / det;
        const double e0 = y[i] - x[i], e1 = y[i + 6] - x[i + 6];
        x[i] = x[i] + (k00 * e0 + k01 * e1);
        x[i + 6] = x[i + 6] + (k10 * e0 + k11 * e1);
        P[3 * i] = pp - (k00 * pp + k01 * pv);
        P[3 * i + 1] = pv - (k00 * pv + k01 * vv);
        P[3 * i + 2] = vv - (k10 * pv + k11 * vv);
      }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) xe[i] = x[i];
#pragma unroll 1
    for (int j = s_new; j < tau; ++j) {  // the forecast
      tick_inputs(ring, j, ep.f_lag, tau - 1, cc, f_last, feet_last, feet, f);
      model_step(mass, gI, dt, a.gravity, xe, feet, f);
    }
  }

  if (c < 12) {
    row[MPCQ_EST_POST + c] = pick<12>(x, c);
    row[MPCQ_EST_PREV + c] = y_own;
    a.est[b * 12 + c] = pick<12>(xe, c);
  }
  row[MPCQ_EST_P + c] = pick<16>(P, c);
  if (c < 2) row[MPCQ_EST_P + 16 + c] = c == 0 ? P[16] : P[17];
  if (c == 0) {
    clk[0] = 1;
    clk[1] = s_new;
    clk[2] = tau + 1;
    clk[3] = 0;
  }
}

}  // namespace

hipError_t launch_estimate(const mpcq_estimator_params& ep, const EstimateArgs& a, hipStream_t s) {
  return launch16(estimate_kernel, ep, a, s);
}

}  // namespace mpcq
