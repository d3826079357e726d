// mpcq_estimator.hip — the estimate stage of a closed-loop session on MI355X, between the
// observe stage and the planner: per robot a Kalman filter on the MPC's own discrete model that
// keeps its posterior at the time the measurement was taken and predicts forward to now through
// the recorded forces and footholds (include/mpcq.h, mpcq_estimator_step_batch /
// mpcq_session_enable_estimator).  No reference counterpart: the reference reads the
// simulator's ground truth.
//
// Sixteen lanes per robot, four robots per wave64, one wave per workgroup, as the channel.  Every
// row (observation, posterior, covariance, ring slot, estimate) is moved by the robot's
// consecutive lanes, lane c < 12 owning component c: a ring slot is 192 contiguous bytes in two
// accesses of 96.  What a lane loaded is handed to the robot's other lanes by row-local shuffles
// (width 16), never through LDS; each lane then runs the robot's whole tick, the model step
// included, so the sums over feet run left to right in foot order on every lane and the bits are
// the plant's.  Control flow is uniform over a robot's sixteen lanes, so every shuffle reads
// lanes that are active.  A robot's row is touched by its own 16 lanes only; nothing that this
// launch stores is loaded again (the previous tick's inputs travel in registers), and every
// load of a word precedes the store that replaces it in program order.  Batch tails are lanes
// that return at once.  No LDS, no atomics, plain vector loads and stores.  The forecast's up to
// 8 model steps are a dependent chain: the launch's cost is latency.  FP64 without contraction:
// tests/estimator_model.py restates it in numpy and differs by the device library's sin / cos.
#include <math.h>

#include "mpcq_internal.h"

#pragma clang fp contract(off)

#include "mpcq_model.h"

namespace mpcq {
namespace {

constexpr int kLanes = 16;             // per robot
constexpr int kRobots = 64 / kLanes;   // per wave
constexpr int kSlots = MPCQ_EST_SLOTS, kSlot = 24;
static_assert(kSlots == MPCQ_ESTIMATOR_MAX_LAG + MPCQ_ESTIMATOR_MAX_F_LAG, "the ring holds lag + f_lag ticks");
static_assert(MPCQ_EST_RING + kSlots * kSlot == MPCQ_EST_ROW && MPCQ_EST_ROW % 2 == 0, "the filter's row");

// v of the robot's lanes 0..11 on every lane of the robot
__device__ __forceinline__ void gather12(double v, double* out) {
#pragma unroll
  for (int i = 0; i < 12; ++i) out[i] = __shfl(v, i, kLanes);
}

// v[c] as a chain of selects.  The empty asm keeps the compiler from folding the chain into
// v[c]: an array indexed by a lane's number would live in scratch.
template <int n>
__device__ __forceinline__ double pick(const double* v, int c) {
  double r = v[0];
#pragma unroll
  for (int i = 1; i < n; ++i) {
    r = c == i ? v[i] : r;
    asm("" : "+v"(r));
  }
  return r;
}

// Tick j's stance feet and the force acting during it (the f0 of tick j - f_lag; before tick 0
// the result before any solve, MPC_Wrapper.py:78) on every lane of the robot.  Tick `last` was
// recorded by this launch: its values come from the lane's registers, not from the ring.
__device__ __forceinline__ void tick_inputs(const double* ring, int j, int f_lag, int last, int cc, double f_last,
                                            double feet_last, double* feet, double* f) {
  const int fj = j - f_lag;
  double feet_own = ring[(j % kSlots) * kSlot + 12 + cc];
  double f_own = cc % 3 == 2 ? 8.0 : 0.0;
  if (fj >= 0) f_own = ring[(fj % kSlots) * kSlot + cc];
  if (j == last) feet_own = feet_last;
  if (fj == last) f_own = f_last;
  gather12(feet_own, feet);
  gather12(f_own, f);
}

__global__ __launch_bounds__(64) void estimate_kernel(mpcq_estimator_params ep, EstimateArgs a) {
  const int c = threadIdx.x & (kLanes - 1);
  const int64_t b = (int64_t)blockIdx.x * kRobots + (threadIdx.x >> 4);
  if (b >= a.batch) return;
  const int cc = c < 12 ? c : 11;  // lanes 12..15 load what lane 11 loads and store no component
  double* row = a.row + b * MPCQ_EST_ROW;
  const double* ring = row + MPCQ_EST_RING;
  int32_t* clk = (int32_t*)(row + MPCQ_EST_CLOCK);
  const int32_t valid = clk[0], s_old = clk[1], tau_next = clk[2];

  const double y_own = a.obs[b * 12 + cc];
  const double prev_own = row[MPCQ_EST_PREV + cc];
  // a missing frame: a non-finite component, or (skip_repeats) the previous row bit for bit
  const unsigned shift = threadIdx.x & 48u;
  const unsigned bad = (unsigned)(__ballot(!isfinite(y_own)) >> shift) & 0xfffu;
  const unsigned same = (unsigned)(__ballot(__double_as_longlong(y_own) == __double_as_longlong(prev_own)) >> shift) & 0xfffu;
  const bool missing = bad != 0u || (ep.skip_repeats != 0 && same == 0xfffu);

  const bool first = a.all_first || (a.first && a.first[b] != 0);
  bool failed = false;
  if (a.failed) {
    failed = a.failed[b] != 0;
  } else if (a.status) {  // the plant's rule
    const int st = a.status[b];
    failed = !(st == MPCQ_STATUS_SOLVED || st == MPCQ_STATUS_SOLVED_INACCURATE || st == MPCQ_STATUS_MAX_ITER_REACHED) ||
             a.plan_status[b] != 0;
  }
  const int s_want = tau_next - 1 - ep.lag;
  // (tau_next < 1 on a valid row is not the filter's own: it initialises too, and every ring
  // index below is then non-negative)
  const bool init = first || valid == 0 || failed || tau_next < 1 || s_old != (s_want > 0 ? s_want : 0);

  double y[12], x[12], xe[12], P[18];
  gather12(y_own, y);
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
    // the robot the controller believes (scalars: a struct chosen at run time would live in scratch)
    const mpcq_robot* rp = a.robots ? a.robots + b : nullptr;
    const double mass = rp ? rp->mass : a.dflt.mass;
    double gI[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) gI[i] = rp ? rp->gI[i] : a.dflt.gI[i];
    const double dt = a.dt;
    gather12(row[MPCQ_EST_POST + cc], x);
    {
      const double p_lo = row[MPCQ_EST_P + c], p_hi = row[MPCQ_EST_P + 16 + (c & 1)];
#pragma unroll
      for (int i = 0; i < 16; ++i) P[i] = __shfl(p_lo, i, kLanes);
      P[16] = __shfl(p_hi, 0, kLanes);
      P[17] = __shfl(p_hi, 1, kLanes);
    }
    // the previous tick's inputs, for the record and for the forecast
    const double f_last = a.f_prev[b * 12 + cc];
    const double feet_last = a.feet_prev ? a.feet_prev[b * 12 + cc]
                                         : a.fsteps[b * 260 + 1 + 3 * (cc & 3) + (cc >> 2)];
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
  if (a.batch <= 0) return hipSuccess;
  if (a.batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(estimate_kernel, dim3((unsigned)((a.batch + kRobots - 1) / kRobots)), dim3(64), 0, s, ep, a);
  return hipGetLastError();
}

}  // namespace mpcq
