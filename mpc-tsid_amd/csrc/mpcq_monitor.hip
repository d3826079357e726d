// mpcq_monitor.hip — the episode monitor of a closed-loop session on MI355X: after a tick,
// whether each robot's episode ended (a non-finite pose, a tilt or height threshold, a failed
// solve, a tick limit), the episode's running statistics, the batch totals and an optional
// trace row (include/mpcq.h, mpcq_monitor_step_batch / mpcq_session_enable_monitor).  The done
// bits it leaves are the device mask mpcq_session_reset takes.  No reference counterpart: the
// reference runs one robot until its script ends.
//
// One thread per robot, blocks of 64 (one wave); a robot's values stay in registers: no LDS,
// no scratch.  FP64, no contraction, every sum left to right in index order:
// tests/monitor_model.py restates it in numpy, bit for bit.  The batch totals are integers,
// counted per wave with a ballot and added by one lane with atomicAdd: their order does not
// show.
#include <math.h>

#include "mpcq_internal.h"

#pragma clang fp contract(off)

namespace mpcq {
namespace {

__global__ __launch_bounds__(64) void monitor_kernel(mpcq_monitor_params mp, MonitorArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  // a lane past the batch does no memory access but stays for the ballots below
  const bool live = b < a.batch;
  int done = 0;
  if (live) {
    double q[6], ep[8];
#pragma unroll
    for (int e = 0; e < 6; ++e) q[e] = a.q_w[b * 6 + e];
#pragma unroll
    for (int e = 0; e < 8; ++e) ep[e] = a.ep[b * 8 + e];
    const int st = a.status[b];
    const int it = a.iters[b];
    bool finite = true;
#pragma unroll
    for (int e = 0; e < 6; ++e) finite = finite && isfinite(q[e]);
    // comparisons, false on NaN: a NaN pose is NONFINITE only
    const double ar = fabs(q[3]), ap = fabs(q[4]);
    if (!finite) done |= MPCQ_DONE_NONFINITE;
    if (ar > mp.max_tilt || ap > mp.max_tilt) done |= MPCQ_DONE_TILT;
    if (q[2] < mp.min_height) done |= MPCQ_DONE_HEIGHT;
    if (!(st == MPCQ_STATUS_SOLVED || st == MPCQ_STATUS_SOLVED_INACCURATE || st == MPCQ_STATUS_MAX_ITER_REACHED))
      done |= MPCQ_DONE_SOLVER;  // the retrieve's own test
    const int ticks = a.ep_ticks[b] + 1;
    if (mp.max_ticks > 0 && ticks >= mp.max_ticks) done |= MPCQ_DONE_TIMEOUT;
    double c = a.cost[b * 13];
#pragma unroll
    for (int e = 1; e < 13; ++e) c = c + a.cost[b * 13 + e];
    double ff;
    {
      const double f = a.f0[b * 12];
      ff = f * f;
    }
#pragma unroll
    for (int e = 1; e < 12; ++e) {
      const double f = a.f0[b * 12 + e];
      ff = ff + f * f;
    }
    // the end-of-tick velocity (the next tick's frame) against this tick's command
    const double d0 = a.state[b * 12 + 6] - a.v_ref[b * 6];
    const double d1 = a.state[b * 12 + 7] - a.v_ref[b * 6 + 1];
    const double d2 = a.state[b * 12 + 11] - a.v_ref[b * 6 + 5];
    const double verr = (d0 * d0 + d1 * d1) + d2 * d2;
    if (!(done & MPCQ_DONE_SOLVER)) {  // a failed solve's cost and forces are not the controller's
      ep[0] = ep[0] + c;
      ep[1] = ep[1] + ff;
      ep[5] = ep[5] + verr;
    }
    ep[2] = ep[2] + (double)it;
    if (!(done & MPCQ_DONE_NONFINITE)) {
      const double t = ar > ap ? ar : ap;
      ep[3] = t > ep[3] ? t : ep[3];
      ep[4] = q[2] < ep[4] ? q[2] : ep[4];
    }
    ep[6] = 0.0;
    ep[7] = 0.0;
    if (a.trace) {
      double* tr = a.trace + b * MPCQ_TRACE;
#pragma unroll
      for (int e = 0; e < 6; ++e) tr[e] = q[e];
      tr[6] = (double)done;
      tr[7] = (double)st;
      tr[8] = (double)it;
      tr[9] = (double)ticks;
      tr[10] = c;
      tr[11] = ff;
#pragma unroll
      for (int e = 12; e < MPCQ_TRACE; ++e) tr[e] = 0.0;
    }
    int ticks_out = ticks;
    if (done) {
      if (a.last) {
        double* la = a.last + b * 16;
#pragma unroll
        for (int e = 0; e < 8; ++e) la[e] = ep[e];
        la[8] = (double)ticks;
        la[9] = (double)done;
#pragma unroll
        for (int e = 0; e < 6; ++e) la[10 + e] = q[e];
      }
      if (a.episodes) a.episodes[b] = a.episodes[b] + 1;
#pragma unroll
      for (int e = 0; e < 8; ++e) ep[e] = 0.0;
      ep[4] = INFINITY;
      ticks_out = 0;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) a.ep[b * 8 + e] = ep[e];
    a.ep_ticks[b] = ticks_out;
    a.done[b] = done;
  }
  if (a.totals) {  // every lane of the wave is here: those past the batch vote false
    const int n_live = __popcll(__ballot(live));
    const int n_done = __popcll(__ballot(done != 0));
    int n_bit[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) n_bit[i] = __popcll(__ballot((done >> i) & 1));
    if (threadIdx.x == 0) {  // lane 0 of a launched block is always inside the batch
      if (n_live) atomicAdd(&a.totals[0], (unsigned long long)n_live);
      if (n_done) atomicAdd(&a.totals[1], (unsigned long long)n_done);
#pragma unroll
      for (int i = 0; i < 5; ++i)
        if (n_bit[i]) atomicAdd(&a.totals[2 + i], (unsigned long long)n_bit[i]);
    }
  }
}

}  // namespace

hipError_t launch_monitor(const mpcq_monitor_params& mp, const MonitorArgs& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  if (a.batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(monitor_kernel, dim3((unsigned)((a.batch + 63) / 64)), dim3(64), 0, s, mp, a);
  return hipGetLastError();
}

}  // namespace mpcq
