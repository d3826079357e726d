// mpcq_session.hip — the per-tick epilogue of a closed-loop session on MI355X:
// everything MPC.run and the Logger do with the QP solution after the solve,
// plus the state the next tick starts from.  One wave64 per robot.
//
//   x_robot = x[:12N] (12 x N, Fortran order) + xref[:, 1:]   MPC.py:432-449
//   q_w += R(q_w[5]) q_next[0:2], ...                          MPC.py:503-510
//   cost components (diag(x) diag(P) x, summed per state and   Logger.py:406-418
//   for the forces, numpy's pairwise summation)
//   next warm start: states shifted one stage (last zeroed),   MPC.py:403-406
//   forces rolled by one stage with wrap-around
//   virtual robot: the next tick's state / feet from x_robot[:, 0]
//   (processing.py:33-38, Interface.py:100-138)
//
// Rounding follows numpy: no contraction except np.dot(R, q_next[0:2]),
// which numpy evaluates as fma(R[i,0], q0, R[i,1] * q1).
#include <math.h>

#include "mpcq_internal.h"

#pragma clang fp contract(off)

#include "mpcq_virtual.h"

namespace mpcq {
namespace {

// numpy's pairwise_sum (umath loops: 8 partial sums below 128 elements,
// halves rounded to a multiple of 8 above), on a strided LDS array
template <int n>
__device__ __forceinline__ double pairwise(const double* v, int stride) {
  if constexpr (n < 8) {
    double s = -0.0;
    for (int i = 0; i < n; ++i) s += v[i * stride];
    return s;
  } else if constexpr (n <= 128) {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = v[j * stride];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] += v[(i + j) * stride];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += v[i * stride];
    return res;
  } else {
    constexpr int n2 = n / 2 - (n / 2) % 8;
    return pairwise<n2>(v, stride) + pairwise<n - n2>(v + n2 * stride, stride);
  }
}

template <int N>
__global__ __launch_bounds__(64) void retrieve_kernel(SessionArgs a) {
  constexpr int n = 24 * N, NP = N + 1;
  __shared__ double xs[n];
  __shared__ double cost[n];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= a.batch) return;
  const double* gx = a.x + b * n;
  const double* xr = a.xref + b * 12 * NP;
  // a robot whose planner failed this tick (where the reference raises) is treated
  // like a failed solve: it keeps its pose and virtual state and restarts cold
  const bool failed = solve_failed(a.status[b], a.plan_status[b]);
  for (int e = lane; e < n; e += 64) {
    const double v = gx[e];
    xs[e] = v;
    double w;  // the robot's own diagonal of P where a table is in force (mpcq_session_set_weights)
    if (a.weights) w = e < 12 * N ? a.weights[b].state[e % 12] : a.weights[b].force;
    else w = e < 12 * N ? a.state_weights[e % 12] : a.force_weight;
    cost[e] = (v * w) * v;  // (diag(x) @ diag(P)) @ x
  }
  __syncthreads();
  // x_robot [12][N] and the next warm start
  double* xo = a.x_robot + b * 12 * N;
  for (int e = lane; e < 12 * N; e += 64) {
    const int r = e / N, k = e % N;
    xo[e] = xs[12 * k + r] + xr[r * NP + k + 1];
  }
  double* wx = a.warm_x + b * n;
  for (int e = lane; e < n; e += 64) {
    double v;
    if (e < 12 * N) v = e < 12 * (N - 1) ? xs[e + 12] : 0.0;
    else v = xs[12 * N + (e - 12 * N + 12) % (12 * N)];
    wx[e] = failed ? 0.0 : v;  // a failed solve restarts cold (osqp would carry NaNs)
  }
  if (failed) {
    double* yy = a.y + b * 44 * N;
    for (int e = lane; e < 44 * N; e += 64) yy[e] = 0.0;
    if (lane == 0) a.rho[b] = a.rho0;
  }
  // cost components: lanes 0..11 the states, lane 12 the forces
  if (lane < 12) a.cost[b * 13 + lane] = pairwise<N>(cost + lane, 12);
  if (lane == 12) a.cost[b * 13 + 12] = pairwise<12 * N>(cost + 12 * N, 1);
  if (lane == 0 && a.plan_status[b] != 0) a.status[b] = a.plan_status[b];
  if (lane == 0 && a.first) a.first[b] = 0;  // a pending reset is served: the next tick runs as k says
  if (lane == 0 && !failed) {  // a failed robot keeps its pose and virtual state
    // q_next = x_robot[0:6, 0], v_next = x_robot[6:12, 0]
    double qn[12];
#pragma unroll
    for (int r = 0; r < 12; ++r) qn[r] = xs[r] + xr[r * NP + 1];
    double* qw = a.q_w + b * 6;
    advance_virtual(qn, qw, qw, a.next_state + b * 12, a.next_l_feet + b * 12, a.fsteps + b * 260,
                    a.gait + b * 100, a.shoulders);
  }
}

// Longest-first dispatch order from the iteration counts of the tick just solved
// (one workgroup; counting sort over buckets of 16 iterations, LDS atomics, so the
// order inside a bucket is arbitrary -- every instance's result is independent of
// the workgroup that solves it).  A robot's warm-started count predicts its next
// one (tools/tick_iters.py), and index-order dispatch puts long solves that land
// late in the launch on its critical path.
constexpr int kOrderBuckets = 256;
// first (or null): a robot with a pending reset solves cold next, the longest a robot ever
// runs: a bucket of its own above every iteration count.
__global__ __launch_bounds__(1024) void order_kernel(const int32_t* __restrict__ iters,
                                                     const int32_t* __restrict__ first, int64_t B,
                                                     int32_t* __restrict__ order) {
  __shared__ int hist[kOrderBuckets + 1];
  const int t = threadIdx.x;
  auto bucket = [&](int64_t i) {
    if (first && first[i] != 0) return kOrderBuckets;
    const int32_t it = iters[i];
    const int q = (it > 0 ? it : 0) >> 4;
    return q < kOrderBuckets - 1 ? q : kOrderBuckets - 1;
  };
  if (t <= kOrderBuckets) hist[t] = 0;
  __syncthreads();
  for (int64_t i = t; i < B; i += blockDim.x) atomicAdd(&hist[bucket(i)], 1);
  __syncthreads();
  if (t == 0) {  // exclusive offsets, the longest bucket first
    int acc = 0;
    for (int q = kOrderBuckets; q >= 0; --q) {
      const int h = hist[q];
      hist[q] = acc;
      acc += h;
    }
  }
  __syncthreads();
  for (int64_t i = t; i < B; i += blockDim.x) order[atomicAdd(&hist[bucket(i)], 1)] = (int32_t)i;
}

// mpcq_session_reset, and the state mpcq_session_create leaves (no mask, first null): one
// wave64 per robot; a robot whose mask entry is 0 is not touched.
__global__ __launch_bounds__(64) void reset_kernel(ResetArgs a) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= a.batch) return;
  if (a.mask && a.mask[b] == 0) return;
  const int N = a.N;
  auto fill = [&](double* p, int64_t per, double v) __attribute__((always_inline)) {
    double* q = p + b * per;
    for (int64_t e = lane; e < per; e += 64) q[e] = v;
  };
  {
    const double* gs = a.gait_src + b * 100;
    double* gd = a.gait + b * 100;
    for (int e = lane; e < 100; e += 64) gd[e] = gs[e];
  }
  fill(a.xref, 12 * (N + 1), 0.0);
  fill(a.fsteps, 260, NAN);
  fill(a.y, 44 * N, 0.0);
  fill(a.warm_x, 24 * N, 0.0);
  fill(a.x, 24 * N, 0.0);
  fill(a.x_robot, 12 * N, 0.0);
  fill(a.f0, 12, 0.0);
  fill(a.cost, 13, 0.0);
  if (lane < 6) {  // MPC.py:53-56
    const double d = lane == 2 ? 0.2027682 : 0.0;
    a.q_w[b * 6 + lane] = a.q_w0 ? a.q_w0[b * 6 + lane] : d;
  }
  if (lane < 12) {  // the virtual robot standing at h_ref, its feet under the shoulders
    a.state[b * 12 + lane] = lane == 2 ? a.h_ref : 0.0;
    a.l_feet[b * 12 + lane] = lane < 8 ? a.shoulders[lane] : 0.0;
  }
  if (lane == 0) {
    a.rot_flag[b] = 0;
    a.h_rot[b] = 0.20;  // FootstepPlanner.py:68
    a.rho[b] = a.rho0;
    a.status[b] = 0;
    a.iters[b] = 0;
    if (a.first) a.first[b] = 1;
  }
  if (a.swing_state) {  // all-zero state = new generators
    fill(a.swing_ref, a.swing_ref_doubles, 0.0);
    fill(a.swing_state, 4 * MPCQ_SWING_STATE, 0.0);
    fill(a.frame, 3, 0.0);
  }
  if (a.ep) {  // the running episode is discarded: no episode is counted (mpcq_monitor.hip)
    if (lane < 8) a.ep[b * 8 + lane] = lane == 4 ? INFINITY : 0.0;
    if (lane == 0) a.ep_ticks[b] = 0;
  }
  if (a.gstate && lane < 4) a.gstate[b * 4 + lane] = lane < 2 ? -1 : 0;  // no request, the table's own roll
}

}  // namespace

hipError_t launch_order(const int32_t* iters, const int32_t* first, int64_t batch, int32_t* order, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  if (batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, s, iters, first, batch, order);
  return hipGetLastError();
}

hipError_t launch_reset(const ResetArgs& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  if (a.batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(reset_kernel, dim3((unsigned)a.batch), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_retrieve(int N, const SessionArgs& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  switch (N) {
#define MPCQ_RET_CASE(NN) \
    case NN: hipLaunchKernelGGL(retrieve_kernel<NN>, dim3((unsigned)a.batch), dim3(64), 0, s, a); break;
    MPCQ_HORIZONS(MPCQ_RET_CASE)
#undef MPCQ_RET_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace mpcq
