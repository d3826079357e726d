// mpcq_stage16.h — the shape the small per-robot stage kernels of a session share (the channel,
// the estimator, the disturbance stage; any later stage that chooses it): sixteen lanes per
// robot, lane c < 12 owning component c of every 12-double row, four robots per wave64, one wave
// per workgroup.  Device-only; include after `#pragma clang fp contract(off)`.
//
// A robot's rows are moved by its own consecutive lanes and touched by no others.  What a lane
// loaded is handed to the robot's other lanes by row-local shuffles (width 16), never through
// LDS.  Control flow is uniform over a robot's sixteen lanes, so every shuffle reads lanes that
// are active.  Batch tails are lanes that return at once.  No LDS, no atomics, plain vector loads
// and stores.
#pragma once
#include "mpcq_internal.h"

namespace mpcq {

constexpr int kLanes = 16;             // per robot
constexpr int kRobots = 64 / kLanes;   // per wave

// Where a lane stands.  A kernel returns at once where b >= its batch.
struct Lane16 {
  int c;           // the lane of the robot, 0..15
  int cc;          // c < 12 ? c : 11: lanes 12..15 load what lane 11 loads and store no component
  int c6;          // the same for the six-component rows
  int64_t b;       // the robot
  unsigned shift;  // of the robot's sixteen bits in a ballot of the wave
};
__device__ __forceinline__ Lane16 lane16() {
  Lane16 l;
  l.c = threadIdx.x & (kLanes - 1);
  l.cc = l.c < 12 ? l.c : 11;
  l.c6 = l.c < 6 ? l.c : 5;
  l.b = (int64_t)blockIdx.x * kRobots + (threadIdx.x >> 4);
  l.shift = threadIdx.x & 48u;
  return l;
}

// v of the robot's lanes 0..n-1 on every lane of the robot
template <int n>
__device__ __forceinline__ void gather(double v, double* out) {
#pragma unroll
  for (int i = 0; i < n; ++i) out[i] = __shfl(v, i, kLanes);
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

// pred of the robot's lanes 0..11, one bit per component, on every lane of the robot
__device__ __forceinline__ unsigned robot_bits12(bool pred, unsigned shift) {
  return (unsigned)(__ballot(pred) >> shift) & 0xfffu;
}

// the force of component cc before tick 0: the result before any solve (MPC_Wrapper.py:78)
__device__ __forceinline__ double f_before_first(int cc) { return cc % 3 == 2 ? 8.0 : 0.0; }

// component cc of the previous tick's feet [3][4]: feet_prev, or (null, a session's tick) row 0
// of fsteps
__device__ __forceinline__ double prev_feet_own(const double* feet_prev, const double* fsteps, int64_t b, int cc) {
  return feet_prev ? feet_prev[b * 12 + cc] : fsteps[b * 260 + 1 + 3 * (cc & 3) + (cc >> 2)];
}

__device__ __forceinline__ bool first_tick(const ModelInputs& m, int64_t b) {
  return m.all_first || (m.first && m.first[b] != 0);
}

// whether the previous tick failed: the caller's mask, or the statuses a session kept
__device__ __forceinline__ bool prev_failed(const ModelInputs& m, int64_t b) {
  if (m.failed) return m.failed[b] != 0;
  return m.status && solve_failed(m.status[b], m.plan_status[b]);
}

// the robot the controller believes (scalars: a struct chosen at run time would live in scratch)
__device__ __forceinline__ void believed_robot(const ModelInputs& m, int64_t b, double& mass, double* gI) {
  const mpcq_robot* rp = m.robots ? m.robots + b : nullptr;
  mass = rp ? rp->mass : m.dflt.mass;
#pragma unroll
  for (int i = 0; i < 9; ++i) gI[i] = rp ? rp->gI[i] : m.dflt.gI[i];
}

// one wave per kRobots robots; a.batch robots
template <class P, class A>
hipError_t launch16(void (*kernel)(P, A), const P& p, const A& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  if (a.batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((a.batch + kRobots - 1) / kRobots)), dim3(64), 0, s, p, a);
  return hipGetLastError();
}

}  // namespace mpcq
