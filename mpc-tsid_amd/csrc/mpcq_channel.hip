// mpcq_channel.hip — the channel between plant and controller of a closed-loop session on
// MI355X: the observe stage in front of the planner (delay, per-episode bias, per-tick noise,
// dropped frames) and the actuate stage in front of the plant (latency, per-episode leg gain,
// per-tick force noise); include/mpcq.h, mpcq_channel_observe_batch / _actuate_batch /
// mpcq_session_enable_channel.  One tick of latency is the reference's asynchronous mode
// (MPC_Wrapper.py:57-78); the rest has no reference counterpart.
//
// Sixteen lanes per robot (mpcq_stage16.h); lanes 12..15 own the four leg gains of the draw row.
// Every row (state, observation, ring slot, force) is 96 contiguous bytes moved by consecutive
// lanes, a wave's access 384 contiguous bytes; the per-component Philox calls run in parallel,
// the robot-uniform hold draw is computed by each of the robot's lanes.  A robot's lanes run in
// lockstep: every load of a row precedes the store that replaces it in program order.  Integer
// arithmetic for the generator, FP64 without contraction for what is derived, every derived
// value exact or a single rounding: mpcq/channel.py and tests/channel_model.py restate it on the
// host, bit for bit.
#include "mpcq_internal.h"

#pragma clang fp contract(off)

#include "mpcq_philox.h"
#include "mpcq_stage16.h"

namespace mpcq {
namespace {

constexpr int kSDepth = MPCQ_CHANNEL_MAX_DELAY, kFDepth = MPCQ_CHANNEL_MAX_LATENCY;

// the centred sum of the four words at unit variance: the sum and the difference are exact
// integers below 2^35, the product the one rounding
__device__ inline double normal4(const W4& w) {
  const int64_t s = (int64_t)((uint64_t)w.w0 + w.w1 + w.w2 + w.w3) - 8589934590ll;
  return (double)s * (1.7320508075688772 * 0x1p-32);
}

// in [-1, 1), exact
__device__ inline double sym(const W4& w) { return 2.0 * u01(w.w0, w.w1) - 1.0; }

__global__ __launch_bounds__(64) void observe_kernel(mpcq_channel_params ch, ObserveArgs a) {
  const Lane16 ln = lane16();
  const int c = ln.c;
  const int64_t b = ln.b;
  if (b >= a.batch) return;
  const uint32_t k0 = (uint32_t)ch.seed, k1 = (uint32_t)(ch.seed >> 32);
  const bool first = a.all_first || (a.first && a.first[b] != 0);
  int32_t epoch = a.clock[2 * b];
  const int32_t stored = a.clock[2 * b + 1];
  const bool init = first || stored < 0;  // a first or a priming tick
  int32_t tau = stored < 0 ? ~stored : stored;
  if (first) {
    epoch = epoch + 1;
    tau = 0;
  }
  const uint32_t ub = (uint32_t)b, ue = (uint32_t)epoch, ut = (uint32_t)tau;

  double d = 0.0;  // lanes 0..11: the robot's bias of component c
  if (init) {  // the episode's draws: lanes 0..11 the biases, 12..15 the leg gains
    if (c < 12) {
      d = ch.bias[c] * sym(philox(ub, ue, 0u, 0x200u + (uint32_t)c, k0, k1));
    } else {
      d = 1.0 + ch.f_gain * sym(philox(ub, ue, 0u, 0x210u + (uint32_t)(c - 12), k0, k1));
      // not first: the force ring waits for the actuate stage's f0, marked in gain 0's sign
      if (c == 12 && !first) d = -d;
    }
    a.draw[b * 16 + c] = d;
  }
  if (c >= 12) return;

  const double truth = a.truth[b * 12 + c];
  double* ring = a.s_ring + b * (kSDepth * 12) + c;
  double delayed = truth;
  if (init) {
#pragma unroll
    for (int s = 0; s < kSDepth; ++s) ring[s * 12] = truth;
    if (first) {  // the result before any solve (MPC_Wrapper.py:78)
      double* fr = a.f_ring + b * (kFDepth * 12) + c;
      const double f = f_before_first(c);
#pragma unroll
      for (int s = 0; s < kFDepth; ++s) fr[s * 12] = f;
    }
  } else if (ch.delay > 0) {
    const int slot = tau % ch.delay;
    delayed = ring[slot * 12];
    ring[slot * 12] = truth;
  }

  double o = delayed;
  if (ch.bias[c] != 0.0) o = o + (init ? d : a.draw[b * 16 + c]);
  if (ch.sigma[c] != 0.0) o = o + ch.sigma[c] * normal4(philox(ub, ue, ut, 0x100u + (uint32_t)c, k0, k1));
  if (ch.hold_prob > 0.0 && !init) {
    const W4 h = philox(ub, ue, ut, 0x110u, k0, k1);
    if ((double)h.w1 * 0x1p-32 < ch.hold_prob) o = a.obs[b * 12 + c];  // a dropped frame
  }
  a.obs[b * 12 + c] = o;
  if (c == 0) {
    a.clock[2 * b] = epoch;
    a.clock[2 * b + 1] = tau + 1;
  }
}

__global__ __launch_bounds__(64) void actuate_kernel(mpcq_channel_params ch, ActuateArgs a) {
  const Lane16 ln = lane16();
  const int c = ln.c;
  const int64_t b = ln.b;
  if (b >= a.batch || c >= 12) return;
  const uint32_t k0 = (uint32_t)ch.seed, k1 = (uint32_t)(ch.seed >> 32);
  const int32_t epoch = a.clock[2 * b];
  const int32_t stored = a.clock[2 * b + 1];
  const int32_t tau = stored > 0 ? stored - 1 : 0;  // (no observe stage has run: 0)
  const int q = c / 3, ax = c - 3 * q;
  const double g0 = a.draw[b * 16 + 12];
  const bool pending = g0 < 0.0;
  const double gain = q == 0 ? (pending ? -g0 : g0) : a.draw[b * 16 + 12 + q];

  const double f0 = a.f0[b * 12 + c];
  double* fr = a.f_ring + b * (kFDepth * 12) + c;
  double cmd = f0;
  if (pending) {  // the ring's first fill after a priming tick: this tick's own result
#pragma unroll
    for (int s = 0; s < kFDepth; ++s) fr[s * 12] = f0;
    if (c == 0) a.draw[b * 16 + 12] = -g0;
  } else if (ch.latency > 0) {
    const int slot = tau % ch.latency;
    cmd = fr[slot * 12];
    fr[slot * 12] = f0;
  }

  double v = cmd;
  if (ch.f_gain != 0.0) v = cmd * gain;
  if (ch.f_sigma[ax] != 0.0)
    v = v + ch.f_sigma[ax] * normal4(philox((uint32_t)b, (uint32_t)epoch, (uint32_t)tau, 0x120u + (uint32_t)c, k0, k1));
  a.f_cmd[b * 12 + c] = v;
}

__global__ __launch_bounds__(64) void arm_kernel(int32_t* clock, int64_t batch) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  const int32_t t = clock[2 * b + 1];
  if (t >= 0) clock[2 * b + 1] = ~t;
}

}  // namespace

hipError_t launch_observe(const mpcq_channel_params& ch, const ObserveArgs& a, hipStream_t s) {
  return launch16(observe_kernel, ch, a, s);
}

hipError_t launch_actuate(const mpcq_channel_params& ch, const ActuateArgs& a, hipStream_t s) {
  return launch16(actuate_kernel, ch, a, s);
}

hipError_t launch_channel_arm(int32_t* clock, int64_t batch, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  if (batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(arm_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, clock, batch);
  return hipGetLastError();
}

}  // namespace mpcq
