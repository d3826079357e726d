// mpcq_scenario.hip — the scenario stage of a closed-loop session on MI355X: at the head of a
// tick, each robot's command for this tick of its episode, its push, and on a first tick the
// episode's true mass and friction (include/mpcq.h, mpcq_scenario_step_batch /
// mpcq_session_enable_scenario).  The command profile is the reference's
// Joystick.update_v_ref_predefined (Joystick.py:82-83: a ramp from rest to a target) made
// per robot, per episode and per segment; pushes and payloads have no reference counterpart.
//
// One thread per robot, blocks of 64 (one wave); a robot's values stay in registers: no LDS,
// no scratch, no atomics.  Stateless but for the robot's epoch and tick: every draw is
// Philox4x32-10 of (robot, epoch, index, stream) under the seed, at most nine calls per
// robot-tick (the constants on a first tick, two command segments, four for a push window).
// Integer arithmetic for the generator, FP64 without contraction for what is derived, every
// derived value exact or a single rounding: mpcq/scenario.py and tests/scenario_model.py
// restate it on the host, bit for bit.
#include "mpcq_internal.h"

#pragma clang fp contract(off)

#include "mpcq_philox.h"  // philox, u01, range (shared with mpcq_channel.hip)

namespace mpcq {
namespace {

// the command target of segment j: vx, vy, wyaw
__device__ inline void target(const mpcq_scenario_params& sc, uint32_t b, uint32_t epoch, uint32_t j, uint32_t k0,
                              uint32_t k1, double* t) {
  const W4 p = philox(b, epoch, 2u * j, 1u, k0, k1);
  const W4 q = philox(b, epoch, 2u * j + 1u, 1u, k0, k1);
  t[0] = range(sc.v_lo[0], sc.v_hi[0], u01(p.w0, p.w1));
  t[1] = range(sc.v_lo[1], sc.v_hi[1], u01(p.w2, p.w3));
  t[2] = range(sc.v_lo[2], sc.v_hi[2], u01(q.w0, q.w1));
}

__global__ __launch_bounds__(64) void scenario_kernel(mpcq_scenario_params sc, ScenarioArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch) return;
  const uint32_t k0 = (uint32_t)sc.seed, k1 = (uint32_t)(sc.seed >> 32);
  const bool first = a.init || a.all_first || (a.first && a.first[b] != 0);
  int32_t epoch = a.epoch[b];
  int32_t tau = a.tick[b];
  if (first && !a.init) {
    epoch = epoch + 1;
    tau = 0;
  }
  const uint32_t ub = (uint32_t)b, ue = (uint32_t)epoch;

  if (first) {  // the episode's constants
    const W4 w = philox(ub, ue, 0u, 0u, k0, k1);
    const double ms = range(sc.mass_scale_lo, sc.mass_scale_hi, u01(w.w0, w.w1));
    const double mu = range(sc.mu_lo, sc.mu_hi, u01(w.w2, w.w3));
    if (a.robots_out) {
      // field by field: a copy of the whole row would go through memory
      const mpcq_robot* src = a.base ? a.base + b : nullptr;
      mpcq_robot* o = a.robots_out + b;
      const double mass = src ? src->mass : a.dflt.mass;
      o->mass = (sc.robots & 1) ? mass * ms : mass;
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        const double gi = src ? src->gI[e] : a.dflt.gI[e];
        o->gI[e] = (sc.robots & 1) ? gi * ms : gi;
      }
      o->mu = (sc.robots & 2) ? mu : src ? src->mu : a.dflt.mu;
      o->fz_max = src ? src->fz_max : a.dflt.fz_max;
#pragma unroll
      for (int e = 0; e < 4; ++e) o->reserved[e] = src ? src->reserved[e] : a.dflt.reserved[e];
    }
    if (a.draw) {
      double* d = a.draw + b * 8;
      d[0] = ms;
      d[1] = mu;
      d[2] = (double)epoch;
#pragma unroll
      for (int e = 3; e < 8; ++e) d[e] = 0.0;
    }
  }

  double v[3] = {0.0, 0.0, 0.0};
  if (sc.commands) {
    const int j = sc.cmd_period > 0 ? tau / sc.cmd_period : 0;
    const int t = tau - j * sc.cmd_period - (j == 0 ? sc.cmd_start : 0);
    double alpha;
    if (sc.cmd_ramp > 0) {
      alpha = (double)t / (double)sc.cmd_ramp;
      alpha = alpha < 0.0 ? 0.0 : alpha > 1.0 ? 1.0 : alpha;
    } else {
      alpha = t >= 0 ? 1.0 : 0.0;
    }
    double tg[3] = {0.0, 0.0, 0.0}, pv[3] = {0.0, 0.0, 0.0};  // a first segment starts from rest
    if (alpha != 0.0) target(sc, ub, ue, (uint32_t)j, k0, k1, tg);
    if (alpha != 1.0 && j > 0) target(sc, ub, ue, (uint32_t)j - 1u, k0, k1, pv);
#pragma unroll
    for (int e = 0; e < 3; ++e)
      v[e] = alpha == 1.0 ? tg[e] : alpha == 0.0 ? pv[e] : pv[e] + (tg[e] - pv[e]) * alpha;
  }

  double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool active = false;
  if (sc.pushes && tau >= sc.push_first) {
    const int j = sc.push_period > 0 ? (tau - sc.push_first) / sc.push_period : 0;
    const uint32_t i0 = 4u * (uint32_t)j;
    const W4 h = philox(ub, ue, i0, 2u, k0, k1);
    const int jitter = (int)(((uint64_t)h.w0 * ((uint64_t)sc.push_jitter + 1)) >> 32);
    const bool occurs = (double)h.w1 * 0x1p-32 < sc.push_prob;
    const int64_t s = (int64_t)sc.push_first + (int64_t)j * sc.push_period + jitter;
    active = occurs && s <= tau && tau < s + sc.push_ticks;
    if (active) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const W4 w = philox(ub, ue, i0 + 1u + (uint32_t)c, 2u, k0, k1);
        const double x = range(sc.wrench_lo[2 * c], sc.wrench_hi[2 * c], u01(w.w0, w.w1));
        const double y = range(sc.wrench_lo[2 * c + 1], sc.wrench_hi[2 * c + 1], u01(w.w2, w.w3));
        const uint32_t flip = (uint32_t)sc.push_flip & h.w2;
        p[2 * c] = (flip >> (2 * c)) & 1u ? -x : x;
        p[2 * c + 1] = (flip >> (2 * c + 1)) & 1u ? -y : y;
      }
    }
  }

  double win[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) win[e] = a.wrench_in ? a.wrench_in[b * 6 + e] : 0.0;
  double* vo = a.v_ref + b * 6;
  vo[0] = v[0];
  vo[1] = v[1];
  vo[2] = 0.0;
  vo[3] = 0.0;
  vo[4] = 0.0;
  vo[5] = v[2];
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    a.push[b * 6 + e] = p[e];
    a.wrench_out[b * 6 + e] = active ? win[e] + p[e] : win[e];
  }
  a.epoch[b] = epoch;
  if (!a.init) a.tick[b] = tau + 1;
}

}  // namespace

hipError_t launch_scenario(const mpcq_scenario_params& sc, const ScenarioArgs& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  if (a.batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scenario_kernel, dim3((unsigned)((a.batch + 63) / 64)), dim3(64), 0, s, sc, a);
  return hipGetLastError();
}

}  // namespace mpcq
