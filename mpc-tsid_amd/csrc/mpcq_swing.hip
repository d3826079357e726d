// mpcq_swing.hip — batched swing-foot trajectories for MI355X (gfx950): the consumer
// of the planner's (gait, fsteps) between two MPC ticks.
//
//   update_footsteps    TSID_Debug_controller_four_legs_fb_vel.py:471-487   the target of
//                                                      every foot, in the world frame
//   update_feet_tasks   TSID_Debug_controller_four_legs_fb_vel.py:247-327   t_swing, t0 and
//                                                      the generator's arguments
//   get_next_foot       FootTrajectoryGenerator.py:222-380   5th-order x / y, 6th-order z
//
// One lane per (robot, foot): 16 robots per wave64, one wave per workgroup.  The substep
// loop is serial per lane (the goal of one substep is the start of the next) with the
// generator's state in registers.  gait, fsteps, the state and the output rows pass
// through LDS (one 21 KB region reused by each in turn) so that every HBM row is moved by
// consecutive lanes; the gait timing (the
// first stance row, the cumulative durations, t_swing) and the target are derived once
// per foot per launch.
//
// Rounding: no contraction.  The scalar chain that decides branches (t_swing, the
// remaining iterations, t0, t0 == 0, t1 - t0 > t_lock) follows the reference's operation
// order exactly; the polynomials use products where the reference calls pow() and one
// reciprocal of the coefficients' common denominator, and are held to a tolerance
// (DESIGN.md section 2).
#include <math.h>

#include "mpcq_internal.h"

#pragma clang fp contract(off)

namespace mpcq {
namespace {

constexpr int kRobots = 16;   // per wave64
constexpr int kChunk = 4;     // substeps of output rows gathered in LDS per flush
constexpr int kFsRows = 5;    // fsteps rows staged at a time
constexpr int kSt = MPCQ_SWING_STATE;

// One wave64 per workgroup: an LDS hand-off between its lanes needs no hardware barrier
// (mpcq_planner.hip lane_sync).
__device__ __forceinline__ void lane_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the d5..d0 of one axis (FootTrajectoryGenerator.py:252-272), the powers of t0 (a) and t1 (b)
struct Pw {
  double a, a2, a3, a4, a5, b, b2, b3, b4, b5, rden;  // rden = 1 / den: one division per call
};

__device__ __forceinline__ void axis_coeffs(const Pw& w, double p, double v, double acc, double* d) {
  const double a = w.a, a2 = w.a2, a3 = w.a3, a4 = w.a4, b = w.b, b2 = w.b2, b3 = w.b3, b4 = w.b4,
               b5 = w.b5, rden = w.rden;
  d[0] = (acc * a2 - 2 * acc * a * b - 6 * v * a + acc * b2 + 6 * v * b + 12 * p) * rden;
  d[1] = (-30 * a * p - 30 * b * p - 2 * a3 * acc - 3 * b3 * acc + 14 * a2 * v - 16 * b2 * v + 2 * a * b * v +
          4 * a * b2 * acc + a2 * b * acc) * rden;
  d[2] = (a4 * acc + 3 * b4 * acc - 8 * a3 * v + 12 * b3 * v + 20 * a2 * p + 20 * b2 * p + 80 * a * b * p +
          4 * a3 * b * acc + 28 * a * b2 * v - 32 * a2 * b * v - 8 * a2 * b2 * acc) * rden;
  d[3] = -(b5 * acc + 4 * a * b4 * acc + 3 * a4 * b * acc + 36 * a * b3 * v - 24 * a3 * b * v + 60 * a * b2 * p +
           60 * a2 * b * p - 8 * a2 * b3 * acc - 12 * a2 * b2 * v) * rden;
  d[4] = -(2 * b5 * v - 2 * a * b5 * acc - 10 * a * b4 * v + a2 * b4 * acc + 4 * a3 * b3 * acc -
           3 * a4 * b2 * acc - 16 * a2 * b3 * v + 24 * a3 * b2 * v - 60 * a2 * b2 * p) * rden;
  d[5] = (-acc * a4 * b3 + 2 * acc * a3 * b4 + 8 * v * a3 * b3 - acc * a2 * b5 - 10 * v * a2 * b4 -
          20 * p * a2 * b3 + 2 * v * a * b5 + 10 * p * a * b4 - 2 * p * b5) * rden;
}

// position, velocity, acceleration of one axis at ev: x1 * c(ev) + d(ev), c and d stored 5..0
__device__ __forceinline__ void axis_eval(const double* c, const double* d, double x1, double e, double e2,
                                          double e3, double e4, double e5, double* o) {
  o[0] = x1 * (c[5] + c[4] * e + c[3] * e2 + c[2] * e3 + c[1] * e4 + c[0] * e5) + d[5] + d[4] * e + d[3] * e2 +
         d[2] * e3 + d[1] * e4 + d[0] * e5;
  o[1] = x1 * (c[4] + 2 * c[3] * e + 3 * c[2] * e2 + 4 * c[1] * e3 + 5 * c[0] * e4) + d[4] + 2 * d[3] * e +
         3 * d[2] * e2 + 4 * d[1] * e3 + 5 * d[0] * e4;
  o[2] = x1 * (2 * c[3] + 3 * 2 * c[2] * e + 4 * 3 * c[1] * e2 + 5 * 4 * c[0] * e3) + 2 * d[3] + 3 * 2 * d[2] * e +
         4 * 3 * d[1] * e2 + 5 * 4 * d[0] * e3;
}

// Az3, Az4, Az5, Az6 (FootTrajectoryGenerator.py:321-324): they depend on t1 and h alone
__device__ __forceinline__ void z_coeffs(double t1, double h, double (&az)[4]) {
  const double hb = t1 / 2, hb3 = hb * hb * hb, rb = t1 - t1 / 2, rb3 = rb * rb * rb;
  const double zd = hb3 * rb3;
  az[0] = ((t1 * t1 * t1) * h) / zd;
  az[1] = -(3 * (t1 * t1) * h) / zd;
  az[2] = (3 * t1 * h) / zd;
  az[3] = -h / zd;
}

// Foot_trajectory_generator.get_next_foot on the state st (slots 0..25 and 34):
// o = x0, dx0, ddx0, y0, dy0, ddy0, z0, dz0, ddz0, gx1, gy1
__device__ __forceinline__ void next_foot(double (&st)[kSt], double x0, double dx0, double ddx0, double y0,
                                          double dy0, double ddy0, double x1, double y1, double t0, double t1,
                                          double dt, const double (&az)[4], double t_lock, double (&o)[11]) {
  const bool adaptive = (t1 - t0) > t_lock;
  if (adaptive) {
    Pw w;
    w.a = t0; w.a2 = t0 * t0; w.a3 = w.a2 * t0; w.a4 = w.a2 * w.a2; w.a5 = w.a4 * t0;
    w.b = t1; w.b2 = t1 * t1; w.b3 = w.b2 * t1; w.b4 = w.b2 * w.b2; w.b5 = w.b4 * t1;
    const double dif = t0 - t1;
    w.rden = 1.0 / (2 * (dif * dif) * (w.a3 - 3 * w.a2 * w.b + 3 * w.a * w.b2 - w.b3));
    const double c5 = (-12) * w.rden;
    const double c4 = (30 * w.a + 30 * w.b) * w.rden;
    const double c3 = (-20 * w.a2 - 20 * w.b2 - 80 * w.a * w.b) * w.rden;
    const double c2 = -(-60 * w.a * w.b2 - 60 * w.a2 * w.b) * w.rden;
    const double c1 = -(60 * w.a2 * w.b2) * w.rden;
    const double c0 = (20 * w.a3 * w.b2 + 2 * w.a5 - 10 * w.a4 * w.b) * w.rden;
    st[0] = c5; st[1] = c4; st[2] = c3; st[3] = c2; st[4] = c1; st[5] = c0;
    st[12] = c5; st[13] = c4; st[14] = c3; st[15] = c2; st[16] = c1; st[17] = c0;
    axis_coeffs(w, x0, dx0, ddx0, &st[6]);
    axis_coeffs(w, y0, dy0, ddy0, &st[18]);
    st[24] = x1;
    st[25] = y1;
  }
  st[34] = adaptive ? 1.0 : 0.0;
  const double Az3 = az[0], Az4 = az[1], Az5 = az[2], Az6 = az[3];  // z (deterministic)
  const double e = t0 + dt, e2 = e * e, e3 = e2 * e, e4 = e2 * e2, e5 = e4 * e, e6 = e3 * e3;
  axis_eval(&st[0], &st[6], st[24], e, e2, e3, e4, e5, &o[0]);
  axis_eval(&st[12], &st[18], st[25], e, e2, e3, e4, e5, &o[3]);
  o[6] = Az3 * e3 + Az4 * e4 + Az5 * e5 + Az6 * e6;
  o[7] = 3 * Az3 * e2 + 4 * Az4 * e3 + 5 * Az5 * e4 + 6 * Az6 * e5;
  o[8] = 2 * 3 * Az3 * e + 3 * 4 * Az4 * e2 + 4 * 5 * Az5 * e3 + 5 * 6 * Az6 * e4;
  o[9] = st[24];
  o[10] = st[25];
}

// rows of `per` doubles of the wave's `nb` robots, contiguous in HBM: consecutive lanes
// move consecutive doubles
__device__ __forceinline__ void rows_in(double* dst, const double* src, int n, int lane) {
  for (int e = lane; e < n; e += 64) dst[e] = src[e];
}

__global__ __launch_bounds__(64) void swing_step_kernel(mpcq_swing_params sp, int64_t batch,
                                                        const double* __restrict__ in, double* state,
                                                        double* __restrict__ out) {
  __shared__ double s_in[kRobots * 40];
  __shared__ double s_st[kRobots * 4 * kSt];
  __shared__ double s_out[kRobots * 44];
  __shared__ int s_skip[64];
  const int lane = threadIdx.x, r = lane >> 2;
  const int64_t b0 = (int64_t)blockIdx.x * kRobots;
  const int nb = batch - b0 < kRobots ? (int)(batch - b0) : kRobots;
  rows_in(s_in, in + b0 * 40, nb * 40, lane);
  rows_in(s_st, state + b0 * 4 * kSt, nb * 4 * kSt, lane);
  lane_sync();
  const bool live = r < nb;
  bool skip = true;
  if (live) {
    const double* a = s_in + lane * 10;
    skip = isnan(a[8]);
    double o[11];
    if (!skip) {
      double st[kSt];
#pragma unroll
      for (int j = 0; j < kSt; ++j) st[j] = s_st[lane * kSt + j];
      double az[4];
      z_coeffs(a[9], sp.max_height, az);
      next_foot(st, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], sp.dt, az, sp.t_lock, o);
#pragma unroll
      for (int j = 0; j < kSt; ++j) s_st[lane * kSt + j] = st[j];
    } else {
#pragma unroll
      for (int j = 0; j < 11; ++j) o[j] = NAN;
    }
#pragma unroll
    for (int j = 0; j < 11; ++j) s_out[lane * 11 + j] = o[j];
  }
  s_skip[lane] = skip;
  lane_sync();
  for (int e = lane; e < nb * 44; e += 64) out[b0 * 44 + e] = s_out[e];
  for (int e = lane; e < nb * 4 * kSt; e += 64)
    if (!s_skip[e / kSt]) state[b0 * 4 * kSt + e] = s_st[e];  // a skipped foot keeps its state
}

// LDS of swing_kernel, one region used three ways so that several waves fit a CU:
//   phase 1   the wave's gait tables and kFsRows rows of its fsteps tables at a time
//   phase 2   the states (in, and out again at the end), in between a chunk of output rows
//             and its t0 (the states live in registers meanwhile)
constexpr int kGaitOff = 0, kFsOff = kRobots * 100, kFsPer = kFsRows * 13;
constexpr int kStOff = 0, kRefOff = 0, kT0Off = kRobots * kChunk * 36;
constexpr int kLds = kFsOff + kRobots * kFsPer;
static_assert(20 % kFsRows == 0, "whole passes over the fsteps rows");
static_assert(kLds >= kRobots * 4 * kSt && kLds >= kT0Off + kRobots * kChunk * 4, "phase 2 fits the region");

__global__ __launch_bounds__(64) void swing_kernel(mpcq_swing_params sp, SwingArgs a) {
  __shared__ double sh[kLds];
  __shared__ double s_frame[kRobots * 3];
  __shared__ double s_feet0[kRobots * 24];
  __shared__ int s_bad[kRobots];
  const int lane = threadIdx.x, r = lane >> 2, f = lane & 3;
  const int64_t b0 = (int64_t)blockIdx.x * kRobots;
  const int nb = a.batch - b0 < kRobots ? (int)(a.batch - b0) : kRobots;
  const bool live = r < nb;
  const int n_sub = a.n_sub;

  // ---- phase 1: the tables
  rows_in(sh + kGaitOff, a.gait + b0 * 100, nb * 100, lane);
  rows_in(s_frame, a.frame + b0 * 3, nb * 3, lane);
  if (a.feet0) rows_in(s_feet0, a.feet0 + b0 * 24, nb * 24, lane);
  if (lane < kRobots) s_bad[lane] = 0;
  lane_sync();

  bool swing = false;
  double cs = 0.0, t_swing = 0.0;     // cumulative durations up to the next stance row, t_swing
  double tx = 0.0, ty = 0.0;          // the target in the world frame
  double sx = NAN, sy = NAN;          // a stance foot's world position (row 0 of fsteps)
  if (live) {
    const double* g = sh + kGaitOff + r * 100;
    swing = g[1 + f] == 0.0;
    if (swing) {
      // a column without any stance row: the reference's forward walk runs off the table
      bool any = false;
      for (int i = 0; i < 20; ++i) any = any || !(g[5 * i + 1 + f] == 0.0);
      if (!any) {
        s_bad[r] = 1;
      } else {
        // TSID:267-268: the first row with a 1, none: index -1 (the rows before the last)
        int index = -1;
        for (int i = 0; i < 20; ++i)
          if (g[5 * i + 1 + f] == 1.0) { index = i; break; }
        const int end = index < 0 ? 19 : index;
        cs = g[0];
        for (int i = 1; i < end; ++i) cs += g[5 * i];  // np.cumsum: left to right
        // TSID:271-280
        t_swing = g[0];
        for (int i = 1; i < 20 && g[5 * i + 1 + f] == 0.0; ++i) t_swing += g[5 * i];
        for (int i = 19; i >= 0 && g[5 * i + 1 + f] == 0.0; --i) t_swing += g[5 * i];  // gait[-1], [-2], ...
        t_swing *= sp.dt * (double)sp.k_mpc;
      }
    }
  }
  // TSID:483-485: the first row of the foot's x column that is neither 0 nor NaN, none: row
  // -1 = row 19; the table passes through LDS kFsRows rows at a time
  double px = 0.0, py = 0.0, qx = NAN, qy = NAN;  // the target and row 0, local frame
  bool found = false;
  for (int p = 0; p < 20 / kFsRows; ++p) {
    for (int e = lane; e < nb * kFsPer; e += 64) {
      const int rr = e / kFsPer, w = e % kFsPer;
      sh[kFsOff + e] = a.fsteps[(b0 + rr) * 260 + p * kFsPer + w];
    }
    lane_sync();
    if (live) {
      const double* fs = sh + kFsOff + r * kFsPer;
      if (p == 0) { qx = fs[1 + 3 * f]; qy = fs[2 + 3 * f]; }
      for (int i = 0; i < kFsRows && !found; ++i) {
        const double v = fs[13 * i + 1 + 3 * f];
        if (!(v == 0.0) && !isnan(v)) { found = true; px = v; py = fs[13 * i + 2 + 3 * f]; }
      }
      if (p == 20 / kFsRows - 1 && !found) {
        px = fs[13 * (kFsRows - 1) + 1 + 3 * f];
        py = fs[13 * (kFsRows - 1) + 2 + 3 * f];
      }
    }
    lane_sync();
  }
  if (live) {
    const double yaw = s_frame[3 * r + 2];
    const double c = cos(yaw), s = sin(yaw);
    tx = (c * px - s * py) + s_frame[3 * r];
    ty = (s * px + c * py) + s_frame[3 * r + 1];
    if (!isnan(qx) && !isnan(qy)) {
      sx = (c * qx - s * qy) + s_frame[3 * r];
      sy = (s * qx + c * qy) + s_frame[3 * r + 1];
    }
  }
  lane_sync();

  // ---- phase 2: the states over the tables, then into registers
  rows_in(sh + kStOff, a.state + b0 * 4 * kSt, nb * 4 * kSt, lane);
  lane_sync();
  double st[kSt];
#pragma unroll
  for (int j = 0; j < kSt; ++j) st[j] = live ? sh[kStOff + lane * kSt + j] : 0.0;
  const bool bad = live && s_bad[r];
  lane_sync();  // the output rows go over the states
  double az[4];  // t1 = t_swing for the whole call
  z_coeffs(t_swing, sp.max_height, az);
  double f0[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) f0[j] = (a.feet0 && live) ? s_feet0[lane * 6 + j] : 0.0;

  for (int k = 0; k < n_sub; ++k) {
    const int slot = k % kChunk;
    double o[9];
    double t0 = NAN;
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] = NAN;
    if (live && !bad) {
      if (swing) {
        const double remaining = cs * (double)sp.k_mpc - (double)(a.k_sub0 + k);
        t0 = rint((t_swing - remaining * sp.dt) * 1000.0) / 1000.0;  // np.round(., decimals=3)
        double g[11];
        if (t0 == 0.0) {  // lift-off: the measured foot, or where the foot last stood
          if (a.feet0) next_foot(st, f0[0], f0[1], f0[2], f0[3], f0[4], f0[5], tx, ty, t0, t_swing, sp.dt, az, sp.t_lock, g);
          else next_foot(st, st[35], 0.0, 0.0, st[36], 0.0, 0.0, tx, ty, t0, t_swing, sp.dt, az, sp.t_lock, g);
        } else {
          next_foot(st, st[26], st[27], st[28], st[29], st[30], st[31], tx, ty, t0, t_swing, sp.dt, az, sp.t_lock, g);
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) st[26 + j] = g[j];
        st[32] = t_swing;
        st[33] = t0;
        o[0] = g[0]; o[1] = g[3]; o[2] = g[6] + sp.feet_z;
        o[3] = g[1]; o[4] = g[4]; o[5] = g[7];
        o[6] = g[2]; o[7] = g[5]; o[8] = g[8];
        st[35] = g[0];
        st[36] = g[3];
      } else if (!isnan(sx)) {
        st[35] = sx;
        st[36] = sy;
      }
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < 9; ++j) sh[kRefOff + (r * kChunk + slot) * 36 + f * 9 + j] = o[j];
      sh[kT0Off + (r * kChunk + slot) * 4 + f] = t0;
    }
    if (slot == kChunk - 1 || k == n_sub - 1) {  // flush the chunk: cnt substeps per robot
      lane_sync();
      const int cnt = slot + 1, k0 = k - slot;
      for (int e = lane; e < nb * cnt * 36; e += 64) {
        const int rr = e / (cnt * 36), w = e % (cnt * 36);
        a.ref[((b0 + rr) * n_sub + k0) * 36 + w] = sh[kRefOff + rr * kChunk * 36 + w];
      }
      if (a.t0_out)
        for (int e = lane; e < nb * cnt * 4; e += 64) {
          const int rr = e / (cnt * 4), w = e % (cnt * 4);
          a.t0_out[((b0 + rr) * n_sub + k0) * 4 + w] = sh[kT0Off + rr * kChunk * 4 + w];
        }
      lane_sync();
    }
  }

  if (live) {
#pragma unroll
    for (int j = 0; j < kSt; ++j) sh[kStOff + lane * kSt + j] = st[j];
  }
  lane_sync();
  for (int e = lane; e < nb * 4 * kSt; e += 64)
    if (!s_bad[e / (4 * kSt)]) a.state[b0 * 4 * kSt + e] = sh[kStOff + e];  // a bad robot keeps its state
  if (a.status && lane < nb) a.status[b0 + lane] = s_bad[lane] ? MPCQ_STATUS_BAD_GAIT : 0;
}

}  // namespace

hipError_t launch_swing(const mpcq_swing_params& sp, const SwingArgs& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  const int64_t blocks = (a.batch + kRobots - 1) / kRobots;
  hipLaunchKernelGGL(swing_kernel, dim3((unsigned)blocks), dim3(64), 0, s, sp, a);
  return hipGetLastError();
}

hipError_t launch_swing_step(const mpcq_swing_params& sp, int64_t batch, const double* in, double* state,
                             double* out, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  const int64_t blocks = (batch + kRobots - 1) / kRobots;
  hipLaunchKernelGGL(swing_step_kernel, dim3((unsigned)blocks), dim3(64), 0, s, sp, batch, in, state, out);
  return hipGetLastError();
}

}  // namespace mpcq
