// mpcq_plant.hip — the rigid-body plant of a closed-loop session on MI355X: the single
// rigid body the MPC is a discretisation of, integrated over one tick under the stance
// feet's forces and an external wrench, with constants of its own (include/mpcq.h,
// mpcq_plant_step_batch / mpcq_session_enable_plant).  No reference counterpart: the
// reference closes its loop with PyBullet and TSID.
//
// One thread per robot, blocks of 64; a robot's state stays in registers.  FP64, no
// contraction, every sum left to right in the order written here: tests/plant_model.py
// restates it in numpy and differs by the device library's sin / cos only.
#include <math.h>

#include "mpcq_internal.h"

#pragma clang fp contract(off)

#include "mpcq_model.h"
#include "mpcq_virtual.h"

namespace mpcq {
namespace {

// One tick of one robot: x [12] in/out; px, py, pz [4] the feet (NaN = swing); f [12] in,
// the effective forces out; w [6] the wrench in x's frame.
__device__ __forceinline__ void plant_step(const mpcq_plant_params& pl, const mpcq_robot& rb, double* x,
                                           const double* px, const double* py, const double* pz, double* f,
                                           const double* w) {
  double F[3] = {0.0, 0.0, 0.0}, T[3] = {0.0, 0.0, 0.0};
  for (int q = 0; q < 4; ++q) {
    double fx = f[3 * q], fy = f[3 * q + 1], fz = f[3 * q + 2];
    double rx = px[q] - x[0], ry = py[q] - x[1], rz = pz[q] - x[2];
    if (isnan(px[q]) || isnan(py[q]) || isnan(pz[q])) {  // a swing foot applies no force
      fx = fy = fz = 0.0;
      rx = ry = rz = 0.0;
    }
    if (pl.clamp) {  // comparisons, not fmin / fmax: a NaN force stays a NaN
      fz = fz < 0.0 ? 0.0 : fz;
      fz = fz > rb.fz_max ? rb.fz_max : fz;
      const double t = sqrt(fx * fx + fy * fy), lim = rb.mu * fz;
      if (t > lim) {
        const double sc = lim / t;
        fx = fx * sc;
        fy = fy * sc;
      }
    }
    f[3 * q] = fx;
    f[3 * q + 1] = fy;
    f[3 * q + 2] = fz;
    F[0] = F[0] + fx;
    F[1] = F[1] + fy;
    F[2] = F[2] + fz;
    T[0] = T[0] + (ry * fz - rz * fy);
    T[1] = T[1] + (rz * fx - rx * fz);
    T[2] = T[2] + (rx * fy - ry * fx);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    F[i] = F[i] + w[i];
    T[i] = T[i] + w[3 + i];
  }
  const double* g = rb.gI;
  if (pl.integrator == MPCQ_PLANT_MODEL) {
    const double dt = pl.dt;
    const double c = cos(x[5]), s = sin(x[5]);
    double m[9], al[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // Rz(yaw0) gI
      m[j] = c * g[j] - s * g[3 + j];
      m[3 + j] = s * g[j] + c * g[3 + j];
      m[6 + j] = g[6 + j];
    }
    solve3(m, T, al);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      x[i] = x[i] + dt * x[6 + i];
      x[3 + i] = x[3 + i] + dt * x[9 + i];
    }
    x[6] = x[6] + (dt * F[0]) / rb.mass;
    x[7] = x[7] + (dt * F[1]) / rb.mass;
    x[8] = (x[8] + (dt * F[2]) / rb.mass) - dt * pl.gravity;
#pragma unroll
    for (int i = 0; i < 3; ++i) x[9 + i] = x[9 + i] + dt * al[i];
    return;
  }
  const double h = pl.dt / (double)pl.n_sub;
  const double a[3] = {F[0] / rb.mass, F[1] / rb.mass, F[2] / rb.mass - pl.gravity};
  for (int k = 0; k < pl.n_sub; ++k) {
    const double cr = cos(x[3]), sr = sin(x[3]), cp = cos(x[4]), sp = sin(x[4]), cy = cos(x[5]), sy = sin(x[5]);
    const double R[9] = {cy * cp, (cy * sp) * sr - sy * cr, (cy * sp) * cr + sy * sr,
                         sy * cp, (sy * sp) * sr + cy * cr, (sy * sp) * cr - cy * sr,
                         -sp,     cp * sr,                  cp * cr};
    double RG[9], Iw[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        RG[3 * i + j] = (R[3 * i] * g[j] + R[3 * i + 1] * g[3 + j]) + R[3 * i + 2] * g[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        Iw[3 * i + j] = (RG[3 * i] * R[3 * j] + RG[3 * i + 1] * R[3 * j + 1]) + RG[3 * i + 2] * R[3 * j + 2];
    const double wx = x[9], wy = x[10], wz = x[11];
    double Lw[3];  // Iw w
#pragma unroll
    for (int i = 0; i < 3; ++i) Lw[i] = (Iw[3 * i] * wx + Iw[3 * i + 1] * wy) + Iw[3 * i + 2] * wz;
    const double rhs[3] = {T[0] - (wy * Lw[2] - wz * Lw[1]), T[1] - (wz * Lw[0] - wx * Lw[2]),
                           T[2] - (wx * Lw[1] - wy * Lw[0])};
    double al[3];
    solve3(Iw, rhs, al);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      x[6 + i] = x[6 + i] + h * a[i];
      x[9 + i] = x[9 + i] + h * al[i];
      x[i] = x[i] + h * x[6 + i];
    }
    const double nx = x[9], ny = x[10], nz = x[11];
    x[3] = x[3] + h * ((cy * nx + sy * ny) / cp);
    x[4] = x[4] + h * ((-sy) * nx + cy * ny);
    x[5] = x[5] + h * (((cy * sp) * nx + (sy * sp) * ny) / cp + nz);
  }
}

__global__ __launch_bounds__(64) void plant_kernel(mpcq_plant_params pl, PlantArgs a) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= a.batch) return;
  double* so = a.state_out + b * 12;
  double* fe = a.f_eff ? a.f_eff + b * 12 : nullptr;
  if (a.tail) {
    if (solve_failed(a.status[b], a.plan_status[b])) {  // the retrieve kept its pose and virtual state: so does the plant
#pragma unroll
      for (int e = 0; e < 12; ++e) {
        so[e] = NAN;
        if (fe) fe[e] = NAN;
      }
      return;
    }
  }
  double x[12], f[12], px[4], py[4], pz[4], w[6];
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    x[e] = a.state[b * 12 + e];
    f[e] = a.f[b * 12 + e];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (a.feet) {
      px[q] = a.feet[b * 12 + q];
      py[q] = a.feet[b * 12 + 4 + q];
      pz[q] = a.feet[b * 12 + 8 + q];
    } else {
      px[q] = a.fsteps[b * 260 + 1 + 3 * q];
      py[q] = a.fsteps[b * 260 + 2 + 3 * q];
      pz[q] = a.fsteps[b * 260 + 3 + 3 * q];
    }
  }
#pragma unroll
  for (int e = 0; e < 6; ++e) w[e] = a.wrench ? a.wrench[b * 6 + e] : 0.0;
  if (a.tail) {  // world frame -> the tick's local frame: Rz(-yaw), force and torque separately
    const double yaw = a.q_w_prev[b * 6 + 5];
    const double c = cos(yaw), s = sin(yaw);
    const double f0 = c * w[0] + s * w[1], f1 = -s * w[0] + c * w[1];
    const double t0 = c * w[3] + s * w[4], t1 = -s * w[3] + c * w[4];
    w[0] = f0;
    w[1] = f1;
    w[3] = t0;
    w[4] = t1;
  }
  const mpcq_robot rb = a.robots ? a.robots[b] : a.dflt;
  plant_step(pl, rb, x, px, py, pz, f, w);
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    so[e] = x[e];
    if (fe) fe[e] = f[e];
  }
  if (a.tail)
    advance_virtual(x, a.q_w_prev + b * 6, a.q_w + b * 6, a.next_state + b * 12, a.next_l_feet + b * 12,
                    a.fsteps + b * 260, a.gait + b * 100, a.shoulders);
}

}  // namespace

hipError_t launch_plant(const mpcq_plant_params& pl, const PlantArgs& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  if (a.batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(plant_kernel, dim3((unsigned)((a.batch + 63) / 64)), dim3(64), 0, s, pl, a);
  return hipGetLastError();
}

}  // namespace mpcq
