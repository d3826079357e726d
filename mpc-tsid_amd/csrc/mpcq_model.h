// mpcq_model.h — the MPC's own discrete step of the single rigid body, shared by the plant
// (mpcq_plant.hip: solve3, under its MPCQ_PLANT_MODEL and MPCQ_PLANT_RIGID branches), the
// estimator (mpcq_estimator.hip: model_step, the filter's every propagation) and the disturbance
// stage (mpcq_disturb.hip: model_step, the prediction its sample is taken against).
//
// Include after `#pragma clang fp contract(off)`: no contraction, every sum left to right in
// the order written here (tests/plant_model.py restates it in numpy).
#pragma once
#include <math.h>

#include "../../include/mpcq.h"

namespace mpcq {

// x = inv(m) b by the adjugate (m row-major 3x3)
__device__ __forceinline__ void solve3(const double* m, const double* b, double* x) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[2] * m[7] - m[1] * m[8], c02 = m[1] * m[5] - m[2] * m[4];
  const double c10 = m[5] * m[6] - m[3] * m[8], c11 = m[0] * m[8] - m[2] * m[6], c12 = m[2] * m[3] - m[0] * m[5];
  const double c20 = m[3] * m[7] - m[4] * m[6], c21 = m[1] * m[6] - m[0] * m[7], c22 = m[0] * m[4] - m[1] * m[3];
  const double det = (m[0] * c00 + m[1] * c10) + m[2] * c20;
  x[0] = ((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det;
  x[1] = ((c10 * b[0] + c11 * b[1]) + c12 * b[2]) / det;
  x[2] = ((c20 * b[0] + c21 * b[1]) + c22 * b[2]) / det;
}

// One tick of the model the controller believes, then the state part of the tick's frame
// change: plant_step's MPCQ_PLANT_MODEL branch (mpcq_plant.hip) without clamp and without
// wrench, operation for operation, followed by advance_virtual's next state (mpcq_virtual.h):
// x, y and yaw zeroed, v and w rotated by Rz(-yaw_end).  x [12] in/out; feet [3][4] as l_feet
// (any NaN coordinate = a swing foot, which applies no force); f [12] foot-major; mass and g [9]
// (gI, row-major) of the robot the controller believes.
__device__ __forceinline__ void model_step(double mass, const double* g, double dt, double gravity, double* x,
                                           const double* feet, const double* f) {
  double F[3] = {0.0, 0.0, 0.0}, T[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double fx = f[3 * q], fy = f[3 * q + 1], fz = f[3 * q + 2];
    double rx = feet[q] - x[0], ry = feet[4 + q] - x[1], rz = feet[8 + q] - x[2];
    if (isnan(feet[q]) || isnan(feet[4 + q]) || isnan(feet[8 + q])) {
      fx = fy = fz = 0.0;
      rx = ry = rz = 0.0;
    }
    F[0] = F[0] + fx;
    F[1] = F[1] + fy;
    F[2] = F[2] + fz;
    T[0] = T[0] + (ry * fz - rz * fy);
    T[1] = T[1] + (rz * fx - rx * fz);
    T[2] = T[2] + (rx * fy - ry * fx);
  }
  const double c = cos(x[5]), s = sin(x[5]);
  double m[9], al[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {  // Rz(yaw0) gI
    m[j] = c * g[j] - s * g[3 + j];
    m[3 + j] = s * g[j] + c * g[3 + j];
    m[6 + j] = g[6 + j];
  }
  solve3(m, T, al);
  double e[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    e[i] = x[i] + dt * x[6 + i];
    e[3 + i] = x[3 + i] + dt * x[9 + i];
  }
  e[6] = x[6] + (dt * F[0]) / mass;
  e[7] = x[7] + (dt * F[1]) / mass;
  e[8] = (x[8] + (dt * F[2]) / mass) - dt * gravity;
#pragma unroll
  for (int i = 0; i < 3; ++i) e[9 + i] = x[9 + i] + dt * al[i];
  const double cy = cos(e[5]), sy = sin(e[5]);
  x[0] = 0.0;
  x[1] = 0.0;
  x[2] = e[2];
  x[3] = e[3];
  x[4] = e[4];
  x[5] = 0.0;
  x[6] = cy * e[6] + sy * e[7];
  x[7] = -sy * e[6] + cy * e[7];
  x[8] = e[8];
  x[9] = cy * e[9] + sy * e[10];
  x[10] = -sy * e[9] + cy * e[10];
  x[11] = e[11];
}

}  // namespace mpcq
