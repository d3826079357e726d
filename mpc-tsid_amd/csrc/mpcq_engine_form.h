// mpcq_engine_form.h — what the engine takes from the formulation, per lane: the per-instance
// robot, weight and disturbance tables, one foot's force columns, the dynamics rows' bounds.
#pragma once
#include "mpcq_internal.h"
#include "mpcq_engine_lanes.h"

namespace mpcq {
namespace {

// ---------------------------------------------------------------------------
// Formulation pieces (restating MPC.py; oracle/mpcq_oracle.c is the CPU twin)

__device__ __forceinline__ void inv3(const double* M, double* R) {
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7],
               i = M[8];
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  const double id = 1.0 / det;
  R[0] = A * id; R[1] = -(b * i - c * h) * id; R[2] = (b * f - c * e) * id;
  R[3] = B * id; R[4] = (a * i - c * g) * id;  R[5] = -(a * f - c * d) * id;
  R[6] = C * id; R[7] = -(a * h - b * g) * id; R[8] = (a * e - b * d) * id;
}

// The per-robot constants of the workgroup's instance (ROB kernels: LaunchArgs::robots[b],
// mpcq_set_robots; the others take the launch's mpcq_params, the code they always had).  b is
// the instance (after the order[] mapping), the same for every lane, so each value is fetched
// once and comes back uniform in SGPRs (uni): fz_max at kernel entry (the bounds need it to the
// end), mass / gI / mu where the formulation starts (their 22 SGPRs are dead again before the
// solve).
struct RobotK {
  double mass, gI[9], mu;
};
__device__ __forceinline__ void load_robot(const mpcq_robot* r, RobotK& rb) {
  rb.mass = uni(r->mass);
#pragma unroll
  for (int j = 0; j < 9; ++j) rb.gI[j] = uni(r->gI[j]);
  rb.mu = uni(r->mu);
}

// The diagonal of P of the workgroup's instance (ROB solve kernels: LaunchArgs::weights[b],
// mpcq_set_weights; the others keep the launch's mpcq_params, the code they always had): the force
// weight uniform in SGPRs, the lane's own state weight (ph = its state index) as one global load.
template <bool TABLE>
__device__ __forceinline__ double weight_f(const LaunchArgs& a, int64_t b, double dflt) {
  if constexpr (TABLE) return uni(a.weights[b].force);
  else return dflt;
}
template <bool TABLE>
__device__ __forceinline__ double weight_x(const LaunchArgs& a, int64_t b, int ph, double dflt) {
  if constexpr (TABLE) return a.weights[b].state[ph];
  else return dflt;
}

// The 24 CSC values of one foot's three force columns in one stage: dt/m row,
// B rows 9..11 = dt inv(Rz(yaw) gI) [lever]x (MPC.py:339-345), swing flag S
// (MPC.py:628), friction-cone coefficients (MPC.py:136-148).
__device__ __forceinline__ void form_foot(const mpcq_params& p, double mass, const double (&gI)[9], double mu,
                                          double yaw, double l0, double l1, double l2, double swing, double* out) {
  const double cy = cos(yaw), sy = sin(yaw);
  const double R[9] = {cy, -sy, 0.0, sy, cy, 0.0, 0.0, 0.0, 1.0};
  double M[9], Mi[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int t = 0; t < 3; ++t)
      M[3 * r + t] = R[3 * r + 0] * gI[0 * 3 + t] + R[3 * r + 1] * gI[1 * 3 + t] +
                     R[3 * r + 2] * gI[2 * 3 + t];
  inv3(M, Mi);
  const double S[9] = {0.0, -l2, l1, l2, 0.0, -l0, -l1, l0, 0.0};
  const double dtm = p.dt / mass;
  int pos = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[pos++] = dtm;
#pragma unroll
    for (int r = 0; r < 3; ++r)
      out[pos++] = p.dt * (Mi[3 * r + 0] * S[0 * 3 + c] + Mi[3 * r + 1] * S[1 * 3 + c] +
                           Mi[3 * r + 2] * S[2 * 3 + c]);
    out[pos++] = swing;
    if (c < 2) {
      out[pos++] = 1.0;
      out[pos++] = -1.0;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) out[pos++] = -mu;
      out[pos++] = -1.0;
    }
  }
}

// The lane's own component of the instance's constant disturbance acceleration (ROB kernels:
// LaunchArgs::disturb[b], mpcq_set_disturbance; the others have none): dynamics row r >= 6 takes
// a[r - 6], one global load per lane like weight_x's, not through uni() -- the solve kernels sit
// at the SGPR ceiling.  Rows r < 6 load a[0] (in bounds) and do not use it.
template <bool TABLE>
__device__ __forceinline__ double disturb_a(const LaunchArgs& a, int64_t b, int r) {
  if constexpr (TABLE) return a.disturb[b].a[r >= 6 ? r - 6 : 0];
  else return 0.0;
}

// Bounds of dynamics row (k, r) (MPC.py:197-221, 366-378, 410); xr = xref staged in LDS.
// TABLE: da = the row's disturbance acceleration (disturb_a), in MPC.py's terms g[r] += dt * da
// on rows r >= 6; a da of +0.0 adds -0.0 and changes no bit.
template <int N, bool TABLE = false>
__device__ __forceinline__ double dyn_bound(const mpcq_params& p, const double* xr, int k, int r,
                                            [[maybe_unused]] double da = 0.0) {
  constexpr int NP1 = N + 1;
  double v = (r == 8) ? -(-p.gravity * p.dt) : -0.0;
  if constexpr (TABLE) {
    if (r >= 6) v = v + (-(p.dt * da));
  }
  if (k == 0) {
    double ax0 = -xr[r * NP1];
    if (r < 6) ax0 = ax0 + p.dt * (-xr[(r + 6) * NP1]);
    v = v + ax0;
  }
  double dv;
  if (k >= 1) {
    dv = -xr[r * NP1 + k];
    if (r < 6) dv = dv + (-p.dt) * xr[(r + 6) * NP1 + k];
    dv = dv + xr[r * NP1 + k + 1];
  } else {
    dv = xr[r * NP1 + 1];
  }
  return v + dv;
}

}  // namespace
}  // namespace mpcq
