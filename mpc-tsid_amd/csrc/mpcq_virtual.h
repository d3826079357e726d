// mpcq_virtual.h — the tail of a session tick, shared by the retrieve (mpcq_session.hip) and
// the rigid-body plant (mpcq_plant.hip): from the state qn[12] a robot ends the tick in,
// expressed in the tick's local frame, the world pose (MPC.py:503-510) and the virtual
// robot's next state and feet (processing.py:33-38, Interface.py:100-138).
//
// Include after `#pragma clang fp contract(off)`: rounding follows numpy, no contraction
// except np.dot(R, q_next[0:2]), which numpy evaluates as fma(R[i,0], q0, R[i,1] * q1).
#pragma once
#include <math.h>

namespace mpcq {

// qw_in [6]: the world pose before the tick; qw [6] out (may be qw_in); ns [12], lf [3][4]
// out; fs [20][13], gt [20][5]: the tick's fsteps and gait; shoulders [2][4].
__device__ __forceinline__ void advance_virtual(const double* qn, const double* qw_in, double* qw, double* ns,
                                                double* lf, const double* fs, const double* gt,
                                                const double* shoulders) {
  const double x0 = qw_in[0], y0 = qw_in[1], yaw0 = qw_in[5];
  const double c = cos(yaw0), s = sin(yaw0);
  const double d0 = fma(c, qn[0], (-s) * qn[1]);
  const double d1 = fma(s, qn[0], c * qn[1]);
  qw[0] = x0 + d0;
  qw[1] = y0 + d1;
  qw[2] = qn[2];
  qw[3] = qn[3];
  qw[4] = qn[4];
  qw[5] = yaw0 + qn[5];
  // virtual robot: new local frame under the base, yaw removed
  const double cy = cos(qn[5]), sy = sin(qn[5]);
  ns[0] = 0.0;
  ns[1] = 0.0;
  ns[2] = qn[2];
  ns[3] = qn[3];
  ns[4] = qn[4];
  ns[5] = 0.0;
  ns[6] = cy * qn[6] + sy * qn[7];
  ns[7] = -sy * qn[6] + cy * qn[7];
  ns[8] = qn[8];
  ns[9] = cy * qn[9] + sy * qn[10];
  ns[10] = -sy * qn[9] + cy * qn[10];
  ns[11] = qn[11];
  // feet: the phase that will be current after the next roll holds the
  // positions of the feet then in stance (row 0 if the phase goes on, row 1
  // if it ends); swing feet sit under their shoulders
  const int row = gt[0] > 1.0 ? 0 : 1;
  for (int q = 0; q < 4; ++q) {
    double px = fs[13 * row + 1 + 3 * q], py = fs[13 * row + 2 + 3 * q], pz = fs[13 * row + 3 + 3 * q];
    if (isnan(px) || isnan(py) || isnan(pz)) {
      px = shoulders[q] + qn[0];
      py = shoulders[4 + q] + qn[1];
      pz = 0.0;
    }
    const double dx = px - qn[0], dy = py - qn[1];
    lf[q] = cy * dx + sy * dy;
    lf[4 + q] = -sy * dx + cy * dy;
    lf[8 + q] = pz;
  }
}

}  // namespace mpcq
