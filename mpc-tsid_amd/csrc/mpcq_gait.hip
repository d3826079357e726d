// mpcq_gait.hip — the gait stage of a closed-loop session on MI355X (gfx950): the planner's roll
// (FootstepPlanner.py:401-425, restated in mpcq_planner.hip) with the step that enters the
// horizon taken from a desired gait cycle, per robot (include/mpcq.h, mpcq_gait_roll_batch /
// mpcq_session_enable_gait).  With no gait active it is the reference's roll, bit for bit.
//
// Thirty-two lanes per robot, two robots per wave64.  Lane r < 20 of a half holds row r of its
// robot's table in five registers (its 40 bytes lie next to its neighbours': the robot's 800
// bytes load and store as consecutive lanes' consecutive bytes).  What one lane has to know of
// another's row reaches it by a ballot masked to the half (`own`, as in planner_kernel) or a
// shuffle; the shift is every lane taking its upper neighbour's row.  No LDS, no scratch; the
// whole body is straight-line code under per-lane predicates, so every lane of the wave is
// active at every cross-lane operation -- a half whose robot is past the batch runs on defaults
// and touches no memory.
//
// The library is not in device memory: one packed word per cycle row (mpcq_internal.h
// gait_pack) and the periods, 672 bytes of kernel arguments.  Lane r reads word (active, r)
// with a per-lane index -- a vector load from the argument segment; the periods and the new
// cycle's first row are read the same way.
//
// All quantities are small integers held in doubles or int32 (the speed of the selection rule
// aside: FP64, no contraction, sqrt correctly rounded): tests/gait_model.py restates the rules
// in numpy, and every comparison against it is exact.
#include <math.h>

#include "mpcq_internal.h"

#pragma clang fp contract(off)

namespace mpcq {
namespace {

__global__ __launch_bounds__(64) void gait_kernel(mpcq_gait_params gp, GaitArgs a) {
  const int sub = (int)(threadIdx.x >> 5), ln = (int)(threadIdx.x & 31);
  const int base = 32 * sub;  // the half's lane 0 in the wave
  const int64_t b = (int64_t)blockIdx.x * 2 + sub;
  const bool live = b < a.batch;     // (the other half, if any, runs on: no early return)
  const bool row = live && ln < 20;  // this lane holds a row
  // this robot's lanes of the wave (a ballot's bits), shifted down to bit 0
  const uint64_t own = 0xffffffffull << base;
  auto half = [&](bool p) __attribute__((always_inline)) -> uint32_t {
    return (uint32_t)((__ballot(p) & own) >> base);
  };

  // ---- every global read of the robot, issued before the first cross-lane operation
  double cnt = 0.0, c[4] = {0.0, 0.0, 0.0, 0.0};
  if (row) {
    const double* g = a.gait + b * 100 + 5 * ln;
    cnt = g[0];
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = g[1 + q];
  }
  int want = -1, active = -1, phase = 0, switches = 0;
  if (live) {  // (the half's lanes read the same four words: one request)
    const int32_t* st = a.gstate + b * 4;
    want = st[0]; active = st[1]; phase = st[2]; switches = st[3];
  }
  const bool by_speed = gp.select == MPCQ_GAIT_BY_SPEED;  // uniform over the launch
  double vx = 0.0, vy = 0.0, wz = 0.0;
  if (by_speed && live) {
    const double* v = a.v_ref + b * 6;
    vx = v[0]; vy = v[1]; wz = v[5];
  }
  // the defensive reads: nothing below indexes outside the library
  const int n = gp.n_gaits;
  if (active < -1 || active >= n) active = -1;
  if (want < -1 || want >= n) want = -1;

  // ---- 1. selection (comparisons: a NaN speed moves nothing)
  if (by_speed) {
    const double s = sqrt(vx * vx + vy * vy) + gp.yaw_weight * fabs(wz);
    if (want < 0) {
      if (s == s) {
        int band = 0;
#pragma unroll
        for (int i = 0; i < MPCQ_GAIT_MAX - 1; ++i)
          if (i < n - 1 && s >= gp.thresholds[i]) ++band;
        want = band;
      }
    } else {
      bool up = false;
#pragma unroll
      for (int i = 0; i < MPCQ_GAIT_MAX - 1; ++i)  // ascending: a chain of bands in one call
        if (want == i && i < n - 1 && s > gp.thresholds[i] + gp.hysteresis) {
          want = i + 1;
          up = true;
        }
      if (!up) {
#pragma unroll
        for (int i = MPCQ_GAIT_MAX - 1; i >= 1; --i)  // descending likewise
          if (want == i && s < gp.thresholds[i - 1] - gp.hysteresis) want = i - 1;
      }
    }
  }

  // ---- 2. switch
  const uint32_t zm = half(ln < 20 && cnt == 0.0);
  const bool valid = zm != 0;  // else next(..., 0.0)[0] raises: nothing is written
  const int index = valid ? __ffs(zm) - 1 : 0;
  const int last = index == 0 ? 19 : index - 1;  // gait[index - 1]; Python wraps -1
  double c0[4];  // row 0's contacts
#pragma unroll
  for (int q = 0; q < 4; ++q) c0[q] = __shfl(c[q], base);
  bool eq0 = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) eq0 = eq0 && (c[q] == c0[q]);
  const bool row0_is_last = (half(eq0) >> last) & 1u;
  // the active cycle: lane r takes its row r, the rows' first steps by a prefix sum of the counts
  const int ga = active < 0 ? 0 : active, gw = want < 0 ? 0 : want;
  const int Pa = a.period[ga], Pw = a.period[gw];
  const int wa = ln < 20 ? a.lib[ga * 20 + ln] : 0;
  const int w0 = a.lib[gw * 20];  // the requested cycle's first row
  if (active >= 0) {
    phase %= Pa;
    if (phase < 0) phase += Pa;
  }
  const int ca = wa & 0xff;
  int incl = ca;
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const int t = __shfl_up(incl, d, 32);
    if (ln >= d) incl += t;
  }
  const int start = incl - ca;
  const bool hit = ca > 0 && phase >= start && phase < incl;  // the row step `phase` lies in
  const uint32_t hm = half(hit);
  const int w_hit = __shfl(wa, base + (hm ? __ffs(hm) - 1 : 0));
  const bool at_start = half(hit && phase == start) != 0;
  const bool boundary = active >= 0 ? at_start : (!row0_is_last || index == 1);
  const bool sw = want >= 0 && want != active && (boundary || gp.align == 0);

  // ---- 3. roll
  int bits = w_hit >> 8, P = Pa;
  if (sw) {
    active = want;
    phase = 0;
    switches = (int)((unsigned)switches + 1u);
    bits = w0 >> 8;
    P = Pw;
  }
  double nc[4];  // the step that enters the horizon
#pragma unroll
  for (int q = 0; q < 4; ++q) nc[q] = active >= 0 ? (((bits >> q) & 1) ? 1.0 : 0.0) : c0[q];
  if (active >= 0) phase = phase + 1 >= P ? 0 : phase + 1;
  bool eqn = true;
#pragma unroll
  for (int q = 0; q < 4; ++q) eqn = eqn && (c[q] == nc[q]);
  const bool same = (half(eqn) >> last) & 1u;
  if (ln == last && same) cnt += 1.0;
  if (ln == index && !same) {
    cnt = 1.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = nc[q];
  }
  // the front: the current phase goes on (count - 1), or ends: every row takes its upper
  // neighbour's (lanes 20..31 hold zeros: row 19 = 0)
  const double g00 = __shfl(cnt, base);
  const bool shift = !(g00 > 1.0);
  const double up_cnt = __shfl_down(cnt, 1, 32);
  double up_c[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) up_c[q] = __shfl_down(c[q], 1, 32);
  if (shift) {
    cnt = up_cnt;
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = up_c[q];
  } else if (ln == 0) {
    cnt -= 1.0;
  }

  // ---- the writes: the robot's whole table and its state row, nothing else
  if (row && valid) {
    double* g = a.gait + b * 100 + 5 * ln;
    g[0] = cnt;
#pragma unroll
    for (int q = 0; q < 4; ++q) g[1 + q] = c[q];
  }
  if (live && valid && ln < 4)
    a.gstate[b * 4 + ln] = ln == 0 ? want : ln == 1 ? active : ln == 2 ? phase : switches;
}

}  // namespace

hipError_t launch_gait(const mpcq_gait_params& gp, const GaitArgs& a, hipStream_t s) {
  if (a.batch <= 0) return hipSuccess;
  if (a.batch > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gait_kernel, dim3((unsigned)((a.batch + 1) / 2)), dim3(64), 0, s, gp, a);
  return hipGetLastError();
}

}  // namespace mpcq
