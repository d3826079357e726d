// mpcq_session_api.cpp — the mpcq_session_* entry points of include/mpcq.h: closed-loop
// sessions, per-robot state resident in HBM.
//
// A session's device arrays come in groups (alloc_group): the main one made by
// mpcq_session_create, and one each for swing, plant, monitor, scenario, channel, estimator and gait, made when
// they are first enabled.  A tick (session_tick) is a list of stages, each filling the argument struct of
// its launch from the groups' arrays.  All numerics run in the HIP kernels.
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "mpcq_host.h"

using namespace mpcq;

namespace {

// Private arrays, behind the named ones of their group: the warm start, the planner's
// status, the engine's info, the staging of host inputs (tick: state, l_feet, v_ref,
// reduced; reset: mask in IN_REDUCED, q_w0 in IN_VREF, gait0 in IN_GAIT), the gait table
// every robot was created with; the copy of q_w a tick with the plant takes before its
// retrieve.
enum { SP_WARM_X = MPCQ_SV_COUNT, SP_PLAN_STATUS, SP_INFO, SP_IN_STATE, SP_IN_LFEET, SP_IN_VREF, SP_IN_REDUCED,
       SP_GAIT_INIT, SP_IN_GAIT, SP_COUNT };
enum { PP_QW_PREV = MPCQ_PV_COUNT, PP_COUNT };

// The arrays of one kind of id: MPCQ_SV_* (the swing slots are null until
// mpcq_session_enable_swing), MPCQ_PV_*, MPCQ_MV_*, MPCQ_CV_*, MPCQ_HV_*, MPCQ_EV_*, MPCQ_GV_*, MPCQ_DV_*.
struct Group {
  const char *kind, *enable;  // "<kind> array %d needs mpcq_session_enable_<enable>"
  int named;                  // the ids the _read / _write / _device_ptr entry points reach
  void* mem = nullptr;
  void* ptr[SP_COUNT] = {};
  size_t bytes[SP_COUNT] = {};
  double* d(int w) const { return (double*)ptr[w]; }
  int32_t* i(int w) const { return (int32_t*)ptr[w]; }
};

}  // namespace

struct mpcq_session {
  mpcq_ctx* ctx = nullptr;
  int64_t B = 0;
  mpcq_planner_params pp{};
  Group sv{"session", "swing", MPCQ_SV_COUNT};
  Group pv{"plant", "plant", MPCQ_PV_COUNT};      // made by the first enable_plant / set_wrench
  Group mv{"monitor", "monitor", MPCQ_MV_COUNT};  // made by the first enable_monitor
  Group cv{"scenario", "scenario", MPCQ_CV_COUNT};  // made by the first enable_scenario
  Group hv{"channel", "channel", MPCQ_HV_COUNT};    // made by the first enable_channel
  Group ev{"estimator", "estimator", MPCQ_EV_COUNT};  // made by the first enable_estimator
  Group gv{"gait", "gait", MPCQ_GV_COUNT};            // made by the first enable_gait
  Group dv{"disturb", "disturb", MPCQ_DV_COUNT};      // made by the first enable_disturb
  void* swing_mem = nullptr;                      // MPCQ_SV_SWING_REF, _SWING_STATE, _FRAME
  bool have_order = false;  // MPCQ_SV_ORDER holds the next solve's order (longest previous first)
  bool use_order = true;    // MPCQ_DISPATCH_ORDER=0 turns it off (A/B timing only; results are identical)
  bool resets = false;      // mpcq_session_reset was called: from then on the ticks consult MPCQ_SV_FIRST
  bool swing = false, plant = false, monitor = false, scenario = false, channel = false, estimator = false;
  bool gait = false;
  bool disturb_on = false;  // the disturbance stage runs (mpcq_session_enable_disturb)
  mpcq_disturb_params dp{};
  mpcq_gait_params gp{};
  mpcq::GaitArgs gait_lib{};  // the library in force, packed (period, lib; the launch fills the rest)
  mpcq_swing_params sp{};
  mpcq_plant_params pl{};
  mpcq_monitor_params mp{};
  mpcq_scenario_params sc{};
  mpcq_channel_params ch{};  // (delay and latency: what the rings in hv were primed under)
  mpcq_estimator_params ep{};
  RobotTable robots;        // mpcq_session_set_robots (the session's own, not the context's)
  RobotTable plant_robots;  // mpcq_session_set_plant_robots
  WeightsTable weights;     // mpcq_session_set_weights (the controller's tuning: no snapshot holds it)
  DisturbTable disturb;     // mpcq_session_set_disturbance (the controller's model: no snapshot holds it)
  FillTables fill;          // the table a ROB launch reads in place of the one that is not set
  mpcq_snapshot* fork_snap = nullptr;  // mpcq_session_fork's own, made on first use
};

namespace {

// Bytes of an array of the main group (layouts: include/mpcq.h).
size_t sv_bytes(int what, int64_t B, int N) {
  const size_t b = (size_t)B;
  switch (what) {
    case MPCQ_SV_F0: case MPCQ_SV_STATE: case MPCQ_SV_L_FEET: case SP_IN_STATE: case SP_IN_LFEET: return b * 12 * 8;
    case MPCQ_SV_X: case SP_WARM_X: return b * 24 * N * 8;
    case MPCQ_SV_X_ROBOT: return b * 12 * N * 8;
    case MPCQ_SV_Q_W: case SP_IN_VREF: return b * 6 * 8;
    case MPCQ_SV_COST: return b * 13 * 8;
    case MPCQ_SV_XREF: return b * 12 * (N + 1) * 8;
    case MPCQ_SV_FSTEPS: return b * 260 * 8;
    case MPCQ_SV_GAIT: case SP_GAIT_INIT: case SP_IN_GAIT: return b * 100 * 8;
    case MPCQ_SV_Y: return b * 44 * N * 8;
    case MPCQ_SV_RHO: case MPCQ_SV_H_ROT: return b * 8;
    case MPCQ_SV_STATUS: case MPCQ_SV_ITERS: case MPCQ_SV_ROT_FLAG: case MPCQ_SV_ORDER: case MPCQ_SV_FIRST:
    case SP_PLAN_STATUS: case SP_IN_REDUCED: return b * 4;
    case SP_INFO: return b * 16;
  }
  return 0;  // (the swing arrays exist from mpcq_session_enable_swing on)
}

// Bytes of the arrays of the other groups: the one statement, for the enables that allocate them
// and for the snapshots that mirror them.
void swing_bytes(size_t B, int k_mpc, size_t nb[3]) {  // MPCQ_SV_SWING_REF, _SWING_STATE, _FRAME
  nb[0] = B * k_mpc * 36 * 8; nb[1] = B * 4 * MPCQ_SWING_STATE * 8; nb[2] = B * 24;
}
void plant_bytes(size_t B, size_t nb[PP_COUNT]) {  // STATE_END, F_EFF, WRENCH, qw_prev
  nb[MPCQ_PV_STATE_END] = B * 96; nb[MPCQ_PV_F_EFF] = B * 96; nb[MPCQ_PV_WRENCH] = B * 48; nb[PP_QW_PREV] = B * 48;
}
void monitor_bytes(size_t B, size_t nb[MPCQ_MV_COUNT]) {  // DONE, EP, EP_TICKS, EPISODES, LAST, TOTALS
  const size_t m[MPCQ_MV_COUNT] = {B * 4, B * 64, B * 4, B * 4, B * 128, 64};
  for (int w = 0; w < MPCQ_MV_COUNT; ++w) nb[w] = m[w];
}
void scenario_bytes(size_t B, size_t nb[MPCQ_CV_COUNT]) {  // EPOCH, TICK, V_REF, PUSH, WRENCH, ROBOTS, DRAW
  const size_t c[MPCQ_CV_COUNT] = {B * 4, B * 4, B * 48, B * 48, B * 48, B * sizeof(mpcq_robot), B * 64};
  for (int w = 0; w < MPCQ_CV_COUNT; ++w) nb[w] = c[w];
}

void channel_bytes(size_t B, size_t nb[MPCQ_HV_COUNT]) {  // CLOCK, OBS, F_CMD, DRAW, S_RING, F_RING
  const size_t h[MPCQ_HV_COUNT] = {B * 8, B * 96, B * 96, B * 128, B * MPCQ_CHANNEL_MAX_DELAY * 96,
                                   B * MPCQ_CHANNEL_MAX_LATENCY * 96};
  for (int w = 0; w < MPCQ_HV_COUNT; ++w) nb[w] = h[w];
}

void estimator_bytes(size_t B, size_t nb[MPCQ_EV_COUNT]) {  // EST, ROW
  nb[MPCQ_EV_EST] = B * 96; nb[MPCQ_EV_ROW] = B * MPCQ_EST_ROW * 8;
}

void disturb_bytes(size_t B, size_t nb[MPCQ_DV_COUNT]) {  // DIST, ROW, RESID
  nb[MPCQ_DV_DIST] = B * sizeof(mpcq_disturbance); nb[MPCQ_DV_ROW] = B * MPCQ_DIST_ROW * 8; nb[MPCQ_DV_RESID] = B * 48;
}

// n arrays of nb[i] bytes, each 256-B aligned, in one allocation zeroed on the context's
// stream (the call blocks): *mem, ptr[i] (null where nb[i] is 0) and bytes[i].  On a failure
// nothing stays allocated and nothing is written.
int alloc_group(mpcq_ctx* c, const char* what, int n, const size_t* nb, void** mem, void** ptr, size_t* bytes) {
  auto padded = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t tot = 0;
  for (int i = 0; i < n; ++i) tot += padded(nb[i]);
  void* m = nullptr;
  if (hipMalloc(&m, tot) != hipSuccess) return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) for %s failed", tot, what);
  hipError_t e = hipMemsetAsync(m, 0, tot, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipFree(m);
    return fail(MPCQ_E_DEVICE, "zeroing %s failed: %s", what, hipGetErrorString(e));
  }
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    ptr[i] = nb[i] ? (char*)m + off : nullptr;
    bytes[i] = nb[i];
    off += padded(nb[i]);
  }
  *mem = m;
  return MPCQ_OK;
}

// The array behind an id of group g, for the _read / _write / _device_ptr entry points.
int find(const Group& g, int what) {
  if (what < 0 || what >= g.named) return fail(MPCQ_E_INVALID, "unknown %s array %d", g.kind, what);
  if (!g.ptr[what]) return fail(MPCQ_E_INVALID, "%s array %d needs mpcq_session_enable_%s", g.kind, what, g.enable);
  return MPCQ_OK;
}

int group_read(mpcq_session* s, Group mpcq_session::*group, int what, void* dst, uint32_t flags) {
  if (!s || !dst) return fail(MPCQ_E_INVALID, "NULL argument");
  const Group& g = s->*group;
  const int rc = find(g, what);
  if (rc) return rc;
  DeviceGuard dg(s->ctx->device);
  const hipMemcpyKind kind = (flags & MPCQ_FLAG_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(hipMemcpyAsync(dst, g.ptr[what], g.bytes[what], kind, s->ctx->stream));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  return MPCQ_OK;
}

int group_device_ptr(mpcq_session* s, Group mpcq_session::*group, int what, void** out) {
  if (!s || !out) return fail(MPCQ_E_INVALID, "NULL argument");
  const int rc = find(s->*group, what);
  if (rc) return rc;
  *out = (s->*group).ptr[what];
  return MPCQ_OK;
}

// An optional input array where the kernels read it: a device pointer as it is; a host array
// through the session's staging buffer `buf`, copied on the context's stream (stream-ordered
// with the ticks; the call has to block before the buffer can be reused).  *e keeps the
// first error.
template <class T>
const T* staged(mpcq_session* s, bool dev, const T* src, int buf, hipError_t* e) {
  if (!src || dev) return src;
  if (*e == hipSuccess)
    *e = hipMemcpyAsync(s->sv.ptr[buf], src, s->sv.bytes[buf], hipMemcpyHostToDevice, s->ctx->stream);
  return (const T*)s->sv.ptr[buf];
}

// What mpcq_session_reset enqueues on the context's stream, from device pointers: the reset
// launch and, on a session that has ticked, the next solve's order.  Shared with a tick's
// auto-reset (mpcq_session_enable_monitor) and, with mark == false over all robots, with
// mpcq_session_create: the creation state is what reset_kernel writes, and nothing else.
hipError_t enqueue_reset(mpcq_session* s, const int32_t* mask, const double* gait0, const double* q_w0, bool mark) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->sv;
  mpcq::ResetArgs ra{};
  ra.batch = s->B; ra.N = c->N; ra.mask = mask; ra.q_w0 = q_w0;
  ra.gait_src = gait0 ? gait0 : v.d(SP_GAIT_INIT);
  ra.h_ref = s->pp.h_ref; ra.rho0 = c->p.rho;
  for (int i = 0; i < 8; ++i) ra.shoulders[i] = s->pp.shoulders[i];
  ra.gait = v.d(MPCQ_SV_GAIT); ra.rot_flag = v.i(MPCQ_SV_ROT_FLAG); ra.h_rot = v.d(MPCQ_SV_H_ROT);
  ra.xref = v.d(MPCQ_SV_XREF); ra.fsteps = v.d(MPCQ_SV_FSTEPS); ra.q_w = v.d(MPCQ_SV_Q_W);
  ra.state = v.d(MPCQ_SV_STATE); ra.l_feet = v.d(MPCQ_SV_L_FEET); ra.rho = v.d(MPCQ_SV_RHO);
  ra.y = v.d(MPCQ_SV_Y); ra.warm_x = v.d(SP_WARM_X); ra.x = v.d(MPCQ_SV_X); ra.f0 = v.d(MPCQ_SV_F0);
  ra.x_robot = v.d(MPCQ_SV_X_ROBOT); ra.cost = v.d(MPCQ_SV_COST);
  ra.status = v.i(MPCQ_SV_STATUS); ra.iters = v.i(MPCQ_SV_ITERS);
  ra.first = mark ? v.i(MPCQ_SV_FIRST) : nullptr;
  if (s->swing) {
    ra.swing_ref = v.d(MPCQ_SV_SWING_REF); ra.swing_ref_doubles = (int64_t)s->sp.k_mpc * 36;
    ra.swing_state = v.d(MPCQ_SV_SWING_STATE); ra.frame = v.d(MPCQ_SV_FRAME);
  }
  if (s->mv.mem) {  // a reset robot's running episode is discarded
    ra.ep = s->mv.d(MPCQ_MV_EP); ra.ep_ticks = s->mv.i(MPCQ_MV_EP_TICKS);
  }
  if (s->gv.mem) ra.gstate = s->gv.i(MPCQ_GV_STATE);  // no request, the table's own roll
  hipError_t e = mpcq::launch_reset(ra, c->stream);
  // the robots with a pending reset to the front of the next solve's dispatch (a session that
  // has not ticked yet has no order in use: it keeps the identity)
  if (e == hipSuccess && s->have_order)
    e = mpcq::launch_order(v.i(MPCQ_SV_ITERS), ra.first, s->B, v.i(MPCQ_SV_ORDER), c->stream);
  if (mark) s->resets = true;
  return e;
}

// The plant's arrays, all zero: made by the first mpcq_session_enable_plant / _set_wrench.
int ensure_plant_mem(mpcq_session* s) {
  if (s->pv.mem) return MPCQ_OK;
  size_t nb[PP_COUNT];
  plant_bytes((size_t)s->B, nb);
  return alloc_group(s->ctx, "the plant arrays", PP_COUNT, nb, &s->pv.mem, s->pv.ptr, s->pv.bytes);
}

// The table of the robots the plant moves, or null (the context's params): the plant's own,
// else the model's.
const mpcq_robot* plant_table(const mpcq_session* s) {
  return s->plant_robots.count ? s->plant_robots.dev : s->robots.count ? s->robots.dev : nullptr;
}

// The scenario launch: a tick's (first = MPCQ_SV_FIRST or null, all_first at k == 0), or with
// init the one mpcq_session_enable_scenario enqueues.
hipError_t enqueue_scenario(mpcq_session* s, const mpcq_scenario_params& sc, const int32_t* first, bool all_first,
                            bool init) {
  const Group& v = s->cv;
  mpcq::ScenarioArgs a{};
  a.batch = s->B; a.first = first; a.all_first = all_first; a.init = init;
  a.epoch = v.i(MPCQ_CV_EPOCH); a.tick = v.i(MPCQ_CV_TICK);
  a.base = plant_table(s);
  mpcq_default_robot(&s->ctx->p, &a.dflt);
  a.wrench_in = s->pv.mem ? s->pv.d(MPCQ_PV_WRENCH) : nullptr;
  a.v_ref = v.d(MPCQ_CV_V_REF); a.push = v.d(MPCQ_CV_PUSH); a.wrench_out = v.d(MPCQ_CV_WRENCH);
  a.robots_out = (mpcq_robot*)v.ptr[MPCQ_CV_ROBOTS]; a.draw = v.d(MPCQ_CV_DRAW);
  return mpcq::launch_scenario(sc, a, s->ctx->stream);
}

}  // namespace

extern "C" {

int mpcq_session_create(mpcq_ctx* c, int64_t B, const mpcq_planner_params* pp, const double* gait0,
                        mpcq_session** out) {
  if (!out) return fail(MPCQ_E_INVALID, "out is NULL");
  *out = nullptr;
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (B < 1) return fail(MPCQ_E_INVALID, "a session needs batch >= 1");
  const int N = c->N;
  mpcq_planner_params P;
  if (pp) P = *pp;
  else mpcq_default_planner_params(&P);
  // host scratch: without gait0 the walking-trot table, then the identity order
  const size_t gb = gait0 ? 0 : (size_t)B * 800;
  char* h = (char*)malloc(gb + (size_t)B * 4);
  if (!h) return fail(MPCQ_E_NOMEM, "host malloc failed");
  if (!gait0) {  // create_walking_trot (FootstepPlanner.py:193-214): [1, 7, 1, 7] per 16-step period
    const int half = (int)(0.5 * P.T_gait / P.dt);
    const int per = 2 * half, nper = per > 0 ? N / per : 0;
    if (nper < 1 || nper * per != N || 4 * nper > 19) {
      free(h);
      return fail(MPCQ_E_INVALID, "no walking-trot table for N=%d with T_gait/dt = %d; pass gait0", N, per);
    }
    for (int64_t b = 0; b < B; ++b) {
      double* gt = (double*)h + b * 100;
      for (int e = 0; e < 100; ++e) gt[e] = 0.0;
      for (int i = 0; i < nper; ++i) {
        const double d[4] = {1.0, half - 1.0, 1.0, half - 1.0};
        const int m[4][4] = {{1, 1, 1, 1}, {1, 0, 0, 1}, {1, 1, 1, 1}, {0, 1, 1, 0}};
        for (int r = 0; r < 4; ++r) {
          gt[5 * (4 * i + r)] = d[r];
          for (int q = 0; q < 4; ++q) gt[5 * (4 * i + r) + 1 + q] = m[r][q];
        }
      }
    }
    gait0 = (const double*)h;
  }
  int32_t* ident = (int32_t*)(h + gb);  // a permutation from the start
  for (int64_t b = 0; b < B; ++b) ident[b] = (int32_t)b;
  mpcq_session* s = new mpcq_session();
  s->ctx = c;
  s->B = B;
  s->pp = P;
  {
    const char* e = getenv("MPCQ_DISPATCH_ORDER");
    s->use_order = !(e && e[0] == '0');
  }
  size_t nb[SP_COUNT];
  for (int w = 0; w < SP_COUNT; ++w) nb[w] = sv_bytes(w, B, N);
  DeviceGuard g(c->device);
  rc = alloc_group(c, "the session", SP_COUNT, nb, &s->sv.mem, s->sv.ptr, s->sv.bytes);
  if (rc) {
    free(h);
    delete s;
    return rc;
  }
  // every array defined before the first tick: the table a reset without gait0 goes back to,
  // the order, and what a reset of every robot writes (the gait table from gait_init) -- but
  // with no reset pending: MPCQ_SV_FIRST stays zero
  const Group& v = s->sv;
  hipError_t e = hipMemcpyAsync(v.ptr[SP_GAIT_INIT], gait0, v.bytes[SP_GAIT_INIT], hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(v.ptr[MPCQ_SV_ORDER], ident, v.bytes[MPCQ_SV_ORDER], hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = enqueue_reset(s, nullptr, nullptr, nullptr, false);
  const hipError_t es = hipStreamSynchronize(c->stream);
  free(h);
  if (e != hipSuccess || es != hipSuccess) {
    mpcq_session_destroy(s);
    return fail(MPCQ_E_DEVICE, "initialising the session failed");
  }
  *out = s;
  return MPCQ_OK;
}

int mpcq_session_destroy(mpcq_session* s) {
  if (!s) return MPCQ_OK;
  if (s->sv.mem) {
    DeviceGuard g(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    (void)hipFree(s->sv.mem);
    if (s->swing_mem) (void)hipFree(s->swing_mem);
    if (s->robots.dev) (void)hipFree(s->robots.dev);
    if (s->pv.mem) (void)hipFree(s->pv.mem);
    if (s->plant_robots.dev) (void)hipFree(s->plant_robots.dev);
    if (s->weights.dev) (void)hipFree(s->weights.dev);
    if (s->disturb.dev) (void)hipFree(s->disturb.dev);
    mpcq::free_tables(s->fill);
    if (s->mv.mem) (void)hipFree(s->mv.mem);
    if (s->cv.mem) (void)hipFree(s->cv.mem);
    if (s->hv.mem) (void)hipFree(s->hv.mem);
    if (s->ev.mem) (void)hipFree(s->ev.mem);
    if (s->gv.mem) (void)hipFree(s->gv.mem);
    if (s->dv.mem) (void)hipFree(s->dv.mem);
    (void)mpcq_session_snapshot_destroy(s->fork_snap);
  }
  delete s;
  return MPCQ_OK;
}

int mpcq_session_set_robots(mpcq_session* s, const mpcq_robot* robots, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  return set_table(s->ctx, s->robots, robots ? s->B : 0, robots, flags);
}

int mpcq_session_get_robots(mpcq_session* s, mpcq_robot* robots, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!robots) return fail(MPCQ_E_INVALID, "robots is NULL");
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  const size_t nb = (size_t)s->B * sizeof(mpcq_robot);
  if (s->robots.count) {
    HIP_TRY(hipMemcpyAsync(robots, s->robots.dev, nb, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MPCQ_OK;
  }
  mpcq_robot d;
  mpcq_default_robot(&c->p, &d);
  if (!dev) {
    for (int64_t b = 0; b < s->B; ++b) robots[b] = d;
    return MPCQ_OK;
  }
  mpcq_robot* h = (mpcq_robot*)malloc(nb);
  if (!h) return fail(MPCQ_E_NOMEM, "host malloc failed");
  for (int64_t b = 0; b < s->B; ++b) h[b] = d;
  const hipError_t e = hipMemcpy(robots, h, nb, hipMemcpyHostToDevice);
  free(h);
  HIP_TRY(e);
  return MPCQ_OK;
}

int mpcq_session_set_weights(mpcq_session* s, const mpcq_weights* weights, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  return set_table(s->ctx, s->weights, weights ? s->B : 0, weights, flags);
}

int mpcq_session_get_weights(mpcq_session* s, mpcq_weights* weights, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!weights) return fail(MPCQ_E_INVALID, "weights is NULL");
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  const size_t nb = (size_t)s->B * sizeof(mpcq_weights);
  if (s->weights.count) {
    HIP_TRY(hipMemcpyAsync(weights, s->weights.dev, nb, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MPCQ_OK;
  }
  mpcq_weights d;
  mpcq_default_weights(&c->p, &d);
  if (!dev) {
    for (int64_t b = 0; b < s->B; ++b) weights[b] = d;
    return MPCQ_OK;
  }
  mpcq_weights* h = (mpcq_weights*)malloc(nb);
  if (!h) return fail(MPCQ_E_NOMEM, "host malloc failed");
  for (int64_t b = 0; b < s->B; ++b) h[b] = d;
  const hipError_t e = hipMemcpy(weights, h, nb, hipMemcpyHostToDevice);
  free(h);
  HIP_TRY(e);
  return MPCQ_OK;
}

int mpcq_session_set_disturbance(mpcq_session* s, const mpcq_disturbance* table, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  return set_table(s->ctx, s->disturb, table ? s->B : 0, table, flags);
}

int mpcq_session_get_disturbance(mpcq_session* s, mpcq_disturbance* table, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!table) return fail(MPCQ_E_INVALID, "table is NULL");
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  const size_t nb = (size_t)s->B * sizeof(mpcq_disturbance);
  if (s->disturb.count) {
    HIP_TRY(hipMemcpyAsync(table, s->disturb.dev, nb, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MPCQ_OK;
  }
  if (!dev) {  // (without a table: no disturbance)
    memset(table, 0, nb);
    return MPCQ_OK;
  }
  HIP_TRY(hipMemset(table, 0, nb));
  return MPCQ_OK;
}

int mpcq_session_enable_swing(mpcq_session* s, const mpcq_swing_params* sp) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_swing_params P;
  int rc = swing_params(sp, &P);
  if (rc) return rc;
  if (s->swing) {
    if (P.k_mpc != s->sp.k_mpc) return fail(MPCQ_E_INVALID, "swing is enabled with k_mpc = %d", s->sp.k_mpc);
    s->sp = P;
    return MPCQ_OK;
  }
  size_t nb[3];  // all-zero state = new generators
  swing_bytes((size_t)s->B, P.k_mpc, nb);
  DeviceGuard g(s->ctx->device);
  rc = alloc_group(s->ctx, "the swing arrays", 3, nb, &s->swing_mem, s->sv.ptr + MPCQ_SV_SWING_REF,
                   s->sv.bytes + MPCQ_SV_SWING_REF);
  if (rc) return rc;
  s->sp = P;
  s->swing = true;
  return MPCQ_OK;
}

int mpcq_session_enable_plant(mpcq_session* s, const mpcq_plant_params* pl) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_plant_params P;
  int rc = plant_params(pl, s->ctx->p.dt, &P);
  if (rc) return rc;
  if (P.dt != s->ctx->p.dt)
    return fail(MPCQ_E_INVALID, "the plant's dt %g is not the context's %g", P.dt, s->ctx->p.dt);
  DeviceGuard g(s->ctx->device);
  rc = ensure_plant_mem(s);
  if (rc) return rc;
  s->pl = P;
  s->plant = true;
  return MPCQ_OK;
}

int mpcq_session_disable_plant(mpcq_session* s) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  s->plant = false;
  return MPCQ_OK;
}

int mpcq_session_set_plant_robots(mpcq_session* s, const mpcq_robot* robots, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  return set_table(s->ctx, s->plant_robots, robots ? s->B : 0, robots, flags);
}

int mpcq_session_set_wrench(mpcq_session* s, const double* wrench, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const int rc = ensure_plant_mem(s);
  if (rc) return rc;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  void* dst = s->pv.ptr[MPCQ_PV_WRENCH];
  const size_t nb = s->pv.bytes[MPCQ_PV_WRENCH];
  // on the context's stream: behind every queued tick that still reads the old wrench
  if (!wrench) HIP_TRY(hipMemsetAsync(dst, 0, nb, c->stream));
  else HIP_TRY(hipMemcpyAsync(dst, wrench, nb, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  if (!(flags & MPCQ_FLAG_ASYNC) || !dev) HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

int mpcq_session_enable_monitor(mpcq_session* s, const mpcq_monitor_params* mp) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_monitor_params P;
  int rc = monitor_params(mp, &P);
  if (rc) return rc;
  if (!s->mv.mem) {  // the arrays, zero but for ep[4] = +inf
    mpcq_ctx* c = s->ctx;
    DeviceGuard g(c->device);
    const size_t B = (size_t)s->B;
    size_t nb[MPCQ_MV_COUNT];
    monitor_bytes(B, nb);
    double* h = (double*)malloc(nb[MPCQ_MV_EP]);
    if (!h) return fail(MPCQ_E_NOMEM, "host malloc failed");
    for (size_t e = 0; e < B * 8; ++e) h[e] = e % 8 == 4 ? INFINITY : 0.0;
    Group mv = s->mv;
    rc = alloc_group(c, "the monitor arrays", MPCQ_MV_COUNT, nb, &mv.mem, mv.ptr, mv.bytes);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(mv.ptr[MPCQ_MV_EP], h, nb[MPCQ_MV_EP], hipMemcpyHostToDevice, c->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    free(h);
    if (rc) return rc;
    if (e != hipSuccess) {
      (void)hipFree(mv.mem);
      return fail(MPCQ_E_DEVICE, "initialising the monitor arrays failed: %s", hipGetErrorString(e));
    }
    s->mv = mv;
  }
  s->mp = P;
  s->monitor = true;
  return MPCQ_OK;
}

int mpcq_session_disable_monitor(mpcq_session* s) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  s->monitor = false;
  return MPCQ_OK;
}

int mpcq_session_enable_scenario(mpcq_session* s, const mpcq_scenario_params* sc) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_scenario_params P;
  int rc = scenario_params(sc, &P);
  if (rc) return rc;
  if (!s->cv.mem) {  // the arrays, zero; the launch gives every robot the draw of epoch 0
    size_t nb[MPCQ_CV_COUNT];
    scenario_bytes((size_t)s->B, nb);
    DeviceGuard g(s->ctx->device);
    Group cv = s->cv;
    rc = alloc_group(s->ctx, "the scenario arrays", MPCQ_CV_COUNT, nb, &cv.mem, cv.ptr, cv.bytes);
    if (rc) return rc;
    s->cv = cv;
    const hipError_t e = enqueue_scenario(s, P, nullptr, false, true);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s->ctx->stream);
      (void)hipFree(cv.mem);
      s->cv = Group{"scenario", "scenario", MPCQ_CV_COUNT};
      return fail(MPCQ_E_DEVICE, "initialising the scenario arrays failed: %s", hipGetErrorString(e));
    }
  }
  s->sc = P;
  s->scenario = true;
  return MPCQ_OK;
}

int mpcq_session_disable_scenario(mpcq_session* s) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  s->scenario = false;
  return MPCQ_OK;
}

int mpcq_session_enable_channel(mpcq_session* s, const mpcq_channel_params* ch) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_channel_params P;
  int rc = channel_params(ch, &P);
  if (rc) return rc;
  DeviceGuard g(s->ctx->device);
  const bool fresh = !s->hv.mem;
  Group hv = s->hv;
  if (fresh) {  // the arrays, zero
    size_t nb[MPCQ_HV_COUNT];
    channel_bytes((size_t)s->B, nb);
    rc = alloc_group(s->ctx, "the channel arrays", MPCQ_HV_COUNT, nb, &hv.mem, hv.ptr, hv.bytes);
    if (rc) return rc;
  }
  // the rings hold nothing the coming ticks may read: every robot primes at its next observe
  if (!s->channel || P.delay != s->ch.delay || P.latency != s->ch.latency) {
    const hipError_t e = mpcq::launch_channel_arm(hv.i(MPCQ_HV_CLOCK), s->B, s->ctx->stream);
    if (e != hipSuccess) {
      if (fresh) {
        (void)hipStreamSynchronize(s->ctx->stream);
        (void)hipFree(hv.mem);
      }
      return fail(MPCQ_E_DEVICE, "arming the channel's clock failed: %s", hipGetErrorString(e));
    }
  }
  s->hv = hv;
  s->ch = P;
  s->channel = true;
  return MPCQ_OK;
}

int mpcq_session_disable_channel(mpcq_session* s) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  s->channel = false;
  return MPCQ_OK;
}

int mpcq_session_enable_estimator(mpcq_session* s, const mpcq_estimator_params* ep) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_estimator_params P;
  int rc = estimator_params(ep, &P);
  if (rc) return rc;
  DeviceGuard g(s->ctx->device);
  if (!s->ev.mem) {  // the arrays, zero: every filter invalid
    size_t nb[MPCQ_EV_COUNT];
    estimator_bytes((size_t)s->B, nb);
    Group ev = s->ev;
    rc = alloc_group(s->ctx, "the estimator arrays", MPCQ_EV_COUNT, nb, &ev.mem, ev.ptr, ev.bytes);
    if (rc) return rc;
    s->ev = ev;
  } else if (!s->estimator) {  // the rings missed the ticks since the disable: every filter invalid again
    HIP_TRY(hipMemsetAsync(s->ev.ptr[MPCQ_EV_ROW], 0, s->ev.bytes[MPCQ_EV_ROW], s->ctx->stream));
  }
  s->ep = P;
  s->estimator = true;
  return MPCQ_OK;
}

int mpcq_session_disable_estimator(mpcq_session* s) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  s->estimator = false;
  return MPCQ_OK;
}

int mpcq_session_enable_disturb(mpcq_session* s, const mpcq_disturb_params* dp) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_disturb_params P;
  int rc = disturb_params(dp, &P);
  if (rc) return rc;
  DeviceGuard g(s->ctx->device);
  if (!s->dv.mem) {  // the arrays, zero: every row invalid, no disturbance
    size_t nb[MPCQ_DV_COUNT];
    disturb_bytes((size_t)s->B, nb);
    Group dv = s->dv;
    rc = alloc_group(s->ctx, "the disturb arrays", MPCQ_DV_COUNT, nb, &dv.mem, dv.ptr, dv.bytes);
    if (rc) return rc;
    s->dv = dv;
  } else if (!s->disturb_on) {  // the rings missed the ticks since the disable: every row invalid again
    for (int w = 0; w < MPCQ_DV_COUNT; ++w)
      HIP_TRY(hipMemsetAsync(s->dv.ptr[w], 0, s->dv.bytes[w], s->ctx->stream));
  }
  s->dp = P;
  s->disturb_on = true;
  return MPCQ_OK;
}

int mpcq_session_disable_disturb(mpcq_session* s) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  s->disturb_on = false;
  return MPCQ_OK;
}

int mpcq_session_enable_gait(mpcq_session* s, const mpcq_gait_params* gp, const double* cycles) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_gait_params P;
  mpcq::GaitArgs lib{};
  int rc = gait_params(gp, cycles, &P, &lib);
  if (rc) return rc;
  if (!s->gv.mem) {  // the rows, every one (-1, -1, 0, 0)
    mpcq_ctx* c = s->ctx;
    DeviceGuard g(c->device);
    const size_t nb[MPCQ_GV_COUNT] = {(size_t)s->B * 16};
    int32_t* h = (int32_t*)malloc(nb[0]);
    if (!h) return fail(MPCQ_E_NOMEM, "host malloc failed");
    for (size_t e = 0; e < (size_t)s->B * 4; ++e) h[e] = e % 4 < 2 ? -1 : 0;
    Group gv = s->gv;
    rc = alloc_group(c, "the gait array", MPCQ_GV_COUNT, nb, &gv.mem, gv.ptr, gv.bytes);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(gv.ptr[MPCQ_GV_STATE], h, nb[0], hipMemcpyHostToDevice, c->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    free(h);
    if (rc) return rc;
    if (e != hipSuccess) {
      (void)hipFree(gv.mem);
      return fail(MPCQ_E_DEVICE, "initialising the gait array failed: %s", hipGetErrorString(e));
    }
    s->gv = gv;
  }
  // (by value into every later launch's arguments: a queued tick keeps the library it was launched with)
  s->gp = P;
  s->gait_lib = lib;
  s->gait = true;
  return MPCQ_OK;
}

int mpcq_session_disable_gait(mpcq_session* s) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  s->gait = false;
  return MPCQ_OK;
}

int mpcq_session_set_gait(mpcq_session* s, const int32_t* ids, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!ids) return fail(MPCQ_E_INVALID, "ids is NULL");
  if (!s->gait) return fail(MPCQ_E_INVALID, "mpcq_session_set_gait needs mpcq_session_enable_gait");
  if (s->gp.select != MPCQ_GAIT_MANUAL)
    return fail(MPCQ_E_INVALID, "mpcq_session_set_gait is refused under MPCQ_GAIT_BY_SPEED: the kernel owns want");
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  if (!dev)
    for (int64_t b = 0; b < s->B; ++b)
      if (ids[b] < -1 || ids[b] >= s->gp.n_gaits)
        return fail(MPCQ_E_INVALID, "ids[%lld] = %d is neither -1 nor a gait of the library (0..%d)", (long long)b,
                    ids[b], s->gp.n_gaits - 1);
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  // want alone: element 0 of every 16-byte row, on the context's stream (behind the queued ticks)
  HIP_TRY(hipMemcpy2DAsync(s->gv.ptr[MPCQ_GV_STATE], 16, ids, 4, 4, (size_t)s->B,
                           dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  if (!(flags & MPCQ_FLAG_ASYNC) || !dev) HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

}  // extern "C"

namespace {

// One tick's inputs where its kernels read them, and what makes it a first tick.
struct Tick {
  int k;
  const double *state, *l_feet, *v_ref;
  const double* plan_state;  // what the planner takes as the state: state, the channel's observation, or
                             // the estimator's estimate
  const int32_t* reduced;  // or null
  // after a mpcq_session_reset: a robot whose MPCQ_SV_FIRST is set runs this tick as a first
  // tick whatever k says (the planner's extra pass then touches those robots only)
  // (k == 0 makes every robot first by itself: only the retrieve takes the flags then, to clear them)
  int32_t* first;          // MPCQ_SV_FIRST, or null before any reset
  const int32_t* first_k;  // first, or null at k == 0
  double* trace;           // [B][MPCQ_TRACE] (device) or null: the monitor's row of this tick
};

// Host arrays through the staging buffers; the virtual robot's state (state / l_feet null)
// lives in arrays the retrieve kernel rewrites: this tick reads a copy.
int tick_inputs(mpcq_session* s, const double* state, const double* l_feet, const double* v_ref,
                const int32_t* reduced, bool dev, Tick& t) {
  const Group& v = s->sv;
  hipStream_t st = s->ctx->stream;
  hipError_t e = hipSuccess;
  t.state = staged(s, dev, state, SP_IN_STATE, &e);
  t.l_feet = staged(s, dev, l_feet, SP_IN_LFEET, &e);
  t.v_ref = staged(s, dev, v_ref, SP_IN_VREF, &e);
  t.reduced = staged(s, dev, reduced, SP_IN_REDUCED, &e);
  if (e != hipSuccess) return fail(MPCQ_E_DEVICE, "staging the tick inputs failed");
  if (!state) {
    HIP_TRY(hipMemcpyAsync(v.ptr[SP_IN_STATE], v.ptr[MPCQ_SV_STATE], v.bytes[SP_IN_STATE], hipMemcpyDeviceToDevice, st));
    t.state = v.d(SP_IN_STATE);
  }
  if (!l_feet) {
    HIP_TRY(hipMemcpyAsync(v.ptr[SP_IN_LFEET], v.ptr[MPCQ_SV_L_FEET], v.bytes[SP_IN_LFEET], hipMemcpyDeviceToDevice, st));
    t.l_feet = v.d(SP_IN_LFEET);
  }
  t.plan_state = t.state;
  t.first = s->resets ? v.i(MPCQ_SV_FIRST) : nullptr;
  t.first_k = t.k == 0 ? nullptr : t.first;
  return MPCQ_OK;
}

// This tick's command, push and (on a first tick) true robots; it takes the first flags as
// the planner will.
int tick_scenario(mpcq_session* s, int k) {
  const int32_t* first = s->resets && k != 0 ? s->sv.i(MPCQ_SV_FIRST) : nullptr;
  HIP_TRY(enqueue_scenario(s, s->sc, first, k == 0, false));
  return MPCQ_OK;
}

// The channel's measurement model: the planner's state becomes the observation of the truth
// (t.state, which the plant keeps); it takes the first flags as the planner will.
int tick_observe(mpcq_session* s, Tick& t) {
  const Group& h = s->hv;
  mpcq::ObserveArgs a{};
  a.batch = s->B; a.first = t.first_k; a.all_first = t.k == 0; a.truth = t.state;
  a.clock = h.i(MPCQ_HV_CLOCK); a.obs = h.d(MPCQ_HV_OBS); a.draw = h.d(MPCQ_HV_DRAW);
  a.s_ring = h.d(MPCQ_HV_S_RING); a.f_ring = h.d(MPCQ_HV_F_RING);
  HIP_TRY(mpcq::launch_observe(s->ch, a, s->ctx->stream));
  t.plan_state = h.d(MPCQ_HV_OBS);
  return MPCQ_OK;
}

// The estimator: the planner's state becomes the filter's estimate from what it would have
// taken (t.plan_state), the previous tick's f0, feet and statuses as they stand before this
// tick's planner, and the model's robots; it takes the first flags as the planner will.
int tick_estimate(mpcq_session* s, Tick& t) {
  mpcq_ctx* c = s->ctx;
  const Group &v = s->sv, &e = s->ev;
  mpcq::EstimateArgs a{};
  a.batch = s->B; a.first = t.first_k; a.all_first = t.k == 0; a.obs = t.plan_state;
  a.f_prev = v.d(MPCQ_SV_F0); a.fsteps = v.d(MPCQ_SV_FSTEPS);
  a.status = v.i(MPCQ_SV_STATUS); a.plan_status = v.i(SP_PLAN_STATUS);
  a.robots = s->robots.count ? s->robots.dev : nullptr;
  mpcq_default_robot(&c->p, &a.dflt);
  a.dt = c->p.dt; a.gravity = c->p.gravity;
  a.row = e.d(MPCQ_EV_ROW); a.est = e.d(MPCQ_EV_EST);
  HIP_TRY(mpcq::launch_estimate(s->ep, a, c->stream));
  t.plan_state = e.d(MPCQ_EV_EST);
  return MPCQ_OK;
}

// The disturbance stage: MPCQ_DV_DIST from what the planner is about to take as its state
// (t.plan_state, which stays), the previous tick's f0, feet and statuses as they stand before
// this tick's planner, and the model's robots; it takes the first flags as the planner will.
int tick_disturb(mpcq_session* s, const Tick& t) {
  mpcq_ctx* c = s->ctx;
  const Group &v = s->sv, &d = s->dv;
  mpcq::DisturbArgs a{};
  a.batch = s->B; a.first = t.first_k; a.all_first = t.k == 0; a.meas = t.plan_state;
  a.f_prev = v.d(MPCQ_SV_F0); a.fsteps = v.d(MPCQ_SV_FSTEPS);
  a.status = v.i(MPCQ_SV_STATUS); a.plan_status = v.i(SP_PLAN_STATUS);
  a.robots = s->robots.count ? s->robots.dev : nullptr;
  mpcq_default_robot(&c->p, &a.dflt);
  a.dt = c->p.dt; a.gravity = c->p.gravity;
  a.row = d.d(MPCQ_DV_ROW); a.dist = (mpcq_disturbance*)d.ptr[MPCQ_DV_DIST]; a.resid = d.d(MPCQ_DV_RESID);
  HIP_TRY(mpcq::launch_disturb(s->dp, a, c->stream));
  return MPCQ_OK;
}

// The channel's actuation model: MPCQ_HV_F_CMD from this tick's (and earlier) MPCQ_SV_F0.
int tick_actuate(mpcq_session* s) {
  const Group& h = s->hv;
  mpcq::ActuateArgs a{};
  a.batch = s->B; a.f0 = s->sv.d(MPCQ_SV_F0); a.clock = h.i(MPCQ_HV_CLOCK); a.draw = h.d(MPCQ_HV_DRAW);
  a.f_ring = h.d(MPCQ_HV_F_RING); a.f_cmd = h.d(MPCQ_HV_F_CMD);
  HIP_TRY(mpcq::launch_actuate(s->ch, a, s->ctx->stream));
  return MPCQ_OK;
}

// The planner (processing.py:80-89, 131), between ev[0] and ev[1].
int tick_plan(mpcq_session* s, const Tick& t) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->sv;
  mpcq::PlanArgs a{};
  a.batch = s->B; a.N = c->N; a.k = t.k; a.first = t.first_k;
  a.state = t.plan_state; a.l_feet = t.l_feet; a.v_ref = t.v_ref; a.reduced = t.reduced;
  a.gait = v.d(MPCQ_SV_GAIT); a.rot_flag = v.i(MPCQ_SV_ROT_FLAG); a.h_rot = v.d(MPCQ_SV_H_ROT);
  a.xref = v.d(MPCQ_SV_XREF); a.fsteps = v.d(MPCQ_SV_FSTEPS); a.status = v.i(SP_PLAN_STATUS);
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  if (t.k == 0 || t.first_k) {  // update_fsteps(0, ...): no roll
    a.ops = MPCQ_PLAN_FOOTSTEPS;
    HIP_TRY(mpcq::launch_plan(s->pp, a, c->stream));
  }
  a.ops = MPCQ_PLAN_TICK;
  if (s->gait) {  // the gait stage rolls in the planner's place, on the command the planner reads
    mpcq::GaitArgs ga = s->gait_lib;
    ga.batch = s->B; ga.v_ref = t.v_ref; ga.gait = v.d(MPCQ_SV_GAIT); ga.gstate = s->gv.i(MPCQ_GV_STATE);
    HIP_TRY(mpcq::launch_gait(s->gp, ga, c->stream));
    a.ops = MPCQ_PLAN_FOOTSTEPS | MPCQ_PLAN_REFSTATES;
  }
  HIP_TRY(mpcq::launch_plan(s->pp, a, c->stream));
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  c->have_form = true;
  return MPCQ_OK;
}

// MPC.run: formulation + OSQP solve (warm from the previous tick when k > 0), between ev[2]
// and ev[3].
int tick_solve(mpcq_session* s, const Tick& t) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->sv;
  mpcq::LaunchArgs a{};
  a.batch = s->B;
  a.mode = t.k == 0 ? MPCQ_MODE_SETUP : MPCQ_MODE_UPDATE;
  a.xref = v.d(MPCQ_SV_XREF); a.fsteps = v.d(MPCQ_SV_FSTEPS);
  if (t.k > 0) {
    a.warm_x = v.d(SP_WARM_X); a.warm_y = v.d(MPCQ_SV_Y); a.rho_in = v.d(MPCQ_SV_RHO);
  }
  a.f0 = v.d(MPCQ_SV_F0); a.x = v.d(MPCQ_SV_X); a.y = v.d(MPCQ_SV_Y); a.rho_out = v.d(MPCQ_SV_RHO);
  a.status = v.i(MPCQ_SV_STATUS); a.iters = v.i(MPCQ_SV_ITERS); a.info = v.i(SP_INFO);
  a.stamps = c->stamps;
  // longest-first by the previous tick's iteration counts (a tick k == 0 restarts cold)
  if (t.k == 0) s->have_order = false;
  a.order = s->have_order && s->use_order ? v.i(MPCQ_SV_ORDER) : nullptr;
  // a compensating disturbance stage: its estimate, ahead of the user's table
  DisturbTable est;
  est.dev = (mpcq_disturbance*)s->dv.ptr[MPCQ_DV_DIST];
  est.cap = est.count = s->B;
  const bool comp = s->disturb_on && s->dp.compensate != 0;
  int rc = mpcq::launch_tables(c, s->robots, &s->weights, comp ? est : s->disturb, s->fill, s->B, &a);
  if (rc) return rc;
  a.first = t.first_k;
  rc = ensure_work(c, s->B, &a.work);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(mpcq::launch_solve(c->N, true, c->p, a, c->stream));
  HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  c->have_solve = true;
  return MPCQ_OK;
}

// retrieve_result, q_w, Logger cost, next warm start, virtual robot; before it, the copies of
// q_w that swing and plant need as it stands before the retrieve moves it.
int tick_retrieve(mpcq_session* s, const Tick& t) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->sv;
  const size_t B = (size_t)s->B;
  mpcq::SessionArgs a{};
  a.batch = s->B;
  a.x = v.d(MPCQ_SV_X); a.xref = v.d(MPCQ_SV_XREF); a.fsteps = v.d(MPCQ_SV_FSTEPS); a.gait = v.d(MPCQ_SV_GAIT);
  a.status = v.i(MPCQ_SV_STATUS); a.plan_status = v.i(SP_PLAN_STATUS);
  a.x_robot = v.d(MPCQ_SV_X_ROBOT); a.warm_x = v.d(SP_WARM_X); a.y = v.d(MPCQ_SV_Y);
  a.rho = v.d(MPCQ_SV_RHO); a.rho0 = c->p.rho; a.cost = v.d(MPCQ_SV_COST); a.q_w = v.d(MPCQ_SV_Q_W);
  a.next_state = v.d(MPCQ_SV_STATE); a.next_l_feet = v.d(MPCQ_SV_L_FEET);
  for (int i = 0; i < 12; ++i) a.state_weights[i] = c->p.state_weights[i];
  a.force_weight = c->p.force_weight;
  a.weights = s->weights.count ? s->weights.dev : nullptr;
  for (int i = 0; i < 8; ++i) a.shoulders[i] = s->pp.shoulders[i];
  a.first = t.first;
  if (s->swing) {  // the frame of this tick's fsteps: q_w's x, y, yaw
    double* fr = v.d(MPCQ_SV_FRAME);
    HIP_TRY(hipMemcpy2DAsync(fr, 24, a.q_w, 48, 16, B, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpy2DAsync(fr + 2, 24, a.q_w + 5, 48, 8, B, hipMemcpyDeviceToDevice, c->stream));
  }
  if (s->plant)  // the world pose the plant starts from
    HIP_TRY(hipMemcpyAsync(s->pv.ptr[PP_QW_PREV], a.q_w, B * 48, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(mpcq::launch_retrieve(c->N, a, c->stream));
  return MPCQ_OK;
}

// The rigid body under this tick's forces takes the place of the prediction.
int tick_plant(mpcq_session* s, const Tick& t) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->sv;
  mpcq::PlantArgs a{};
  a.batch = s->B;
  a.state = t.state; a.fsteps = v.d(MPCQ_SV_FSTEPS);
  a.f = s->channel ? s->hv.d(MPCQ_HV_F_CMD) : v.d(MPCQ_SV_F0);  // (tick_actuate has run)
  // a scenario's pushes ride on the user's wrench, its robots replace the table
  a.wrench = s->scenario && s->sc.pushes ? s->cv.d(MPCQ_CV_WRENCH) : s->pv.d(MPCQ_PV_WRENCH);
  a.robots = s->scenario && s->sc.robots ? (const mpcq_robot*)s->cv.ptr[MPCQ_CV_ROBOTS] : plant_table(s);
  mpcq_default_robot(&c->p, &a.dflt);
  a.state_out = s->pv.d(MPCQ_PV_STATE_END); a.f_eff = s->pv.d(MPCQ_PV_F_EFF);
  a.tail = 1;
  a.status = v.i(MPCQ_SV_STATUS); a.plan_status = v.i(SP_PLAN_STATUS); a.gait = v.d(MPCQ_SV_GAIT);
  a.q_w_prev = s->pv.d(PP_QW_PREV); a.q_w = v.d(MPCQ_SV_Q_W);
  a.next_state = v.d(MPCQ_SV_STATE); a.next_l_feet = v.d(MPCQ_SV_L_FEET);
  for (int i = 0; i < 8; ++i) a.shoulders[i] = s->pp.shoulders[i];
  HIP_TRY(mpcq::launch_plant(s->pl, a, c->stream));
  return MPCQ_OK;
}

// Whose episode ended with this tick, and the episodes' statistics.
int tick_monitor(mpcq_session* s, const Tick& t) {
  const Group &v = s->sv, &m = s->mv;
  mpcq::MonitorArgs a{};
  a.batch = s->B;
  a.q_w = v.d(MPCQ_SV_Q_W); a.status = v.i(MPCQ_SV_STATUS); a.iters = v.i(MPCQ_SV_ITERS); a.f0 = v.d(MPCQ_SV_F0);
  a.cost = v.d(MPCQ_SV_COST); a.state = v.d(MPCQ_SV_STATE); a.v_ref = t.v_ref;
  a.ep = m.d(MPCQ_MV_EP); a.ep_ticks = m.i(MPCQ_MV_EP_TICKS); a.episodes = m.i(MPCQ_MV_EPISODES);
  a.last = m.d(MPCQ_MV_LAST); a.done = m.i(MPCQ_MV_DONE); a.totals = (unsigned long long*)m.ptr[MPCQ_MV_TOTALS];
  a.trace = t.trace;
  HIP_TRY(mpcq::launch_monitor(s->mp, a, s->ctx->stream));
  return MPCQ_OK;
}

// The next solve's dispatch order (the retrieve has cleared every pending reset: by
// iteration counts alone).
int tick_order(mpcq_session* s) {
  const Group& v = s->sv;
  HIP_TRY(mpcq::launch_order(v.i(MPCQ_SV_ITERS), nullptr, s->B, v.i(MPCQ_SV_ORDER), s->ctx->stream));
  s->have_order = true;
  return MPCQ_OK;
}

// The tick's swing-foot references, substeps 0..k_mpc-1 (virtual-robot lift-off).
int tick_swing(mpcq_session* s) {
  const Group& v = s->sv;
  mpcq::SwingArgs a{};
  a.batch = s->B; a.k_sub0 = 0; a.n_sub = s->sp.k_mpc;
  a.gait = v.d(MPCQ_SV_GAIT); a.fsteps = v.d(MPCQ_SV_FSTEPS); a.frame = v.d(MPCQ_SV_FRAME);
  a.state = v.d(MPCQ_SV_SWING_STATE); a.ref = v.d(MPCQ_SV_SWING_REF);
  HIP_TRY(mpcq::launch_swing(s->sp, a, s->ctx->stream));
  return MPCQ_OK;
}

// One tick: its stages in stream order ([scenario] -> inputs -> [observe] -> [estimate] -> [disturb] -> planner (with [gait]
// between its first tick's footsteps-only pass and its main pass) -> solve ->
// retrieve -> [actuate -> plant] -> [monitor] -> order -> [swing] -> [auto-reset]).
int session_tick(mpcq_session* s, int k, const double* state, const double* l_feet, const double* v_ref,
                 const int32_t* reduced, uint32_t flags, double* trace) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!v_ref && !(s->scenario && s->sc.commands))
    return fail(MPCQ_E_INVALID, "v_ref is required (without a scenario that commands)");
  if (k < 0) return fail(MPCQ_E_INVALID, "k must be >= 0");
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  Tick t{};
  t.k = k;
  t.trace = trace;
  int rc = s->scenario ? tick_scenario(s, k) : MPCQ_OK;
  if (!rc) rc = tick_inputs(s, state, l_feet, v_ref, reduced, dev, t);
  if (!rc && !v_ref) t.v_ref = s->cv.d(MPCQ_CV_V_REF);
  if (!rc && s->channel) rc = tick_observe(s, t);
  if (!rc && s->estimator) rc = tick_estimate(s, t);
  if (!rc && s->disturb_on) rc = tick_disturb(s, t);
  if (!rc) rc = tick_plan(s, t);
  if (!rc) rc = tick_solve(s, t);
  if (!rc) rc = tick_retrieve(s, t);
  if (!rc && s->plant && s->channel) rc = tick_actuate(s);
  if (!rc && s->plant) rc = tick_plant(s, t);
  if (!rc && s->monitor) rc = tick_monitor(s, t);
  if (!rc) rc = tick_order(s);
  if (!rc && s->swing) rc = tick_swing(s);
  if (rc) return rc;
  // auto-reset, last: the swing launch above has read the tick's gait and fsteps
  if (s->monitor && s->mp.auto_reset) HIP_TRY(enqueue_reset(s, s->mv.i(MPCQ_MV_DONE), nullptr, nullptr, true));
  // host inputs are staged in buffers the next tick reuses: host calls block
  if (!(flags & MPCQ_FLAG_ASYNC) || !dev) HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

}  // namespace

extern "C" {

int mpcq_session_tick(mpcq_session* s, int k, const double* state, const double* l_feet, const double* v_ref,
                      const int32_t* reduced, uint32_t flags) {
  return session_tick(s, k, state, l_feet, v_ref, reduced, flags, nullptr);
}

int mpcq_session_run(mpcq_session* s, int k0, int n_ticks, const double* v_ref, int v_ref_ticks, double* trace,
                     uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!(flags & MPCQ_FLAG_DEVICE_PTRS)) return fail(MPCQ_E_INVALID, "mpcq_session_run needs MPCQ_FLAG_DEVICE_PTRS");
  if (!v_ref && !(s->scenario && s->sc.commands))
    return fail(MPCQ_E_INVALID, "v_ref is required (without a scenario that commands)");
  if (v_ref && v_ref_ticks < 1) return fail(MPCQ_E_INVALID, "v_ref [v_ref_ticks][B][6] needs v_ref_ticks >= 1");
  if (k0 < 0 || n_ticks < 1) return fail(MPCQ_E_INVALID, "need k0 >= 0 and n_ticks >= 1");
  if (k0 > INT32_MAX - n_ticks) return fail(MPCQ_E_INVALID, "k0 + n_ticks overflows");
  if (trace && !s->monitor) return fail(MPCQ_E_INVALID, "a trace needs mpcq_session_enable_monitor");
  const size_t B = (size_t)s->B;
  for (int t = 0; t < n_ticks; ++t) {
    const int row = t < v_ref_ticks ? t : v_ref_ticks - 1;
    const int rc = session_tick(s, k0 + t, nullptr, nullptr, v_ref ? v_ref + (size_t)row * B * 6 : nullptr, nullptr,
                                MPCQ_FLAG_DEVICE_PTRS | MPCQ_FLAG_ASYNC,
                                trace ? trace + (size_t)t * B * MPCQ_TRACE : nullptr);
    if (rc) {
      (void)hipStreamSynchronize(s->ctx->stream);
      return rc;
    }
  }
  if (!(flags & MPCQ_FLAG_ASYNC)) {
    DeviceGuard g(s->ctx->device);
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  }
  return MPCQ_OK;
}

int mpcq_session_reset(mpcq_session* s, const int32_t* mask, const double* gait0, const double* q_w0,
                       uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  hipError_t e = hipSuccess;
  mask = staged(s, dev, mask, SP_IN_REDUCED, &e);
  gait0 = staged(s, dev, gait0, SP_IN_GAIT, &e);
  q_w0 = staged(s, dev, q_w0, SP_IN_VREF, &e);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    return fail(MPCQ_E_DEVICE, "staging the reset's inputs failed");
  }
  e = enqueue_reset(s, mask, gait0, q_w0, true);
  if (!(flags & MPCQ_FLAG_ASYNC) || !dev) {
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
  }
  HIP_TRY(e);
  return MPCQ_OK;
}

int mpcq_session_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, &mpcq_session::sv, what, dst, flags);
}

int mpcq_session_plant_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, &mpcq_session::pv, what, dst, flags);
}

int mpcq_session_monitor_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, &mpcq_session::mv, what, dst, flags);
}

int mpcq_session_scenario_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, &mpcq_session::cv, what, dst, flags);
}

int mpcq_session_channel_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, &mpcq_session::hv, what, dst, flags);
}

int mpcq_session_estimator_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, &mpcq_session::ev, what, dst, flags);
}

int mpcq_session_disturb_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, &mpcq_session::dv, what, dst, flags);
}

int mpcq_session_gait_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, &mpcq_session::gv, what, dst, flags);
}

int mpcq_session_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, &mpcq_session::sv, what, out);
}

int mpcq_session_plant_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, &mpcq_session::pv, what, out);
}

int mpcq_session_monitor_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, &mpcq_session::mv, what, out);
}

int mpcq_session_scenario_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, &mpcq_session::cv, what, out);
}

int mpcq_session_channel_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, &mpcq_session::hv, what, out);
}

int mpcq_session_estimator_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, &mpcq_session::ev, what, out);
}

int mpcq_session_disturb_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, &mpcq_session::dv, what, out);
}

int mpcq_session_gait_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, &mpcq_session::gv, what, out);
}

int mpcq_session_write(mpcq_session* s, int what, const void* src, uint32_t flags) {
  if (!s || !src) return fail(MPCQ_E_INVALID, "NULL argument");
  const int rc = find(s->sv, what);
  if (rc) return rc;
  // the engine indexes robots through the order: only order_kernel writes it
  if (what == MPCQ_SV_ORDER) return fail(MPCQ_E_INVALID, "MPCQ_SV_ORDER is read-only");
  // only mpcq_session_reset sets it (with the state a first tick needs), only the retrieve clears it
  if (what == MPCQ_SV_FIRST) return fail(MPCQ_E_INVALID, "MPCQ_SV_FIRST is read-only");
  if (what == MPCQ_SV_SWING_REF || what == MPCQ_SV_FRAME)
    return fail(MPCQ_E_INVALID, "MPCQ_SV_SWING_REF and MPCQ_SV_FRAME are read-only");
  DeviceGuard g(s->ctx->device);
  const hipMemcpyKind kind = (flags & MPCQ_FLAG_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(hipMemcpyAsync(s->sv.ptr[what], src, s->sv.bytes[what], kind, s->ctx->stream));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  return MPCQ_OK;
}

}  // extern "C"

// ---- snapshots: save, restore and branch robots on the device (include/mpcq.h) ------------

namespace {

// The parts of a snapshot, in the blob's order; each is one allocation (alloc_group).
enum { G_MAIN, G_SWING, G_PLANT, G_MONITOR, G_SCENARIO, G_ROBOTS, G_PLANT_ROBOTS, G_CHANNEL, G_ESTIMATOR,
       G_GAIT, G_DISTURB, G_COUNT };
const char* const kPartName[G_COUNT] = {"the snapshot's session arrays", "the snapshot's swing arrays",
                                        "the snapshot's plant arrays", "the snapshot's monitor arrays",
                                        "the snapshot's scenario arrays", "the snapshot's robots table",
                                        "the snapshot's plant robots table", "the snapshot's channel arrays",
                                        "the snapshot's estimator row", "the snapshot's gait rows",
                                        "the snapshot's disturb rows"};

// What a snapshot's allocations follow from, with the context's N.
struct SnapShape {
  int64_t B = 0;
  int k_mpc = 0;  // 0: no swing arrays
  bool pv = false, mv = false, cv = false, robots = false, plant_robots = false;
  bool hv = false;              // the channel arrays, primed under
  int delay = 0, latency = 0;   // these depths
  bool ev = false;              // the estimator's row (self-describing: no parameter travels)
  bool gv = false;              // the gait stage's rows, indices into a library of
  int n_gaits = 0;              // this many cycles (the library itself is configuration: not held)
  bool dv = false;              // the disturbance stage's row (self-describing, as the estimator's)
};

}  // namespace

struct mpcq_snapshot {
  mpcq_ctx* ctx = nullptr;
  bool saved = false;
  SnapShape sh;
  Group g[G_COUNT];         // ptr / bytes by the part's own array ids; mem null: the part is absent
  bool have_order = false;  // a tick had run since create
  bool resets = false;      // mpcq_session_reset had been called
};

namespace {

SnapShape shape_of(const mpcq_session* s) {
  SnapShape sh;
  sh.B = s->B;
  sh.k_mpc = s->swing ? s->sp.k_mpc : 0;
  sh.pv = s->pv.mem; sh.mv = s->mv.mem; sh.cv = s->cv.mem;
  sh.robots = s->robots.count > 0; sh.plant_robots = s->plant_robots.count > 0;
  sh.hv = s->hv.mem;
  if (sh.hv) { sh.delay = s->ch.delay; sh.latency = s->ch.latency; }
  sh.ev = s->ev.mem;
  sh.gv = s->gv.mem;
  if (sh.gv) sh.n_gaits = s->gp.n_gaits;
  sh.dv = s->dv.mem;
  return sh;
}

// The main group's arrays a snapshot holds: not the staging of host inputs (every tick
// rewrites it before reading), not MPCQ_SV_ORDER (a permutation: rebuilt, never copied by
// rows), not the swing slots (a part of their own).
bool main_held(int w) {
  return w != MPCQ_SV_ORDER && w != MPCQ_SV_SWING_REF && w != MPCQ_SV_SWING_STATE && w != MPCQ_SV_FRAME &&
         w != SP_IN_STATE && w != SP_IN_LFEET && w != SP_IN_VREF && w != SP_IN_REDUCED && w != SP_IN_GAIT;
}

// Bytes of every array of every part of a snapshot of this shape (0: not held).
void snap_sizes(const SnapShape& sh, int N, size_t nb[G_COUNT][SP_COUNT]) {
  const size_t B = (size_t)sh.B;
  memset(nb, 0, sizeof(size_t) * G_COUNT * SP_COUNT);
  for (int w = 0; w < SP_COUNT; ++w)
    if (main_held(w)) nb[G_MAIN][w] = sv_bytes(w, sh.B, N);
  if (sh.k_mpc > 0) swing_bytes(B, sh.k_mpc, nb[G_SWING]);
  if (sh.pv) {
    plant_bytes(B, nb[G_PLANT]);
    nb[G_PLANT][PP_QW_PREV] = 0;  // (a tick with the plant takes it before its retrieve)
  }
  if (sh.mv) monitor_bytes(B, nb[G_MONITOR]);
  if (sh.cv) scenario_bytes(B, nb[G_SCENARIO]);
  if (sh.robots) nb[G_ROBOTS][0] = B * sizeof(mpcq_robot);
  if (sh.plant_robots) nb[G_PLANT_ROBOTS][0] = B * sizeof(mpcq_robot);
  if (sh.hv) channel_bytes(B, nb[G_CHANNEL]);
  if (sh.ev) {
    estimator_bytes(B, nb[G_ESTIMATOR]);
    nb[G_ESTIMATOR][MPCQ_EV_EST] = 0;  // (derived: every tick rewrites it before anything reads it)
  }
  if (sh.gv) nb[G_GAIT][MPCQ_GV_STATE] = B * 16;
  if (sh.dv) nb[G_DISTURB][MPCQ_DV_ROW] = B * MPCQ_DIST_ROW * 8;  // (MPCQ_DV_DIST, _RESID: derived)
}

// The session's arrays seen as a snapshot's parts (the arrays a snapshot does not hold: null).
void session_parts(const mpcq_session* s, Group out[G_COUNT]) {
  for (int w = 0; w < SP_COUNT; ++w)
    if (main_held(w)) { out[G_MAIN].ptr[w] = s->sv.ptr[w]; out[G_MAIN].bytes[w] = s->sv.bytes[w]; }
  if (s->swing)
    for (int i = 0; i < 3; ++i) {
      out[G_SWING].ptr[i] = s->sv.ptr[MPCQ_SV_SWING_REF + i]; out[G_SWING].bytes[i] = s->sv.bytes[MPCQ_SV_SWING_REF + i];
    }
  if (s->pv.mem)
    for (int w = 0; w < MPCQ_PV_COUNT; ++w) { out[G_PLANT].ptr[w] = s->pv.ptr[w]; out[G_PLANT].bytes[w] = s->pv.bytes[w]; }
  if (s->mv.mem)
    for (int w = 0; w < MPCQ_MV_COUNT; ++w) { out[G_MONITOR].ptr[w] = s->mv.ptr[w]; out[G_MONITOR].bytes[w] = s->mv.bytes[w]; }
  if (s->cv.mem)
    for (int w = 0; w < MPCQ_CV_COUNT; ++w) { out[G_SCENARIO].ptr[w] = s->cv.ptr[w]; out[G_SCENARIO].bytes[w] = s->cv.bytes[w]; }
  const size_t tb = (size_t)s->B * sizeof(mpcq_robot);
  if (s->robots.count > 0) { out[G_ROBOTS].ptr[0] = s->robots.dev; out[G_ROBOTS].bytes[0] = tb; }
  if (s->plant_robots.count > 0) { out[G_PLANT_ROBOTS].ptr[0] = s->plant_robots.dev; out[G_PLANT_ROBOTS].bytes[0] = tb; }
  if (s->hv.mem)
    for (int w = 0; w < MPCQ_HV_COUNT; ++w) { out[G_CHANNEL].ptr[w] = s->hv.ptr[w]; out[G_CHANNEL].bytes[w] = s->hv.bytes[w]; }
  if (s->ev.mem) { out[G_ESTIMATOR].ptr[MPCQ_EV_ROW] = s->ev.ptr[MPCQ_EV_ROW]; out[G_ESTIMATOR].bytes[MPCQ_EV_ROW] = s->ev.bytes[MPCQ_EV_ROW]; }
  if (s->gv.mem) { out[G_GAIT].ptr[MPCQ_GV_STATE] = s->gv.ptr[MPCQ_GV_STATE]; out[G_GAIT].bytes[MPCQ_GV_STATE] = s->gv.bytes[MPCQ_GV_STATE]; }
  if (s->dv.mem) { out[G_DISTURB].ptr[MPCQ_DV_ROW] = s->dv.ptr[MPCQ_DV_ROW]; out[G_DISTURB].bytes[MPCQ_DV_ROW] = s->dv.bytes[MPCQ_DV_ROW]; }
}

// One array of a snapshot (a) next to its counterpart (b; null without one), in the blob's order.
struct SnapItem {
  void *a, *b;
  size_t bytes_a, bytes_b;
  bool rows;  // per-robot rows (all but MPCQ_MV_TOTALS)
};

// The listing's bound, a constant of its own: every array of every part (51 with every group
// enabled, MPCQ_MV_TOTALS among them, which is listed and never gathered).  A restore gathers
// them kGatherMax to a launch.
constexpr int kListMax = 64;
constexpr int kGatherChunks = (kListMax + mpcq::kGatherMax - 1) / mpcq::kGatherMax;

// The table save, restore, fork, export and import all walk: every array parts `a` hold, with
// the same array of parts `b` (null: none).  An array `a` holds and `b` lacks is an error (-1).
int list_arrays(const Group a[G_COUNT], const Group* b, SnapItem out[kListMax]) {
  int n = 0;
  for (int gi = 0; gi < G_COUNT; ++gi)
    for (int w = 0; w < SP_COUNT; ++w) {
      if (!a[gi].ptr[w]) continue;
      if (n == kListMax || (b && !b[gi].ptr[w])) return -1;
      out[n++] = SnapItem{a[gi].ptr[w], b ? b[gi].ptr[w] : nullptr, a[gi].bytes[w], b ? b[gi].bytes[w] : 0,
                          !(gi == G_MONITOR && w == MPCQ_MV_TOTALS)};
    }
  return n;
}

void free_parts(mpcq_snapshot* p) {
  for (int gi = 0; gi < G_COUNT; ++gi) {
    if (p->g[gi].mem) (void)hipFree(p->g[gi].mem);
    p->g[gi] = Group{};
  }
  p->saved = false;
}

// The allocations of a snapshot of this shape into *p (which holds none): all or nothing.
int alloc_parts(mpcq_ctx* c, const SnapShape& sh, mpcq_snapshot* p) {
  size_t nb[G_COUNT][SP_COUNT];
  snap_sizes(sh, c->N, nb);
  for (int gi = 0; gi < G_COUNT; ++gi) {
    size_t tot = 0;
    for (int w = 0; w < SP_COUNT; ++w) tot += nb[gi][w];
    if (!tot) continue;
    const int rc = alloc_group(c, kPartName[gi], SP_COUNT, nb[gi], &p->g[gi].mem, p->g[gi].ptr, p->g[gi].bytes);
    if (rc) {
      free_parts(p);
      return rc;
    }
  }
  p->ctx = c;
  p->sh = sh;
  return MPCQ_OK;
}

// The first difference between a snapshot's shape and a session's, as text; or null.
const char* shape_difference(const SnapShape& a, const SnapShape& b, bool batch_too) {
  if (batch_too && a.B != b.B) return "the batch sizes differ (a restore without a map needs the same batch)";
  if ((a.k_mpc > 0) != (b.k_mpc > 0)) return "the swing arrays exist on one side only";
  if (a.k_mpc != b.k_mpc) return "the swing k_mpc differs";
  if (a.pv != b.pv) return "the plant arrays exist on one side only";
  if (a.mv != b.mv) return "the monitor arrays exist on one side only";
  if (a.cv != b.cv) return "the scenario arrays exist on one side only";
  if (a.robots != b.robots) return "the robots table is in force on one side only";
  if (a.plant_robots != b.plant_robots) return "the plant robots table is in force on one side only";
  if (a.hv != b.hv) return "the channel arrays exist on one side only";
  if (a.delay != b.delay) return "the channel's delay differs (the rings were filled under another)";
  if (a.latency != b.latency) return "the channel's latency differs (the rings were filled under another)";
  if (a.ev != b.ev) return "the estimator arrays exist on one side only";
  if (a.gv != b.gv) return "the gait arrays exist on one side only";
  if (a.n_gaits != b.n_gaits) return "the gait library sizes differ (the rows index another library)";
  if (a.dv != b.dv) return "the disturb arrays exist on one side only";
  return nullptr;
}

// A host map: every entry -1 or in [0, rows_src); with `full`, no -1 either.
int check_host_map(const int32_t* map, int64_t n, int64_t rows_src, bool full) {
  for (int64_t b = 0; b < n; ++b) {
    if (map[b] < -1 || map[b] >= rows_src)
      return fail(MPCQ_E_INVALID, "map[%lld] = %d is neither -1 nor a row of the snapshot (0..%lld)", (long long)b,
                  map[b], (long long)rows_src - 1);
    if (full && map[b] == -1)
      return fail(MPCQ_E_INVALID, "map[%lld] = -1: restoring ticked state into a session that has not ticked yet "
                  "must cover every robot", (long long)b);
  }
  return MPCQ_OK;
}

// The launch's table from the arrays: the wide ones first, by access width, then the narrow ones.
int gather_table(const SnapItem* it, int n, int64_t rows_src, int64_t rows_dst, mpcq::GatherArgs* a) {
  a->n = 0;
  const int widths[4] = {16, 8, 4, 0};  // the passes: wide by width, then narrow
  for (int pass = 0; pass < 4; ++pass) {
    for (int i = 0; i < n; ++i) {
      if (!it[i].rows) continue;
      const int64_t rb = (int64_t)(it[i].bytes_a / (size_t)rows_src);
      if (rb < 4 || rb > INT32_MAX || (size_t)rb * (size_t)rows_src != it[i].bytes_a ||
          (size_t)rb * (size_t)rows_dst != it[i].bytes_b)
        return fail(MPCQ_E_INVALID, "array %d: %zu bytes for %lld rows against %zu bytes for %lld rows", i,
                    it[i].bytes_a, (long long)rows_src, it[i].bytes_b, (long long)rows_dst);
      const int vec = mpcq::gather_vec(it[i].a, it[i].b, rb);
      if (!vec) return fail(MPCQ_E_INVALID, "array %d: rows of %lld bytes at %p / %p are not 4-byte aligned", i,
                            (long long)rb, it[i].a, it[i].b);
      if (rb > mpcq::kGatherNarrow ? vec != widths[pass] : pass != 3) continue;
      if (a->n == mpcq::kGatherMax) return fail(MPCQ_E_INVALID, "more than %d arrays", mpcq::kGatherMax);
      a->d[a->n++] = mpcq::GatherDesc{it[i].a, it[i].b, (int32_t)rb, vec};
    }
    if (pass == 0) a->n_wide16 = a->n;
    if (pass == 1) a->n_wide8 = a->n;
    if (pass == 2) a->n_wide = a->n;
  }
  a->rows_src = rows_src;
  a->rows_dst = rows_dst;
  return MPCQ_OK;
}

int snapshot_save(mpcq_session* s, mpcq_snapshot* p, uint32_t flags) {
  mpcq_ctx* c = s->ctx;
  if (p->ctx != c) return fail(MPCQ_E_INVALID, "the snapshot belongs to another context");
  DeviceGuard dg(c->device);
  const SnapShape sh = shape_of(s);
  if (!p->g[G_MAIN].mem || shape_difference(p->sh, sh, true)) {  // the new allocations first
    mpcq_snapshot fresh;
    const int rc = alloc_parts(c, sh, &fresh);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // a queued restore may still read the old ones
    free_parts(p);
    for (int gi = 0; gi < G_COUNT; ++gi) p->g[gi] = fresh.g[gi];
    p->sh = sh;
  }
  Group live[G_COUNT];
  session_parts(s, live);
  SnapItem it[kListMax];
  const int n = list_arrays(p->g, live, it);
  if (n < 0) return fail(MPCQ_E_DEVICE, "the snapshot's arrays do not match the session's");
  for (int i = 0; i < n; ++i)
    if (it[i].bytes_a != it[i].bytes_b)
      return fail(MPCQ_E_DEVICE, "the snapshot's array %d has %zu bytes, the session's %zu", i, it[i].bytes_a, it[i].bytes_b);
  p->saved = false;
  for (int i = 0; i < n; ++i)
    HIP_TRY(hipMemcpyAsync(it[i].a, it[i].b, it[i].bytes_a, hipMemcpyDeviceToDevice, c->stream));
  p->have_order = s->have_order;
  p->resets = s->resets;
  p->saved = true;
  if (!(flags & MPCQ_FLAG_ASYNC)) HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

int snapshot_restore(mpcq_session* s, const mpcq_snapshot* p, const int32_t* map, uint32_t flags) {
  mpcq_ctx* c = s->ctx;
  if (!p->saved) return fail(MPCQ_E_INVALID, "the snapshot holds nothing: save into it first");
  if (p->ctx != c) return fail(MPCQ_E_INVALID, "the snapshot belongs to another context");
  const char* diff = shape_difference(p->sh, shape_of(s), !map);
  if (diff) return fail(MPCQ_E_INVALID, "the snapshot's shape is not the session's: %s", diff);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  // ticked state into a session that has not ticked: a robot left out would run a warm tick on
  // creation state
  const bool full = p->have_order && !s->have_order;
  if (map && dev && full)
    return fail(MPCQ_E_INVALID, "restoring ticked state into a session that has not ticked yet needs a host map "
                "(it must cover every robot)");
  if (map && !dev) {
    const int rc = check_host_map(map, s->B, p->sh.B, full);
    if (rc) return rc;
  }
  Group live[G_COUNT];
  session_parts(s, live);
  SnapItem it[kListMax];
  const int n = list_arrays(p->g, live, it);
  if (n < 0) return fail(MPCQ_E_INVALID, "the snapshot's arrays do not match the session's");
  // the per-robot arrays, kGatherMax to a launch (one launch up to 48 arrays); every launch's
  // table is made before the first is enqueued
  int nr = 0;
  for (int i = 0; i < n; ++i)
    if (it[i].rows) it[nr++] = it[i];
  const int chunks = (nr + mpcq::kGatherMax - 1) / mpcq::kGatherMax;
  mpcq::GatherArgs ga[kGatherChunks] = {};
  for (int ch = 0; ch < chunks; ++ch) {
    const int lo = ch * mpcq::kGatherMax, cnt = nr - lo < mpcq::kGatherMax ? nr - lo : mpcq::kGatherMax;
    const int rc = gather_table(it + lo, cnt, p->sh.B, s->B, &ga[ch]);
    if (rc) return rc;
  }
  DeviceGuard dg(c->device);
  hipError_t e = hipSuccess;
  const int32_t* dmap = staged(s, dev, map, SP_IN_REDUCED, &e);
  for (int ch = 0; ch < chunks && e == hipSuccess; ++ch) {
    ga[ch].map = dmap;
    // creation state, which only a first tick may consume: the rows come with a pending reset
    ga[ch].first = p->have_order ? nullptr : s->sv.i(MPCQ_SV_FIRST);
    e = mpcq::launch_gather_rows(ga[ch], c->stream);
  }
  if (e == hipSuccess && !map && p->sh.mv)  // the batch-wide totals go with the whole batch only
    e = hipMemcpyAsync(s->mv.ptr[MPCQ_MV_TOTALS], p->g[G_MONITOR].ptr[MPCQ_MV_TOTALS], s->mv.bytes[MPCQ_MV_TOTALS],
                       hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) {
    if (!p->have_order || p->resets) s->resets = true;
    if (s->have_order || p->have_order) {  // as enqueue_reset: the pending resets to the front
      e = mpcq::launch_order(s->sv.i(MPCQ_SV_ITERS), s->resets ? s->sv.i(MPCQ_SV_FIRST) : nullptr, s->B,
                             s->sv.i(MPCQ_SV_ORDER), c->stream);
      s->have_order = true;
    }
  }
  if (!(flags & MPCQ_FLAG_ASYNC) || (map && !dev)) {
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
  }
  HIP_TRY(e);
  return MPCQ_OK;
}

// The blob's header (include/mpcq.h, mpcq_session_snapshot_export).
struct BlobHeader {
  char magic[8];
  uint32_t version;
  int32_t N;
  int64_t B;
  int32_t k_mpc;
  uint32_t flags;
  int64_t group_bytes[G_CHANNEL];  // the seven parts of format version 1
  int64_t total;
  int64_t user;
  int64_t channel_bytes;   // format version 2: the eighth part,
  int32_t delay, latency;  // and the depths its rings were filled under
  int64_t estimator_bytes; // format version 3: the ninth part
  // format version 4 only, behind the 128 bytes of versions 1 to 3: the tenth part and the size
  // of the library its rows index
  int64_t gait_bytes;
  int32_t n_gaits, pad;
  // format version 5 only, behind the 144 bytes of version 4: the eleventh part
  int64_t disturb_bytes;
  int64_t pad5;
};
static_assert(sizeof(BlobHeader) == 160 && offsetof(BlobHeader, gait_bytes) == 128 &&
                  offsetof(BlobHeader, disturb_bytes) == 144 && G_CHANNEL == 7 && G_ESTIMATOR == 8 && G_GAIT == 9 &&
                  G_DISTURB == 10 && G_COUNT == 11,
              "the blob's header is 128 bytes, 144 in format version 4, 160 from version 5 on");
size_t header_bytes(uint32_t version) {
  return version >= 5 ? sizeof(BlobHeader) : version == 4 ? offsetof(BlobHeader, disturb_bytes)
                                                          : offsetof(BlobHeader, gait_bytes);
}

// The header's byte count of part gi.
int64_t& part_bytes(BlobHeader& h, int gi) {
  return gi == G_DISTURB ? h.disturb_bytes : gi == G_GAIT ? h.gait_bytes : gi == G_ESTIMATOR ? h.estimator_bytes : gi == G_CHANNEL ? h.channel_bytes
                                                                                                : h.group_bytes[gi];
}
const char kMagic[8] = {'M', 'P', 'C', 'Q', 'S', 'N', 'P', '1'};

void blob_header(const SnapShape& sh, int N, bool have_order, bool resets, BlobHeader* h) {
  size_t nb[G_COUNT][SP_COUNT];
  snap_sizes(sh, N, nb);
  memset(h, 0, sizeof(*h));
  memcpy(h->magic, kMagic, 8);
  h->version = sh.dv ? 5 : sh.gv ? 4 : sh.ev ? 3 : sh.hv ? 2 : 1; h->N = N; h->B = sh.B; h->k_mpc = sh.k_mpc;
  h->flags = (have_order ? 1u : 0u) | (resets ? 2u : 0u) | (sh.k_mpc > 0 ? 4u : 0u) | (sh.pv ? 8u : 0u) |
             (sh.mv ? 16u : 0u) | (sh.cv ? 32u : 0u) | (sh.robots ? 64u : 0u) | (sh.plant_robots ? 128u : 0u) |
             (sh.hv ? 256u : 0u) | (sh.ev ? 512u : 0u) | (sh.gv ? 1024u : 0u) | (sh.dv ? 2048u : 0u);
  h->delay = sh.delay; h->latency = sh.latency;
  h->n_gaits = sh.n_gaits;
  h->total = (int64_t)header_bytes(h->version);
  for (int gi = 0; gi < G_COUNT; ++gi) {
    int64_t& gb = part_bytes(*h, gi);
    for (int w = 0; w < SP_COUNT; ++w) gb += (int64_t)nb[gi][w];
    h->total += gb;
  }
}

}  // namespace

extern "C" {

int mpcq_session_snapshot_create(mpcq_session* s, mpcq_snapshot** out) {
  if (!out) return fail(MPCQ_E_INVALID, "out is NULL");
  *out = nullptr;
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_snapshot* p = new mpcq_snapshot();
  p->ctx = s->ctx;
  *out = p;
  return MPCQ_OK;
}

int mpcq_session_snapshot_destroy(mpcq_snapshot* p) {
  if (!p) return MPCQ_OK;
  if (p->g[G_MAIN].mem) {
    DeviceGuard g(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    free_parts(p);
  }
  delete p;
  return MPCQ_OK;
}

int mpcq_session_snapshot_save(mpcq_session* s, mpcq_snapshot* p, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!p) return fail(MPCQ_E_INVALID, "snapshot is NULL");
  return snapshot_save(s, p, flags);
}

int mpcq_session_snapshot_restore(mpcq_session* s, const mpcq_snapshot* p, const int32_t* map, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!p) return fail(MPCQ_E_INVALID, "snapshot is NULL");
  return snapshot_restore(s, p, map, flags);
}

int mpcq_session_fork(mpcq_session* s, const int32_t* map, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!map) return fail(MPCQ_E_INVALID, "map is NULL (a fork needs one)");
  if (!(flags & MPCQ_FLAG_DEVICE_PTRS)) {  // before anything is launched
    const int rc = check_host_map(map, s->B, s->B, false);
    if (rc) return rc;
  }
  if (!s->fork_snap) {
    const int rc = mpcq_session_snapshot_create(s, &s->fork_snap);
    if (rc) return rc;
  }
  const int rc = snapshot_save(s, s->fork_snap, MPCQ_FLAG_ASYNC);
  if (rc) return rc;
  return snapshot_restore(s, s->fork_snap, map, flags);
}

int mpcq_session_snapshot_bytes(const mpcq_snapshot* p, int64_t* bytes) {
  if (!p || !bytes) return fail(MPCQ_E_INVALID, "NULL argument");
  if (!p->saved) return fail(MPCQ_E_INVALID, "the snapshot holds nothing: save into it first");
  BlobHeader h;
  blob_header(p->sh, p->ctx->N, p->have_order, p->resets, &h);
  *bytes = h.total;
  return MPCQ_OK;
}

int mpcq_session_snapshot_export(const mpcq_snapshot* p, void* dst, int64_t bytes) {
  if (!p || !dst) return fail(MPCQ_E_INVALID, "NULL argument");
  if (!p->saved) return fail(MPCQ_E_INVALID, "the snapshot holds nothing: save into it first");
  BlobHeader h;
  blob_header(p->sh, p->ctx->N, p->have_order, p->resets, &h);
  if (bytes != h.total) return fail(MPCQ_E_INVALID, "the blob has %lld bytes, dst %lld", (long long)h.total, (long long)bytes);
  SnapItem it[kListMax];
  const int n = list_arrays(p->g, nullptr, it);
  if (n < 0) return fail(MPCQ_E_DEVICE, "the snapshot holds more than %d arrays", kListMax);
  mpcq_ctx* c = p->ctx;
  DeviceGuard dg(c->device);
  memcpy(dst, &h, header_bytes(h.version));
  size_t off = header_bytes(h.version);
  hipError_t e = hipSuccess;
  for (int i = 0; i < n && e == hipSuccess; ++i) {
    e = hipMemcpyAsync((char*)dst + off, it[i].a, it[i].bytes_a, hipMemcpyDeviceToHost, c->stream);
    off += it[i].bytes_a;
  }
  const hipError_t es = hipStreamSynchronize(c->stream);
  HIP_TRY(e);
  HIP_TRY(es);
  if ((int64_t)off != h.total) return fail(MPCQ_E_DEVICE, "wrote %zu of %lld bytes", off, (long long)h.total);
  return MPCQ_OK;
}

int mpcq_session_snapshot_import(mpcq_session* s, mpcq_snapshot* p, const void* src, int64_t bytes) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!p || !src) return fail(MPCQ_E_INVALID, "NULL argument");
  mpcq_ctx* c = s->ctx;
  if (p->ctx != c) return fail(MPCQ_E_INVALID, "the snapshot belongs to another context");
  BlobHeader h;
  memset(&h, 0, sizeof(h));
  if (bytes < (int64_t)header_bytes(1)) return fail(MPCQ_E_INVALID, "%lld bytes are less than a header", (long long)bytes);
  memcpy(&h, src, header_bytes(1));
  if (memcmp(h.magic, kMagic, 8) != 0) return fail(MPCQ_E_INVALID, "not a snapshot blob (magic)");
  if (h.version < 1 || h.version > 5)
    return fail(MPCQ_E_INVALID, "blob format version %u, this library reads 1 to 5", h.version);
  if (bytes < (int64_t)header_bytes(h.version))
    return fail(MPCQ_E_INVALID, "%lld bytes are less than a version-%u header", (long long)bytes, h.version);
  memcpy(&h, src, header_bytes(h.version));
  if (h.N != c->N) return fail(MPCQ_E_INVALID, "the blob is of a context with N = %d, this one has N = %d", h.N, c->N);
  const bool chan = h.flags & 256u, est = h.flags & 512u, gait = h.flags & 1024u, dist = h.flags & 2048u;
  if (h.B < 1 || h.B > (int64_t)0x7fffffff || h.k_mpc < 0 || h.k_mpc > 65536 || (h.flags >> 12) ||
      ((h.flags & 4u) != 0) != (h.k_mpc > 0) || h.version != (dist ? 5u : gait ? 4u : est ? 3u : chan ? 2u : 1u) ||
      (!est && h.estimator_bytes != 0) || (gait && (h.n_gaits < 1 || h.n_gaits > MPCQ_GAIT_MAX || h.pad != 0)) ||
      (!gait && (h.n_gaits != 0 || h.pad != 0)) || h.pad5 != 0 ||
      (chan ? h.delay < 0 || h.delay > MPCQ_CHANNEL_MAX_DELAY || h.latency < 0 || h.latency > MPCQ_CHANNEL_MAX_LATENCY
            : h.delay != 0 || h.latency != 0 || h.channel_bytes != 0))
    return fail(MPCQ_E_INVALID, "the blob's header is inconsistent (B %lld, k_mpc %d, flags %#x)", (long long)h.B,
                h.k_mpc, h.flags);
  SnapShape sh;
  sh.B = h.B; sh.k_mpc = h.k_mpc;
  sh.pv = h.flags & 8u; sh.mv = h.flags & 16u; sh.cv = h.flags & 32u;
  sh.robots = h.flags & 64u; sh.plant_robots = h.flags & 128u;
  sh.hv = chan; sh.delay = h.delay; sh.latency = h.latency;
  sh.ev = est;
  sh.gv = gait; sh.n_gaits = gait ? h.n_gaits : 0;
  sh.dv = dist;
  BlobHeader want;
  blob_header(sh, c->N, h.flags & 1u, h.flags & 2u, &want);
  for (int gi = 0; gi < G_COUNT; ++gi) {
    const int64_t have = part_bytes(h, gi), need = part_bytes(want, gi);
    if (have != need)
      return fail(MPCQ_E_INVALID, "the blob's part %d has %lld bytes, its shape says %lld", gi, (long long)have,
                  (long long)need);
  }
  if (h.total != want.total || bytes != want.total)
    return fail(MPCQ_E_INVALID, "the blob says %lld bytes, its shape %lld, the caller %lld (truncated?)",
                (long long)h.total, (long long)want.total, (long long)bytes);
  DeviceGuard dg(c->device);
  mpcq_snapshot fresh;
  int rc = alloc_parts(c, sh, &fresh);
  if (rc) return rc;
  SnapItem it[kListMax];
  const int n = list_arrays(fresh.g, nullptr, it);
  size_t off = header_bytes(h.version);
  hipError_t e = n < 0 ? hipErrorInvalidValue : hipSuccess;
  for (int i = 0; i < n && e == hipSuccess; ++i) {
    e = hipMemcpyAsync(it[i].a, (const char*)src + off, it[i].bytes_a, hipMemcpyHostToDevice, c->stream);
    off += it[i].bytes_a;
  }
  const hipError_t es = hipStreamSynchronize(c->stream);  // (also: a queued restore may still read p's arrays)
  if (e != hipSuccess || es != hipSuccess) {
    free_parts(&fresh);
    return fail(MPCQ_E_DEVICE, "copying the blob to the device failed");
  }
  free_parts(p);
  for (int gi = 0; gi < G_COUNT; ++gi) p->g[gi] = fresh.g[gi];
  p->sh = sh;
  p->have_order = h.flags & 1u;
  p->resets = h.flags & 2u;
  p->saved = true;
  return MPCQ_OK;
}

int mpcq_debug_gather_rows(mpcq_ctx* c, int n, const void* const* src, void* const* dst, const int64_t* row_bytes,
                           int64_t rows_src, int64_t rows_dst, const int32_t* map, uint32_t flags) {
  int rc = check_ctx(c, rows_dst);
  if (!rc) rc = check_ctx(c, rows_src);
  if (rc) return rc;
  if (n < 1 || n > mpcq::kGatherMax || !src || !dst || !row_bytes)
    return fail(MPCQ_E_INVALID, "1..%d arrays and their three tables are required", mpcq::kGatherMax);
  for (int i = 0; i < n; ++i)
    if (!src[i] || !dst[i] || row_bytes[i] < 4 || row_bytes[i] % 4 || row_bytes[i] > (1 << 24))
      return fail(MPCQ_E_INVALID, "array %d: NULL, or rows of %lld bytes (a multiple of 4 is required)", i,
                  (long long)row_bytes[i]);
  if (rows_src == 0 || rows_dst == 0) return MPCQ_OK;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  DeviceGuard dg(c->device);
  auto padded = [](size_t b) { return (b + 255) & ~size_t(255); };
  SnapItem it[mpcq::kGatherMax];
  void* mem = nullptr;
  const int32_t* dmap = map;
  if (!dev) {  // the arrays, destinations included (their other rows must come back as they were), and the map
    size_t tot = map ? padded((size_t)rows_dst * 4) : 0;
    for (int i = 0; i < n; ++i) tot += padded((size_t)rows_src * row_bytes[i]) + padded((size_t)rows_dst * row_bytes[i]);
    if (hipMalloc(&mem, tot) != hipSuccess) return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) failed", tot);
  }
  hipError_t e = hipSuccess;
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    const size_t sb = (size_t)rows_src * row_bytes[i], db = (size_t)rows_dst * row_bytes[i];
    it[i] = SnapItem{const_cast<void*>(src[i]), dst[i], sb, db, true};
    if (dev) continue;
    it[i].a = (char*)mem + off; off += padded(sb);
    it[i].b = (char*)mem + off; off += padded(db);
    if (e == hipSuccess) e = hipMemcpyAsync(it[i].a, src[i], sb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(it[i].b, dst[i], db, hipMemcpyHostToDevice, c->stream);
  }
  if (!dev && map) {
    dmap = (const int32_t*)((char*)mem + off);
    if (e == hipSuccess) e = hipMemcpyAsync((char*)mem + off, map, (size_t)rows_dst * 4, hipMemcpyHostToDevice, c->stream);
  }
  mpcq::GatherArgs a{};
  rc = e == hipSuccess ? gather_table(it, n, rows_src, rows_dst, &a) : MPCQ_OK;
  if (!rc && e == hipSuccess) {
    a.map = dmap;
    e = mpcq::launch_gather_rows(a, c->stream);
  }
  if (!dev)
    for (int i = 0; i < n && !rc && e == hipSuccess; ++i)
      e = hipMemcpyAsync(dst[i], it[i].b, it[i].bytes_b, hipMemcpyDeviceToHost, c->stream);
  if (!dev || !(flags & MPCQ_FLAG_ASYNC)) {
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
  }
  if (mem) (void)hipFree(mem);
  if (rc) return rc;
  HIP_TRY(e);
  return MPCQ_OK;
}

}  // extern "C"
