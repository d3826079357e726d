// mpcq_session_api.cpp — the mpcq_session_* entry points of include/mpcq.h: closed-loop
// sessions, per-robot state resident in HBM.
//
// A session's device arrays come in parts (grp[], one allocation each): the main one made by
// mpcq_session_create, the others when their stage is first enabled.  What a part is -- its arrays,
// their sizes, what a snapshot holds of it, its place in a blob -- is one row of kParts
// (mpcq_session_layout.h); enables, reads, snapshots and blobs walk that table.  A tick
// (session_tick) is a list of stages, each filling the argument struct of its launch from the
// parts' arrays.  All numerics run in the HIP kernels.
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "mpcq_host.h"
#include "mpcq_session_layout.h"

using namespace mpcq;

namespace {

// The arrays of one part, by the part's own ids (null: not there, or not held).
struct Group {
  void* mem = nullptr;  // the allocation (null: the part is absent, or a table's, which its Table<> owns)
  void* ptr[kPartArrays] = {};
  size_t bytes[kPartArrays] = {};
  bool there() const { return mem || ptr[0]; }
  double* d(int w) const { return (double*)ptr[w]; }
  int32_t* i(int w) const { return (int32_t*)ptr[w]; }
};

}  // namespace

struct mpcq_session {
  mpcq_ctx* ctx = nullptr;
  int64_t B = 0;
  mpcq_planner_params pp{};
  Group grp[G_COUNT];       // the parts' arrays (made by mpcq_session_create and the first enable of each)
  bool on[G_COUNT] = {};    // the part's stage runs (mpcq_session_enable_* / _disable_*)
  bool have_order = false;  // MPCQ_SV_ORDER holds the next solve's order (longest previous first)
  bool use_order = true;    // MPCQ_DISPATCH_ORDER=0 turns it off (A/B timing only; results are identical)
  bool resets = false;      // mpcq_session_reset was called: from then on the ticks consult MPCQ_SV_FIRST
  mpcq_disturb_params dp{};
  mpcq_gait_params gp{};
  mpcq::GaitArgs gait_lib{};  // the library in force, packed (period, lib; the launch fills the rest)
  mpcq_swing_params sp{};
  mpcq_plant_params pl{};
  mpcq_monitor_params mp{};
  mpcq_scenario_params sc{};
  mpcq_channel_params ch{};  // (delay and latency: what the channel's rings were primed under)
  mpcq_estimator_params ep{};
  RobotTable robots;        // mpcq_session_set_robots (the session's own, not the context's)
  RobotTable plant_robots;  // mpcq_session_set_plant_robots
  WeightsTable weights;     // mpcq_session_set_weights (the controller's tuning: no snapshot holds it)
  DisturbTable disturb;     // mpcq_session_set_disturbance (the controller's model: no snapshot holds it)
  FillTables fill;          // the table a ROB launch reads in place of the one that is not set
  mpcq_snapshot* fork_snap = nullptr;  // mpcq_session_fork's own, made on first use
};

namespace {

// The arrays of nb[w] bytes, each 256-B aligned, in one allocation zeroed on the context's
// stream (the call blocks): g->mem, ptr[w] (null where nb[w] is 0) and bytes[w].  On a failure
// nothing stays allocated and nothing is written.
int alloc_group(mpcq_ctx* c, const char* what, const size_t nb[kPartArrays], Group* g) {
  auto padded = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t tot = 0;
  for (int w = 0; w < kPartArrays; ++w) tot += padded(nb[w]);
  void* m = nullptr;
  if (hipMalloc(&m, tot) != hipSuccess) return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) for %s failed", tot, what);
  hipError_t e = hipMemsetAsync(m, 0, tot, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipFree(m);
    return fail(MPCQ_E_DEVICE, "zeroing %s failed: %s", what, hipGetErrorString(e));
  }
  size_t off = 0;
  for (int w = 0; w < kPartArrays; ++w) {
    g->ptr[w] = nb[w] ? (char*)m + off : nullptr;
    g->bytes[w] = nb[w];
    off += padded(nb[w]);
  }
  g->mem = m;
  return MPCQ_OK;
}

// Part gi of the session as g (an empty Group takes it away); a part whose arrays are ids of
// another part too shows there as well.
void install_part(mpcq_session* s, int gi, const Group& g) {
  const Part& p = kParts[gi];
  s->grp[gi] = g;
  for (int w = 0; p.alias >= 0 && w < p.count; ++w) {
    s->grp[p.alias].ptr[p.alias_at + w] = g.ptr[w];
    s->grp[p.alias].bytes[p.alias_at + w] = g.bytes[w];
  }
}

// Nothing to fill: the arrays stay zero.
int no_fill(const Group&) { return MPCQ_OK; }

// Part gi of the session where it does not exist yet: allocated from its row of kParts, zero, then
// fill(g) (enqueues on the context's stream; an mpcq code).  All or nothing: on a failure the
// session is as it was.
template <class Fill>
int ensure_part(mpcq_session* s, int gi, Fill fill, int k_mpc = 0) {
  if (s->grp[gi].mem) return MPCQ_OK;
  mpcq_ctx* c = s->ctx;
  size_t nb[kPartArrays];
  part_sizes(gi, (size_t)s->B, c->N, k_mpc, false, nb);
  Group g;
  int rc = alloc_group(c, kParts[gi].live, nb, &g);
  if (rc) return rc;
  install_part(s, gi, g);
  rc = fill(s->grp[gi]);
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(g.mem);
    install_part(s, gi, Group{});
  }
  return rc;
}

int init_failed(int gi, hipError_t e) {
  return fail(MPCQ_E_DEVICE, "initialising %s failed: %s", kParts[gi].live, hipGetErrorString(e));
}

// Array w of a fresh part from one row of row_bytes bytes, the same for every robot (blocking).
int fill_rows(mpcq_session* s, int gi, const Group& g, int w, const void* row, size_t row_bytes) {
  char* h = (char*)malloc(g.bytes[w]);
  if (!h) return fail(MPCQ_E_NOMEM, "host malloc failed");
  for (size_t off = 0; off < g.bytes[w]; off += row_bytes) memcpy(h + off, row, row_bytes);
  hipError_t e = hipMemcpyAsync(g.ptr[w], h, g.bytes[w], hipMemcpyHostToDevice, s->ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);
  free(h);
  return e == hipSuccess ? MPCQ_OK : init_failed(gi, e);
}

// A part whose rows missed the ticks since its stage was disabled: arrays [w0, w1) zero again.
int rezero(mpcq_session* s, int gi, int w0, int w1) {
  const Group& g = s->grp[gi];
  for (int w = w0; w < w1; ++w) HIP_TRY(hipMemsetAsync(g.ptr[w], 0, g.bytes[w], s->ctx->stream));
  return MPCQ_OK;
}

int disable_part(mpcq_session* s, int gi) {  // (the arrays stay)
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  s->on[gi] = false;
  return MPCQ_OK;
}

// The array behind an id of part gi, for the _read / _write / _device_ptr entry points.
int find(const mpcq_session* s, int gi, int what) {
  const Part& p = kParts[gi];
  if (what < 0 || what >= p.named) return fail(MPCQ_E_INVALID, "unknown %s array %d", p.kind, what);
  if (!s->grp[gi].ptr[what])
    return fail(MPCQ_E_INVALID, "%s array %d needs mpcq_session_enable_%s", p.kind, what, p.enable);
  return MPCQ_OK;
}

int group_read(mpcq_session* s, int gi, int what, void* dst, uint32_t flags) {
  if (!s || !dst) return fail(MPCQ_E_INVALID, "NULL argument");
  const int rc = find(s, gi, what);
  if (rc) return rc;
  const Group& g = s->grp[gi];
  DeviceGuard dg(s->ctx->device);
  const hipMemcpyKind kind = (flags & MPCQ_FLAG_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(hipMemcpyAsync(dst, g.ptr[what], g.bytes[what], kind, s->ctx->stream));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  return MPCQ_OK;
}

int group_device_ptr(mpcq_session* s, int gi, int what, void** out) {
  if (!s || !out) return fail(MPCQ_E_INVALID, "NULL argument");
  const int rc = find(s, gi, what);
  if (rc) return rc;
  *out = s->grp[gi].ptr[what];
  return MPCQ_OK;
}

// A table of robots seen as its part: one array, there while the table is in force (the Table<>
// owns the memory).
void table_part(mpcq_session* s, int gi, const RobotTable& t) {
  Group g;
  if (t.count > 0) {
    g.ptr[0] = t.dev;
    g.bytes[0] = kParts[gi].bytes(0, (size_t)s->B, s->ctx->N, 0);
  }
  s->grp[gi] = g;
}

// The session's own table (robots, weights or disturbance) into `out`, or without one B records
// of `dflt`; the bytes the caller receives are the table's, to a host or a device pointer.
template <class R>
int get_table_t(mpcq_session* s, const Table<R>& t, const R& dflt, R* out, uint32_t flags) {
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  const size_t nb = (size_t)s->B * sizeof(R);
  if (t.count) {
    HIP_TRY(hipMemcpyAsync(out, t.dev, nb, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MPCQ_OK;
  }
  if (!dev) {
    for (int64_t b = 0; b < s->B; ++b) out[b] = dflt;
    return MPCQ_OK;
  }
  R* h = (R*)malloc(nb);
  if (!h) return fail(MPCQ_E_NOMEM, "host malloc failed");
  for (int64_t b = 0; b < s->B; ++b) h[b] = dflt;
  const hipError_t e = hipMemcpy(out, h, nb, hipMemcpyHostToDevice);
  free(h);
  HIP_TRY(e);
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
    *e = hipMemcpyAsync(s->grp[G_MAIN].ptr[buf], src, s->grp[G_MAIN].bytes[buf], hipMemcpyHostToDevice, s->ctx->stream);
  return (const T*)s->grp[G_MAIN].ptr[buf];
}

// What mpcq_session_reset enqueues on the context's stream, from device pointers: the reset
// launch and, on a session that has ticked, the next solve's order.  Shared with a tick's
// auto-reset (mpcq_session_enable_monitor) and, with mark == false over all robots, with
// mpcq_session_create: the creation state is what reset_kernel writes, and nothing else.
hipError_t enqueue_reset(mpcq_session* s, const int32_t* mask, const double* gait0, const double* q_w0, bool mark) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->grp[G_MAIN];
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
  if (s->on[G_SWING]) {
    ra.swing_ref = v.d(MPCQ_SV_SWING_REF); ra.swing_ref_doubles = (int64_t)s->sp.k_mpc * 36;
    ra.swing_state = v.d(MPCQ_SV_SWING_STATE); ra.frame = v.d(MPCQ_SV_FRAME);
  }
  if (s->grp[G_MONITOR].mem) {  // a reset robot's running episode is discarded
    ra.ep = s->grp[G_MONITOR].d(MPCQ_MV_EP); ra.ep_ticks = s->grp[G_MONITOR].i(MPCQ_MV_EP_TICKS);
  }
  if (s->grp[G_GAIT].mem) ra.gstate = s->grp[G_GAIT].i(MPCQ_GV_STATE);  // no request, the table's own roll
  hipError_t e = mpcq::launch_reset(ra, c->stream);
  // the robots with a pending reset to the front of the next solve's dispatch (a session that
  // has not ticked yet has no order in use: it keeps the identity)
  if (e == hipSuccess && s->have_order)
    e = mpcq::launch_order(v.i(MPCQ_SV_ITERS), ra.first, s->B, v.i(MPCQ_SV_ORDER), c->stream);
  if (mark) s->resets = true;
  return e;
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
  const Group& v = s->grp[G_SCENARIO];
  mpcq::ScenarioArgs a{};
  a.batch = s->B; a.first = first; a.all_first = all_first; a.init = init;
  a.epoch = v.i(MPCQ_CV_EPOCH); a.tick = v.i(MPCQ_CV_TICK);
  a.base = plant_table(s);
  mpcq_default_robot(&s->ctx->p, &a.dflt);
  a.wrench_in = s->grp[G_PLANT].mem ? s->grp[G_PLANT].d(MPCQ_PV_WRENCH) : nullptr;
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
  DeviceGuard g(c->device);
  rc = ensure_part(s, G_MAIN, no_fill);
  if (rc) {
    free(h);
    delete s;
    return rc;
  }
  // every array defined before the first tick: the table a reset without gait0 goes back to,
  // the order, and what a reset of every robot writes (the gait table from gait_init) -- but
  // with no reset pending: MPCQ_SV_FIRST stays zero
  const Group& v = s->grp[G_MAIN];
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
  if (s->grp[G_MAIN].mem) {
    DeviceGuard g(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    for (int gi = 0; gi < G_COUNT; ++gi)
      if (s->grp[gi].mem) (void)hipFree(s->grp[gi].mem);
    if (s->robots.dev) (void)hipFree(s->robots.dev);
    if (s->plant_robots.dev) (void)hipFree(s->plant_robots.dev);
    if (s->weights.dev) (void)hipFree(s->weights.dev);
    if (s->disturb.dev) (void)hipFree(s->disturb.dev);
    mpcq::free_tables(s->fill);
    (void)mpcq_session_snapshot_destroy(s->fork_snap);
  }
  delete s;
  return MPCQ_OK;
}

int mpcq_session_set_robots(mpcq_session* s, const mpcq_robot* robots, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  const int rc = set_table(s->ctx, s->robots, robots ? s->B : 0, robots, flags);
  table_part(s, G_ROBOTS, s->robots);
  return rc;
}

int mpcq_session_get_robots(mpcq_session* s, mpcq_robot* robots, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!robots) return fail(MPCQ_E_INVALID, "robots is NULL");
  mpcq_robot d;
  mpcq_default_robot(&s->ctx->p, &d);
  return get_table_t(s, s->robots, d, robots, flags);
}

int mpcq_session_set_weights(mpcq_session* s, const mpcq_weights* weights, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  return set_table(s->ctx, s->weights, weights ? s->B : 0, weights, flags);
}

int mpcq_session_get_weights(mpcq_session* s, mpcq_weights* weights, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!weights) return fail(MPCQ_E_INVALID, "weights is NULL");
  mpcq_weights d;
  mpcq_default_weights(&s->ctx->p, &d);
  return get_table_t(s, s->weights, d, weights, flags);
}

int mpcq_session_set_disturbance(mpcq_session* s, const mpcq_disturbance* table, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  return set_table(s->ctx, s->disturb, table ? s->B : 0, table, flags);
}

int mpcq_session_get_disturbance(mpcq_session* s, mpcq_disturbance* table, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!table) return fail(MPCQ_E_INVALID, "table is NULL");
  return get_table_t(s, s->disturb, mpcq_disturbance{}, table, flags);  // (without a table: no disturbance)
}

int mpcq_session_enable_swing(mpcq_session* s, const mpcq_swing_params* sp) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_swing_params P;
  int rc = swing_params(sp, &P);
  if (rc) return rc;
  if (s->on[G_SWING] && P.k_mpc != s->sp.k_mpc)
    return fail(MPCQ_E_INVALID, "swing is enabled with k_mpc = %d", s->sp.k_mpc);
  DeviceGuard g(s->ctx->device);
  rc = ensure_part(s, G_SWING, no_fill, P.k_mpc);  // all-zero state = new generators
  if (rc) return rc;
  s->sp = P;
  s->on[G_SWING] = true;
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
  rc = ensure_part(s, G_PLANT, no_fill);
  if (rc) return rc;
  s->pl = P;
  s->on[G_PLANT] = true;
  return MPCQ_OK;
}

int mpcq_session_disable_plant(mpcq_session* s) { return disable_part(s, G_PLANT); }

int mpcq_session_set_plant_robots(mpcq_session* s, const mpcq_robot* robots, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  const int rc = set_table(s->ctx, s->plant_robots, robots ? s->B : 0, robots, flags);
  table_part(s, G_PLANT_ROBOTS, s->plant_robots);
  return rc;
}

int mpcq_session_set_wrench(mpcq_session* s, const double* wrench, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const int rc = ensure_part(s, G_PLANT, no_fill);  // (the first of this and mpcq_session_enable_plant makes it)
  if (rc) return rc;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  void* dst = s->grp[G_PLANT].ptr[MPCQ_PV_WRENCH];
  const size_t nb = s->grp[G_PLANT].bytes[MPCQ_PV_WRENCH];
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
  DeviceGuard g(s->ctx->device);
  const double ep0[8] = {0.0, 0.0, 0.0, 0.0, INFINITY, 0.0, 0.0, 0.0};  // the arrays, zero but for ep[4] = +inf
  rc = ensure_part(s, G_MONITOR,
                   [&](const Group& m) { return fill_rows(s, G_MONITOR, m, MPCQ_MV_EP, ep0, sizeof(ep0)); });
  if (rc) return rc;
  s->mp = P;
  s->on[G_MONITOR] = true;
  return MPCQ_OK;
}

int mpcq_session_disable_monitor(mpcq_session* s) { return disable_part(s, G_MONITOR); }

int mpcq_session_enable_scenario(mpcq_session* s, const mpcq_scenario_params* sc) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_scenario_params P;
  int rc = scenario_params(sc, &P);
  if (rc) return rc;
  DeviceGuard g(s->ctx->device);
  // the arrays, zero; the launch gives every robot the draw of epoch 0
  rc = ensure_part(s, G_SCENARIO, [&](const Group&) {
    const hipError_t e = enqueue_scenario(s, P, nullptr, false, true);
    return e == hipSuccess ? MPCQ_OK : init_failed(G_SCENARIO, e);
  });
  if (rc) return rc;
  s->sc = P;
  s->on[G_SCENARIO] = true;
  return MPCQ_OK;
}

int mpcq_session_disable_scenario(mpcq_session* s) { return disable_part(s, G_SCENARIO); }

int mpcq_session_enable_channel(mpcq_session* s, const mpcq_channel_params* ch) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_channel_params P;
  int rc = channel_params(ch, &P);
  if (rc) return rc;
  DeviceGuard g(s->ctx->device);
  // the rings hold nothing the coming ticks may read: every robot primes at its next observe
  auto arm = [&](const Group& h) {
    const hipError_t e = mpcq::launch_channel_arm(h.i(MPCQ_HV_CLOCK), s->B, s->ctx->stream);
    return e == hipSuccess ? MPCQ_OK
                           : fail(MPCQ_E_DEVICE, "arming the channel's clock failed: %s", hipGetErrorString(e));
  };
  if (!s->grp[G_CHANNEL].mem) rc = ensure_part(s, G_CHANNEL, arm);  // the arrays, zero
  else if (!s->on[G_CHANNEL] || P.delay != s->ch.delay || P.latency != s->ch.latency) rc = arm(s->grp[G_CHANNEL]);
  if (rc) return rc;
  s->ch = P;
  s->on[G_CHANNEL] = true;
  return MPCQ_OK;
}

int mpcq_session_disable_channel(mpcq_session* s) { return disable_part(s, G_CHANNEL); }

int mpcq_session_enable_estimator(mpcq_session* s, const mpcq_estimator_params* ep) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_estimator_params P;
  int rc = estimator_params(ep, &P);
  if (rc) return rc;
  DeviceGuard g(s->ctx->device);
  // the arrays, zero: every filter invalid (again, where the rings missed the ticks since a disable)
  if (s->grp[G_ESTIMATOR].mem && !s->on[G_ESTIMATOR]) rc = rezero(s, G_ESTIMATOR, MPCQ_EV_ROW, MPCQ_EV_ROW + 1);
  else rc = ensure_part(s, G_ESTIMATOR, no_fill);
  if (rc) return rc;
  s->ep = P;
  s->on[G_ESTIMATOR] = true;
  return MPCQ_OK;
}

int mpcq_session_disable_estimator(mpcq_session* s) { return disable_part(s, G_ESTIMATOR); }

int mpcq_session_enable_disturb(mpcq_session* s, const mpcq_disturb_params* dp) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_disturb_params P;
  int rc = disturb_params(dp, &P);
  if (rc) return rc;
  DeviceGuard g(s->ctx->device);
  // the arrays, zero: every row invalid, no disturbance (again, after a disable)
  if (s->grp[G_DISTURB].mem && !s->on[G_DISTURB]) rc = rezero(s, G_DISTURB, 0, MPCQ_DV_COUNT);
  else rc = ensure_part(s, G_DISTURB, no_fill);
  if (rc) return rc;
  s->dp = P;
  s->on[G_DISTURB] = true;
  return MPCQ_OK;
}

int mpcq_session_disable_disturb(mpcq_session* s) { return disable_part(s, G_DISTURB); }

int mpcq_session_enable_gait(mpcq_session* s, const mpcq_gait_params* gp, const double* cycles) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  mpcq_gait_params P;
  mpcq::GaitArgs lib{};
  int rc = gait_params(gp, cycles, &P, &lib);
  if (rc) return rc;
  DeviceGuard g(s->ctx->device);
  const int32_t row0[4] = {-1, -1, 0, 0};  // the rows, every one (want, active, phase, switches) = (-1, -1, 0, 0)
  rc = ensure_part(s, G_GAIT,
                   [&](const Group& v) { return fill_rows(s, G_GAIT, v, MPCQ_GV_STATE, row0, sizeof(row0)); });
  if (rc) return rc;
  // (by value into every later launch's arguments: a queued tick keeps the library it was launched with)
  s->gp = P;
  s->gait_lib = lib;
  s->on[G_GAIT] = true;
  return MPCQ_OK;
}

int mpcq_session_disable_gait(mpcq_session* s) { return disable_part(s, G_GAIT); }

int mpcq_session_set_gait(mpcq_session* s, const int32_t* ids, uint32_t flags) {
  if (!s) return fail(MPCQ_E_INVALID, "session is NULL");
  if (!ids) return fail(MPCQ_E_INVALID, "ids is NULL");
  if (!s->on[G_GAIT]) return fail(MPCQ_E_INVALID, "mpcq_session_set_gait needs mpcq_session_enable_gait");
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
  HIP_TRY(hipMemcpy2DAsync(s->grp[G_GAIT].ptr[MPCQ_GV_STATE], 16, ids, 4, 4, (size_t)s->B,
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
  const Group& v = s->grp[G_MAIN];
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
  const int32_t* first = s->resets && k != 0 ? s->grp[G_MAIN].i(MPCQ_SV_FIRST) : nullptr;
  HIP_TRY(enqueue_scenario(s, s->sc, first, k == 0, false));
  return MPCQ_OK;
}

// The channel's measurement model: the planner's state becomes the observation of the truth
// (t.state, which the plant keeps); it takes the first flags as the planner will.
int tick_observe(mpcq_session* s, Tick& t) {
  const Group& h = s->grp[G_CHANNEL];
  mpcq::ObserveArgs a{};
  a.batch = s->B; a.first = t.first_k; a.all_first = t.k == 0; a.truth = t.state;
  a.clock = h.i(MPCQ_HV_CLOCK); a.obs = h.d(MPCQ_HV_OBS); a.draw = h.d(MPCQ_HV_DRAW);
  a.s_ring = h.d(MPCQ_HV_S_RING); a.f_ring = h.d(MPCQ_HV_F_RING);
  HIP_TRY(mpcq::launch_observe(s->ch, a, s->ctx->stream));
  t.plan_state = h.d(MPCQ_HV_OBS);
  return MPCQ_OK;
}

// What the estimator and the disturbance stage read in a tick: what the planner would take as
// its state (t.plan_state), the previous tick's f0, feet and statuses as they stand before this
// tick's planner, and the model's robots; they take the first flags as the planner will.
void tick_model_inputs(mpcq_session* s, const Tick& t, mpcq::ModelInputs* a) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->grp[G_MAIN];
  a->batch = s->B; a->first = t.first_k; a->all_first = t.k == 0; a->meas = t.plan_state;
  a->f_prev = v.d(MPCQ_SV_F0); a->fsteps = v.d(MPCQ_SV_FSTEPS);
  a->status = v.i(MPCQ_SV_STATUS); a->plan_status = v.i(SP_PLAN_STATUS);
  a->robots = s->robots.count ? s->robots.dev : nullptr;
  mpcq_default_robot(&c->p, &a->dflt);
  a->dt = c->p.dt; a->gravity = c->p.gravity;
}

// The estimator: the planner's state becomes the filter's estimate from what it would have
// taken (tick_model_inputs).
int tick_estimate(mpcq_session* s, Tick& t) {
  const Group& e = s->grp[G_ESTIMATOR];
  mpcq::EstimateArgs a{};
  tick_model_inputs(s, t, &a);
  a.row = e.d(MPCQ_EV_ROW); a.est = e.d(MPCQ_EV_EST);
  HIP_TRY(mpcq::launch_estimate(s->ep, a, s->ctx->stream));
  t.plan_state = e.d(MPCQ_EV_EST);
  return MPCQ_OK;
}

// The disturbance stage: MPCQ_DV_DIST from what the planner is about to take as its state
// (t.plan_state, which stays; tick_model_inputs).
int tick_disturb(mpcq_session* s, const Tick& t) {
  const Group& d = s->grp[G_DISTURB];
  mpcq::DisturbArgs a{};
  tick_model_inputs(s, t, &a);
  a.row = d.d(MPCQ_DV_ROW); a.dist = (mpcq_disturbance*)d.ptr[MPCQ_DV_DIST]; a.resid = d.d(MPCQ_DV_RESID);
  HIP_TRY(mpcq::launch_disturb(s->dp, a, s->ctx->stream));
  return MPCQ_OK;
}

// The channel's actuation model: MPCQ_HV_F_CMD from this tick's (and earlier) MPCQ_SV_F0.
int tick_actuate(mpcq_session* s) {
  const Group& h = s->grp[G_CHANNEL];
  mpcq::ActuateArgs a{};
  a.batch = s->B; a.f0 = s->grp[G_MAIN].d(MPCQ_SV_F0); a.clock = h.i(MPCQ_HV_CLOCK); a.draw = h.d(MPCQ_HV_DRAW);
  a.f_ring = h.d(MPCQ_HV_F_RING); a.f_cmd = h.d(MPCQ_HV_F_CMD);
  HIP_TRY(mpcq::launch_actuate(s->ch, a, s->ctx->stream));
  return MPCQ_OK;
}

// The planner (processing.py:80-89, 131), between ev[0] and ev[1].
int tick_plan(mpcq_session* s, const Tick& t) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->grp[G_MAIN];
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
  if (s->on[G_GAIT]) {  // the gait stage rolls in the planner's place, on the command the planner reads
    mpcq::GaitArgs ga = s->gait_lib;
    ga.batch = s->B; ga.v_ref = t.v_ref; ga.gait = v.d(MPCQ_SV_GAIT); ga.gstate = s->grp[G_GAIT].i(MPCQ_GV_STATE);
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
  const Group& v = s->grp[G_MAIN];
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
  est.dev = (mpcq_disturbance*)s->grp[G_DISTURB].ptr[MPCQ_DV_DIST];
  est.cap = est.count = s->B;
  const bool comp = s->on[G_DISTURB] && s->dp.compensate != 0;
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
  const Group& v = s->grp[G_MAIN];
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
  if (s->on[G_SWING]) {  // the frame of this tick's fsteps: q_w's x, y, yaw
    double* fr = v.d(MPCQ_SV_FRAME);
    HIP_TRY(hipMemcpy2DAsync(fr, 24, a.q_w, 48, 16, B, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpy2DAsync(fr + 2, 24, a.q_w + 5, 48, 8, B, hipMemcpyDeviceToDevice, c->stream));
  }
  if (s->on[G_PLANT])  // the world pose the plant starts from
    HIP_TRY(hipMemcpyAsync(s->grp[G_PLANT].ptr[PP_QW_PREV], a.q_w, B * 48, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(mpcq::launch_retrieve(c->N, a, c->stream));
  return MPCQ_OK;
}

// The rigid body under this tick's forces takes the place of the prediction.
int tick_plant(mpcq_session* s, const Tick& t) {
  mpcq_ctx* c = s->ctx;
  const Group& v = s->grp[G_MAIN];
  mpcq::PlantArgs a{};
  a.batch = s->B;
  a.state = t.state; a.fsteps = v.d(MPCQ_SV_FSTEPS);
  a.f = s->on[G_CHANNEL] ? s->grp[G_CHANNEL].d(MPCQ_HV_F_CMD) : v.d(MPCQ_SV_F0);  // (tick_actuate has run)
  // a scenario's pushes ride on the user's wrench, its robots replace the table
  a.wrench = s->on[G_SCENARIO] && s->sc.pushes ? s->grp[G_SCENARIO].d(MPCQ_CV_WRENCH) : s->grp[G_PLANT].d(MPCQ_PV_WRENCH);
  a.robots = s->on[G_SCENARIO] && s->sc.robots ? (const mpcq_robot*)s->grp[G_SCENARIO].ptr[MPCQ_CV_ROBOTS] : plant_table(s);
  mpcq_default_robot(&c->p, &a.dflt);
  a.state_out = s->grp[G_PLANT].d(MPCQ_PV_STATE_END); a.f_eff = s->grp[G_PLANT].d(MPCQ_PV_F_EFF);
  a.tail = 1;
  a.status = v.i(MPCQ_SV_STATUS); a.plan_status = v.i(SP_PLAN_STATUS); a.gait = v.d(MPCQ_SV_GAIT);
  a.q_w_prev = s->grp[G_PLANT].d(PP_QW_PREV); a.q_w = v.d(MPCQ_SV_Q_W);
  a.next_state = v.d(MPCQ_SV_STATE); a.next_l_feet = v.d(MPCQ_SV_L_FEET);
  for (int i = 0; i < 8; ++i) a.shoulders[i] = s->pp.shoulders[i];
  HIP_TRY(mpcq::launch_plant(s->pl, a, c->stream));
  return MPCQ_OK;
}

// Whose episode ended with this tick, and the episodes' statistics.
int tick_monitor(mpcq_session* s, const Tick& t) {
  const Group &v = s->grp[G_MAIN], &m = s->grp[G_MONITOR];
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
  const Group& v = s->grp[G_MAIN];
  HIP_TRY(mpcq::launch_order(v.i(MPCQ_SV_ITERS), nullptr, s->B, v.i(MPCQ_SV_ORDER), s->ctx->stream));
  s->have_order = true;
  return MPCQ_OK;
}

// The tick's swing-foot references, substeps 0..k_mpc-1 (virtual-robot lift-off).
int tick_swing(mpcq_session* s) {
  const Group& v = s->grp[G_MAIN];
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
  if (!v_ref && !(s->on[G_SCENARIO] && s->sc.commands))
    return fail(MPCQ_E_INVALID, "v_ref is required (without a scenario that commands)");
  if (k < 0) return fail(MPCQ_E_INVALID, "k must be >= 0");
  mpcq_ctx* c = s->ctx;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  Tick t{};
  t.k = k;
  t.trace = trace;
  int rc = s->on[G_SCENARIO] ? tick_scenario(s, k) : MPCQ_OK;
  if (!rc) rc = tick_inputs(s, state, l_feet, v_ref, reduced, dev, t);
  if (!rc && !v_ref) t.v_ref = s->grp[G_SCENARIO].d(MPCQ_CV_V_REF);
  if (!rc && s->on[G_CHANNEL]) rc = tick_observe(s, t);
  if (!rc && s->on[G_ESTIMATOR]) rc = tick_estimate(s, t);
  if (!rc && s->on[G_DISTURB]) rc = tick_disturb(s, t);
  if (!rc) rc = tick_plan(s, t);
  if (!rc) rc = tick_solve(s, t);
  if (!rc) rc = tick_retrieve(s, t);
  if (!rc && s->on[G_PLANT] && s->on[G_CHANNEL]) rc = tick_actuate(s);
  if (!rc && s->on[G_PLANT]) rc = tick_plant(s, t);
  if (!rc && s->on[G_MONITOR]) rc = tick_monitor(s, t);
  if (!rc) rc = tick_order(s);
  if (!rc && s->on[G_SWING]) rc = tick_swing(s);
  if (rc) return rc;
  // auto-reset, last: the swing launch above has read the tick's gait and fsteps
  if (s->on[G_MONITOR] && s->mp.auto_reset) HIP_TRY(enqueue_reset(s, s->grp[G_MONITOR].i(MPCQ_MV_DONE), nullptr, nullptr, true));
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
  if (!v_ref && !(s->on[G_SCENARIO] && s->sc.commands))
    return fail(MPCQ_E_INVALID, "v_ref is required (without a scenario that commands)");
  if (v_ref && v_ref_ticks < 1) return fail(MPCQ_E_INVALID, "v_ref [v_ref_ticks][B][6] needs v_ref_ticks >= 1");
  if (k0 < 0 || n_ticks < 1) return fail(MPCQ_E_INVALID, "need k0 >= 0 and n_ticks >= 1");
  if (k0 > INT32_MAX - n_ticks) return fail(MPCQ_E_INVALID, "k0 + n_ticks overflows");
  if (trace && !s->on[G_MONITOR]) return fail(MPCQ_E_INVALID, "a trace needs mpcq_session_enable_monitor");
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
  return group_read(s, G_MAIN, what, dst, flags);
}

int mpcq_session_plant_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, G_PLANT, what, dst, flags);
}

int mpcq_session_monitor_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, G_MONITOR, what, dst, flags);
}

int mpcq_session_scenario_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, G_SCENARIO, what, dst, flags);
}

int mpcq_session_channel_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, G_CHANNEL, what, dst, flags);
}

int mpcq_session_estimator_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, G_ESTIMATOR, what, dst, flags);
}

int mpcq_session_disturb_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, G_DISTURB, what, dst, flags);
}

int mpcq_session_gait_read(mpcq_session* s, int what, void* dst, uint32_t flags) {
  return group_read(s, G_GAIT, what, dst, flags);
}

int mpcq_session_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, G_MAIN, what, out);
}

int mpcq_session_plant_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, G_PLANT, what, out);
}

int mpcq_session_monitor_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, G_MONITOR, what, out);
}

int mpcq_session_scenario_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, G_SCENARIO, what, out);
}

int mpcq_session_channel_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, G_CHANNEL, what, out);
}

int mpcq_session_estimator_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, G_ESTIMATOR, what, out);
}

int mpcq_session_disturb_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, G_DISTURB, what, out);
}

int mpcq_session_gait_device_ptr(mpcq_session* s, int what, void** out) {
  return group_device_ptr(s, G_GAIT, what, out);
}

int mpcq_session_write(mpcq_session* s, int what, const void* src, uint32_t flags) {
  if (!s || !src) return fail(MPCQ_E_INVALID, "NULL argument");
  const int rc = find(s, G_MAIN, what);
  if (rc) return rc;
  // the engine indexes robots through the order: only order_kernel writes it
  if (what == MPCQ_SV_ORDER) return fail(MPCQ_E_INVALID, "MPCQ_SV_ORDER is read-only");
  // only mpcq_session_reset sets it (with the state a first tick needs), only the retrieve clears it
  if (what == MPCQ_SV_FIRST) return fail(MPCQ_E_INVALID, "MPCQ_SV_FIRST is read-only");
  if (what == MPCQ_SV_SWING_REF || what == MPCQ_SV_FRAME)
    return fail(MPCQ_E_INVALID, "MPCQ_SV_SWING_REF and MPCQ_SV_FRAME are read-only");
  DeviceGuard g(s->ctx->device);
  const hipMemcpyKind kind = (flags & MPCQ_FLAG_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(hipMemcpyAsync(s->grp[G_MAIN].ptr[what], src, s->grp[G_MAIN].bytes[what], kind, s->ctx->stream));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  return MPCQ_OK;
}

}  // extern "C"

// ---- snapshots: save, restore and branch robots on the device (include/mpcq.h) ------------

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
  for (int gi = 0; gi < G_COUNT; ++gi) sh.has[gi] = s->grp[gi].there();
  // the parameters the parts' arrays were filled under
  if (sh.has[G_SWING]) sh.k_mpc = s->sp.k_mpc;
  if (sh.has[G_CHANNEL]) { sh.delay = s->ch.delay; sh.latency = s->ch.latency; }
  if (sh.has[G_GAIT]) sh.n_gaits = s->gp.n_gaits;
  return sh;
}

// The session's arrays seen as a snapshot's parts (the arrays a snapshot does not hold: null).
void session_parts(const mpcq_session* s, Group out[G_COUNT]) {
  for (int gi = 0; gi < G_COUNT; ++gi)
    for (int w = 0; w < kParts[gi].count; ++w)
      if (kParts[gi].held >> w & 1u) { out[gi].ptr[w] = s->grp[gi].ptr[w]; out[gi].bytes[w] = s->grp[gi].bytes[w]; }
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
    for (int w = 0; w < kPartArrays; ++w) {
      if (!a[gi].ptr[w]) continue;
      if (n == kListMax || (b && !b[gi].ptr[w])) return -1;
      out[n++] = SnapItem{a[gi].ptr[w], b ? b[gi].ptr[w] : nullptr, a[gi].bytes[w], b ? b[gi].bytes[w] : 0,
                          (kParts[gi].rows >> w & 1u) != 0};
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
  size_t nb[G_COUNT][kPartArrays];
  snap_sizes(sh, c->N, nb);
  for (int gi = 0; gi < G_COUNT; ++gi) {
    if (!sh.has[gi]) continue;
    const int rc = alloc_group(c, kParts[gi].snap, nb[gi], &p->g[gi]);
    if (rc) {
      free_parts(p);
      return rc;
    }
  }
  p->ctx = c;
  p->sh = sh;
  return MPCQ_OK;
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
  // (the batch-wide ones -- MPCQ_MV_TOTALS -- go with the whole batch only, behind the gathers)
  SnapItem whole[kListMax];
  int nr = 0, nw = 0;
  for (int i = 0; i < n; ++i) {
    if (it[i].rows) it[nr++] = it[i];
    else whole[nw++] = it[i];
  }
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
    ga[ch].first = p->have_order ? nullptr : s->grp[G_MAIN].i(MPCQ_SV_FIRST);
    e = mpcq::launch_gather_rows(ga[ch], c->stream);
  }
  for (int i = 0; i < nw && !map && e == hipSuccess; ++i)
    e = hipMemcpyAsync(whole[i].b, whole[i].a, whole[i].bytes_b, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) {
    if (!p->have_order || p->resets) s->resets = true;
    if (s->have_order || p->have_order) {  // as enqueue_reset: the pending resets to the front
      e = mpcq::launch_order(s->grp[G_MAIN].i(MPCQ_SV_ITERS), s->resets ? s->grp[G_MAIN].i(MPCQ_SV_FIRST) : nullptr, s->B,
                             s->grp[G_MAIN].i(MPCQ_SV_ORDER), c->stream);
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
  SnapShape sh;
  bool have_order = false, resets = false;
  char msg[256];
  if (!parse_blob_header(src, bytes, c->N, &sh, &have_order, &resets, msg, sizeof(msg)))
    return fail(MPCQ_E_INVALID, "%s", msg);
  BlobHeader h;
  blob_header(sh, c->N, have_order, resets, &h);
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
  p->have_order = have_order;
  p->resets = resets;
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
