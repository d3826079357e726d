// mpcq_api.cpp — host side of the C ABI declared in include/mpcq.h: contexts, the batch
// entry points and the mpcq_debug_* diagnostics (sessions: mpcq_session_api.cpp).
//
// Owns HIP contexts, device staging buffers for host-pointer calls, stream
// and event handling.  All numerics run in the HIP kernels (mpcq_engine.hip,
// mpcq_planner.hip, mpcq_session.hip, mpcq_order.hip, mpcq_swing.hip, mpcq_plant.hip,
// mpcq_monitor.hip, mpcq_scenario.hip, mpcq_channel.hip); there is no CPU fallback: a missing
// device is an error.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "mpcq_host.h"

using namespace mpcq;

static thread_local std::string g_err;  // mpcq_last_error

int mpcq::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

namespace {

int check_params(const mpcq_params* p) {
  if (!p) return fail(MPCQ_E_INVALID, "params is NULL");
  if (!(p->dt > 0) || !(p->mass > 0)) return fail(MPCQ_E_INVALID, "dt and mass must be > 0");
  if (!(p->rho > 0) || !(p->sigma > 0) || !(p->alpha > 0 && p->alpha < 2))
    return fail(MPCQ_E_INVALID, "need rho > 0, sigma > 0, 0 < alpha < 2");
  if (!(p->eps_abs >= 0) || !(p->eps_rel >= 0)) return fail(MPCQ_E_INVALID, "eps must be >= 0");
  if (!(p->eps_prim_inf >= 0) || !(p->eps_dual_inf >= 0))
    return fail(MPCQ_E_INVALID, "eps_prim_inf / eps_dual_inf must be >= 0");
  if (p->dual_warm != 0 && p->dual_warm != 1) return fail(MPCQ_E_INVALID, "dual_warm must be 0 or 1");
  if (p->max_iter < 1 || p->check_termination < 0 || p->scaling < 0 || p->adaptive_rho_interval < 0)
    return fail(MPCQ_E_INVALID, "max_iter >= 1, check_termination/scaling/interval >= 0");
  if (!(p->adaptive_rho_tolerance >= 1)) return fail(MPCQ_E_INVALID, "adaptive_rho_tolerance >= 1");
  if (!(p->force_weight > 0)) return fail(MPCQ_E_INVALID, "force_weight must be > 0");
  for (int i = 0; i < 12; ++i)
    if (!(p->state_weights[i] > 0)) return fail(MPCQ_E_INVALID, "state weights must be > 0");
  if (p->polish < 0 || p->polish > 2) return fail(MPCQ_E_INVALID, "polish must be 0, 1 or 2");
  if (p->polish && (!(p->delta > 0) || p->polish_refine_iter < 0 || p->polish_rounds < 1))
    return fail(MPCQ_E_INVALID, "polish needs delta > 0, polish_refine_iter >= 0, polish_rounds >= 1");
  return MPCQ_OK;
}

// One array argument of a batch entry point: the caller's pointer as an input (host_in), as an
// output (host_out), or both (an in/out array), its byte count, and where the kernel reaches it
// (dev, from stage(); it converts to the argument struct's pointer type).  Every entry point
// names each argument once, here, and fills its argument struct from dev in both pointer modes.
struct Xfer {
  const void* host_in;
  void* host_out;
  size_t bytes;
  void* dev;
  template <class T>
  operator T*() const { return (T*)dev; }
};

int ensure_arena(mpcq_ctx* c, size_t bytes) {
  if (bytes <= c->arena_bytes) return MPCQ_OK;
  if (c->arena) HIP_TRY(hipFree(c->arena));
  c->arena = nullptr;
  c->arena_bytes = 0;
  size_t want = bytes + bytes / 4;
  if (hipMalloc(&c->arena, want) != hipSuccess) {
    c->arena = nullptr;
    return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) failed", want);
  }
  c->arena_bytes = want;
  return MPCQ_OK;
}

// MPCQ_FLAG_ORDER_BY_CLASS scratch: the class table (zeroed once, kept for the context's
// life) and 3 B int32 (class slots, order, iteration counts)
int ensure_class_table(mpcq_ctx* c) {
  const int slots = mpcq::class_table_slots();
  if (!c->cls_sum) {
    void* tab = nullptr;
    const size_t tb = (size_t)slots * (8 + 8);
    if (hipMalloc(&tab, tb) != hipSuccess) return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) for the class table failed", tb);
    c->cls_sum = (uint64_t*)tab;
    c->cls_cnt = c->cls_sum + slots;
    HIP_TRY(hipMemsetAsync(tab, 0, tb, c->stream));
  }
  return MPCQ_OK;
}

int ensure_order(mpcq_ctx* c, int64_t B) {
  const int trc = ensure_class_table(c);
  if (trc) return trc;
  if (B > c->ord_cap) {
    if (c->ord_buf) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(hipFree(c->ord_buf));
    }
    c->ord_buf = nullptr;
    c->ord_cap = 0;
    if (hipMalloc(&c->ord_buf, (size_t)B * 12) != hipSuccess) {
      c->ord_buf = nullptr;
      return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) for the dispatch order failed", (size_t)B * 12);
    }
    c->ord_cap = B;
  }
  return MPCQ_OK;
}

// Host pointers: the listed arrays into the context's arena, the inputs copied on its stream.
// Device pointers (dev): nothing is allocated or copied, the kernel reads the caller's arrays.
// An entry without a pointer has dev null in both.
int stage(mpcq_ctx* c, Xfer* xs, int nx, bool dev = false) {
  if (dev) {
    for (int i = 0; i < nx; ++i) xs[i].dev = xs[i].host_out ? xs[i].host_out : const_cast<void*>(xs[i].host_in);
    return MPCQ_OK;
  }
  size_t tot = 0;
  for (int i = 0; i < nx; ++i)
    if (xs[i].host_in || xs[i].host_out) tot += (xs[i].bytes + 255) & ~size_t(255);
  int rc = ensure_arena(c, tot);
  if (rc) return rc;
  size_t off = 0;
  for (int i = 0; i < nx; ++i) {
    xs[i].dev = nullptr;
    if (!(xs[i].host_in || xs[i].host_out)) continue;
    xs[i].dev = (char*)c->arena + off;
    off += (xs[i].bytes + 255) & ~size_t(255);
    if (xs[i].host_in)
      HIP_TRY(hipMemcpyAsync(xs[i].dev, xs[i].host_in, xs[i].bytes, hipMemcpyHostToDevice, c->stream));
  }
  return MPCQ_OK;
}

int unstage(mpcq_ctx* c, Xfer* xs, int nx) {
  for (int i = 0; i < nx; ++i)
    if (xs[i].host_out)
      HIP_TRY(hipMemcpyAsync(xs[i].host_out, xs[i].dev, xs[i].bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

// The end of a batch entry point: host pointers get their outputs back (blocking); with device
// pointers the call waits for the stream unless MPCQ_FLAG_ASYNC.
int finish(mpcq_ctx* c, Xfer* xs, int nx, uint32_t flags) {
  if (!(flags & MPCQ_FLAG_DEVICE_PTRS)) return unstage(c, xs, nx);
  if (!(flags & MPCQ_FLAG_ASYNC)) HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

// Sliced-solve scratch (mpcq_set_slice): the suspended iterates, the dispatch lists, the count
int ensure_slice(mpcq_ctx* c, int64_t B) {
  if (!c->sl_count) {
    if (hipMalloc(&c->sl_count, 4) != hipSuccess) {
      c->sl_count = nullptr;
      return fail(MPCQ_E_NOMEM, "hipMalloc(4) for the slice count failed");
    }
  }
  if (B > c->sl_cap) {
    if (c->res) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(hipFree(c->res));
      HIP_TRY(hipFree(c->sl_buf));
    }
    c->res = nullptr;
    c->sl_buf = nullptr;
    c->sl_cap = 0;
    const size_t rb = (size_t)B * (8 * (size_t)mpcq::res_lanes(c->N) + 3) * 8 + (size_t)B * 32;
    if (hipMalloc(&c->res, rb) != hipSuccess) {
      c->res = nullptr;
      return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) for the suspended iterates failed", rb);
    }
    if (hipMalloc(&c->sl_buf, (size_t)B * 12) != hipSuccess) {
      c->sl_buf = nullptr;
      return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) for the slice lists failed", (size_t)B * 12);
    }
    c->res_rho = c->res + (size_t)B * 8 * (size_t)mpcq::res_lanes(c->N);
    c->res_key = c->res_rho + B;
    c->res_i = (int32_t*)(c->res_key + 2 * B);
    c->sl_cap = B;
    // no half-way sample yet (res_i[8 b + 4] = 0): an instance suspended before its first one
    // -- a slice shorter than two segments -- then takes the key's fallback, not unwritten
    // memory.  Zeroed here once; every call's launch_suspended clears what its first launch
    // sampled, so each first launch starts without one.  (The other counters are written at
    // suspension, before the resumed launch reads them.)
    HIP_TRY(hipMemsetAsync(c->res_i, 0, (size_t)B * 32, c->stream));
  }
  return MPCQ_OK;
}

// The first entry of a host table that mpcq_set_robots rejects, named in the message.
int check_robots(const mpcq_robot* r, int64_t count) {
  for (int64_t i = 0; i < count; ++i) {
    const char* what = nullptr;
    if (!(isfinite(r[i].mass) && r[i].mass > 0)) what = "mass must be finite and > 0";
    for (int j = 0; j < 9 && !what; ++j)
      if (!isfinite(r[i].gI[j])) what = "gI must be finite";
    if (!what && !(isfinite(r[i].mu) && r[i].mu > 0)) what = "mu must be finite and > 0";
    if (!what && !(isfinite(r[i].fz_max) && r[i].fz_max > 0)) what = "fz_max must be finite and > 0";
    for (int j = 0; j < 4 && !what; ++j)
      if (!(r[i].reserved[j] == 0.0)) what = "reserved must be zero";
    if (what) return fail(MPCQ_E_INVALID, "robots[%lld]: %s", (long long)i, what);
  }
  return MPCQ_OK;
}

// What mpcq_estimator_step_batch and mpcq_disturb_step_batch share, after their parameters: the
// context, the required arrays (the measurement and the first output under the entry point's own
// names; xs[MI_NX] is its row), a host table's entries, the record's context fields, and the
// staging of xs[0 .. nx) -- the record's arrays in front, the entry point's own rows behind.
// B == 0 returns MPCQ_OK with nothing staged.
enum { MI_FIRST, MI_MEAS, MI_F_PREV, MI_FEET, MI_FAILED, MI_ROBOTS, MI_NX };
int model_inputs(mpcq_ctx* c, int64_t B, const int32_t* first, int all_first, const char* meas_name, const double* meas,
                 const double* f_prev, const double* feet_prev, const int32_t* failed_prev, const mpcq_robot* robots,
                 const char* out_name, uint32_t flags, Xfer* xs, int nx, mpcq::ModelInputs* a) {
  int rc = mpcq::check_ctx(c, B);
  if (rc) return rc;
  if (!meas || !f_prev || !feet_prev || !xs[MI_NX].host_out || !xs[MI_NX + 1].host_out)
    return fail(MPCQ_E_INVALID, "%s, f_prev, feet_prev, row and %s are required", meas_name, out_name);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  if (robots && !dev) {
    rc = check_robots(robots, B);
    if (rc) return rc;
  }
  if (B == 0) return MPCQ_OK;
  DeviceGuard g(c->device);
  a->batch = B;
  a->all_first = all_first != 0;
  a->dt = c->p.dt;
  a->gravity = c->p.gravity;
  mpcq_default_robot(&c->p, &a->dflt);
  const size_t b = (size_t)B;
  xs[MI_FIRST] = {first, nullptr, b * 4, nullptr};
  xs[MI_MEAS] = {meas, nullptr, b * 96, nullptr};
  xs[MI_F_PREV] = {f_prev, nullptr, b * 96, nullptr};
  xs[MI_FEET] = {feet_prev, nullptr, b * 96, nullptr};
  xs[MI_FAILED] = {failed_prev, nullptr, b * 4, nullptr};
  xs[MI_ROBOTS] = {robots, nullptr, b * sizeof(mpcq_robot), nullptr};
  rc = stage(c, xs, nx, dev);
  if (rc) return rc;
  a->first = xs[MI_FIRST]; a->meas = xs[MI_MEAS]; a->f_prev = xs[MI_F_PREV]; a->feet_prev = xs[MI_FEET];
  a->failed = xs[MI_FAILED]; a->robots = xs[MI_ROBOTS];
  return MPCQ_OK;
}

// The first entry of a host table that mpcq_set_weights rejects, named in the message.
int check_weights(const mpcq_weights* w, int64_t count) {
  for (int64_t i = 0; i < count; ++i) {
    for (int j = 0; j < 12; ++j)
      if (!(isfinite(w[i].state[j]) && w[i].state[j] > 0))
        return fail(MPCQ_E_INVALID, "weights[%lld]: state[%d] must be finite and > 0", (long long)i, j);
    if (!(isfinite(w[i].force) && w[i].force > 0))
      return fail(MPCQ_E_INVALID, "weights[%lld]: force must be finite and > 0", (long long)i);
    for (int j = 0; j < 3; ++j)
      if (!(w[i].reserved[j] == 0.0))
        return fail(MPCQ_E_INVALID, "weights[%lld]: reserved must be zero", (long long)i);
  }
  return MPCQ_OK;
}

// The first entry of a host table that mpcq_set_disturbance rejects, named in the message.
int check_disturbance(const mpcq_disturbance* d, int64_t count) {
  for (int64_t i = 0; i < count; ++i) {
    for (int j = 0; j < 6; ++j)
      if (!isfinite(d[i].a[j]))
        return fail(MPCQ_E_INVALID, "disturbance[%lld]: a[%d] must be finite", (long long)i, j);
    for (int j = 0; j < 2; ++j)
      if (!(d[i].reserved[j] == 0.0))
        return fail(MPCQ_E_INVALID, "disturbance[%lld]: reserved must be zero", (long long)i);
  }
  return MPCQ_OK;
}

// The table a launch of `batch` instances reads: null without one, an error if it is too short.
template <class R>
int launch_table(const Table<R>& t, const char* what, int64_t batch, const R** out) {
  *out = nullptr;
  if (t.count == 0) return MPCQ_OK;
  if (batch > t.count)
    return fail(MPCQ_E_INVALID, "batch %lld > the %s table's count %lld", (long long)batch, what, (long long)t.count);
  *out = t.dev;
  return MPCQ_OK;
}

// set_table over any record type; check: the host table's validation.
template <class R>
int set_table_t(mpcq_ctx* c, Table<R>& t, int64_t count, const R* rows, uint32_t flags, const char* what,
                int (*check)(const R*, int64_t)) {
  if (count < 0 || count > (int64_t)0x7fffffff) return fail(MPCQ_E_INVALID, "bad %s count %lld", what, (long long)count);
  if (count == 0 || !rows) {
    t.count = 0;
    return MPCQ_OK;
  }
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  if (!dev) {
    const int rc = check(rows, count);
    if (rc) return rc;
  }
  DeviceGuard g(c->device);
  if (count > t.cap) {  // the new buffer first: a failed allocation leaves the table in force as it was
    const size_t nb = (size_t)count * sizeof(R);
    R* grown = nullptr;
    if (hipMalloc(&grown, nb) != hipSuccess)
      return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) for the %s table failed", nb, what);
    if (t.dev) {
      hipError_t e = hipStreamSynchronize(c->stream);  // a queued launch may still read it
      if (e == hipSuccess) e = hipFree(t.dev);
      if (e != hipSuccess) {
        (void)hipFree(grown);
        return fail(MPCQ_E_DEVICE, "releasing the previous %s table failed: %s", what, hipGetErrorString(e));
      }
    }
    t.dev = grown;
    t.cap = count;
    t.count = 0;  // (nothing copied yet)
  }
  HIP_TRY(hipMemcpyAsync(t.dev, rows, (size_t)count * sizeof(R), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                         c->stream));
  t.count = count;
  if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

// `rows` copies of the context's own record in a fill table (mpcq_host.h FillTables).
template <class R>
int ensure_fill(mpcq_ctx* c, Table<R>& t, int64_t rows, const R& rec) {
  if (t.count >= rows) return MPCQ_OK;
  R* h = (R*)malloc((size_t)rows * sizeof(R));
  if (!h) return fail(MPCQ_E_NOMEM, "malloc for a table of the context's values failed");
  for (int64_t i = 0; i < rows; ++i) h[i] = rec;
  const int rc = mpcq::set_table(c, t, rows, h, 0);
  free(h);
  return rc;
}

}  // namespace

// What mpcq_session_api.cpp shares (mpcq_host.h).

int mpcq::swing_params(const mpcq_swing_params* sp, mpcq_swing_params* out) {
  if (sp) *out = *sp;
  else mpcq_default_swing_params(out);
  if (!(out->dt > 0) || out->k_mpc < 1 || !(out->t_lock >= 0))
    return fail(MPCQ_E_INVALID, "swing needs dt > 0, k_mpc >= 1, t_lock >= 0");
  return MPCQ_OK;
}

int mpcq::plant_params(const mpcq_plant_params* pl, double dt_default, mpcq_plant_params* out) {
  if (pl) *out = *pl;
  else {
    mpcq_default_plant_params(out);
    if (dt_default > 0) out->dt = dt_default;
  }
  if (!(out->dt > 0) || out->n_sub < 1 ||
      (out->integrator != MPCQ_PLANT_MODEL && out->integrator != MPCQ_PLANT_RIGID))
    return fail(MPCQ_E_INVALID, "the plant needs dt > 0, n_sub >= 1, integrator MPCQ_PLANT_MODEL or MPCQ_PLANT_RIGID");
  return MPCQ_OK;
}

int mpcq::monitor_params(const mpcq_monitor_params* mp, mpcq_monitor_params* out) {
  if (mp) *out = *mp;
  else mpcq_default_monitor_params(out);
  if (!(out->max_tilt > 0)) return fail(MPCQ_E_INVALID, "the monitor needs max_tilt > 0 (+inf: no tilt test)");
  if (isnan(out->min_height) || out->min_height == INFINITY)
    return fail(MPCQ_E_INVALID, "the monitor needs a finite min_height (or -inf: no height test)");
  if (out->max_ticks < 0) return fail(MPCQ_E_INVALID, "the monitor needs max_ticks >= 0");
  if (out->auto_reset != 0 && out->auto_reset != 1) return fail(MPCQ_E_INVALID, "auto_reset must be 0 or 1");
  return MPCQ_OK;
}

int mpcq::scenario_params(const mpcq_scenario_params* sc, mpcq_scenario_params* out) {
  if (sc) *out = *sc;
  else mpcq_default_scenario_params(out);
  const mpcq_scenario_params& p = *out;
  auto bounds = [](const double* lo, const double* hi, int n) {
    for (int i = 0; i < n; ++i)
      if (!isfinite(lo[i]) || !isfinite(hi[i]) || lo[i] > hi[i]) return false;
    return true;
  };
  if (!bounds(p.v_lo, p.v_hi, 3) || !bounds(p.wrench_lo, p.wrench_hi, 6) ||
      !bounds(&p.mass_scale_lo, &p.mass_scale_hi, 1) || !bounds(&p.mu_lo, &p.mu_hi, 1))
    return fail(MPCQ_E_INVALID, "the scenario needs finite bounds with lo <= hi");
  if ((p.robots & 1) && !(p.mass_scale_lo > 0)) return fail(MPCQ_E_INVALID, "the scenario needs mass_scale_lo > 0");
  if ((p.robots & 2) && !(p.mu_lo > 0)) return fail(MPCQ_E_INVALID, "the scenario needs mu_lo > 0");
  if (!(p.push_prob >= 0 && p.push_prob <= 1)) return fail(MPCQ_E_INVALID, "the scenario needs push_prob in [0, 1]");
  const int32_t ints[] = {p.commands, p.cmd_start, p.cmd_ramp, p.cmd_period, p.pushes, p.push_first,
                          p.push_period, p.push_jitter, p.push_ticks, p.push_flip, p.robots};
  for (int32_t v : ints)
    if (v < 0) return fail(MPCQ_E_INVALID, "the scenario's integer fields must be >= 0");
  if (p.pushes && p.push_ticks < 1) return fail(MPCQ_E_INVALID, "the scenario's pushes need push_ticks >= 1");
  if (p.cmd_period != 0 && (int64_t)p.cmd_period < (int64_t)p.cmd_start + p.cmd_ramp)
    return fail(MPCQ_E_INVALID, "the scenario needs cmd_period == 0 or cmd_period >= cmd_start + cmd_ramp");
  if (p.push_period != 0 && (int64_t)p.push_jitter + p.push_ticks > (int64_t)p.push_period)
    return fail(MPCQ_E_INVALID, "the scenario needs push_period == 0 or push_jitter + push_ticks <= push_period");
  if (p.robots > 3) return fail(MPCQ_E_INVALID, "the scenario's robots has bits beyond 3");
  if (p.push_flip > 63) return fail(MPCQ_E_INVALID, "the scenario's push_flip has bits beyond 63");
  for (int i = 0; i < 5; ++i)
    if (p.reserved[i]) return fail(MPCQ_E_INVALID, "the scenario's reserved fields must be zero");
  return MPCQ_OK;
}

int mpcq::channel_params(const mpcq_channel_params* ch, mpcq_channel_params* out) {
  if (ch) *out = *ch;
  else mpcq_default_channel_params(out);
  const mpcq_channel_params& p = *out;
  if (p.delay < 0 || p.delay > MPCQ_CHANNEL_MAX_DELAY)
    return fail(MPCQ_E_INVALID, "the channel needs delay in 0..%d (got %d)", MPCQ_CHANNEL_MAX_DELAY, p.delay);
  if (p.latency < 0 || p.latency > MPCQ_CHANNEL_MAX_LATENCY)
    return fail(MPCQ_E_INVALID, "the channel needs latency in 0..%d (got %d)", MPCQ_CHANNEL_MAX_LATENCY, p.latency);
  if (!(p.hold_prob >= 0 && p.hold_prob <= 1)) return fail(MPCQ_E_INVALID, "the channel needs hold_prob in [0, 1]");
  auto amplitude = [](double v) { return isfinite(v) && v >= 0; };
  for (int i = 0; i < 12; ++i)
    if (!amplitude(p.sigma[i])) return fail(MPCQ_E_INVALID, "the channel needs a finite sigma[%d] >= 0", i);
  for (int i = 0; i < 12; ++i)
    if (!amplitude(p.bias[i])) return fail(MPCQ_E_INVALID, "the channel needs a finite bias[%d] >= 0", i);
  for (int i = 0; i < 3; ++i)
    if (!amplitude(p.f_sigma[i])) return fail(MPCQ_E_INVALID, "the channel needs a finite f_sigma[%d] >= 0", i);
  if (!amplitude(p.f_gain) || !(p.f_gain < 1)) return fail(MPCQ_E_INVALID, "the channel needs 0 <= f_gain < 1");
  for (int i = 0; i < 2; ++i)
    if (p.reserved[i]) return fail(MPCQ_E_INVALID, "the channel's reserved fields must be zero");
  return MPCQ_OK;
}

int mpcq::estimator_params(const mpcq_estimator_params* ep, mpcq_estimator_params* out) {
  if (ep) *out = *ep;
  else mpcq_default_estimator_params(out);
  const mpcq_estimator_params& p = *out;
  if (p.lag < 0 || p.lag > MPCQ_ESTIMATOR_MAX_LAG)
    return fail(MPCQ_E_INVALID, "the estimator needs lag in 0..%d (got %d)", MPCQ_ESTIMATOR_MAX_LAG, p.lag);
  if (p.f_lag < 0 || p.f_lag > MPCQ_ESTIMATOR_MAX_F_LAG)
    return fail(MPCQ_E_INVALID, "the estimator needs f_lag in 0..%d (got %d)", MPCQ_ESTIMATOR_MAX_F_LAG, p.f_lag);
  for (int i = 0; i < 12; ++i)
    if (!(isfinite(p.q[i]) && p.q[i] >= 0)) return fail(MPCQ_E_INVALID, "the estimator needs a finite q[%d] >= 0", i);
  for (int i = 0; i < 12; ++i)
    if (!(isfinite(p.r[i]) && p.r[i] > 0)) return fail(MPCQ_E_INVALID, "the estimator needs a finite r[%d] > 0", i);
  for (int i = 0; i < 12; ++i)
    if (!(isfinite(p.p0[i]) && p.p0[i] >= 0)) return fail(MPCQ_E_INVALID, "the estimator needs a finite p0[%d] >= 0", i);
  for (int i = 0; i < 5; ++i)
    if (p.reserved[i]) return fail(MPCQ_E_INVALID, "the estimator's reserved fields must be zero");
  return MPCQ_OK;
}

int mpcq::disturb_params(const mpcq_disturb_params* dp, mpcq_disturb_params* out) {
  if (dp) *out = *dp;
  else mpcq_default_disturb_params(out);
  const mpcq_disturb_params& p = *out;
  for (int i = 0; i < 6; ++i)
    if (!(p.alpha[i] >= 0 && p.alpha[i] <= 1))
      return fail(MPCQ_E_INVALID, "the disturbance stage needs alpha[%d] in [0, 1]", i);
  for (int i = 0; i < 6; ++i)
    if (!(isfinite(p.d_max[i]) && p.d_max[i] > 0))
      return fail(MPCQ_E_INVALID, "the disturbance stage needs a finite d_max[%d] > 0", i);
  if (p.f_lag < 0 || p.f_lag > MPCQ_DISTURB_MAX_F_LAG)
    return fail(MPCQ_E_INVALID, "the disturbance stage needs f_lag in 0..%d (got %d)", MPCQ_DISTURB_MAX_F_LAG, p.f_lag);
  for (int i = 0; i < 5; ++i)
    if (p.reserved[i]) return fail(MPCQ_E_INVALID, "the disturbance stage's reserved fields must be zero");
  return MPCQ_OK;
}

int mpcq::gait_params(const mpcq_gait_params* gp, const double* cycles, mpcq_gait_params* out, mpcq::GaitArgs* lib) {
  if (!gp) return fail(MPCQ_E_INVALID, "the gait parameters are NULL (n_gaits has no default)");
  if (!cycles) return fail(MPCQ_E_INVALID, "the gait cycles are NULL");
  const mpcq_gait_params& p = *gp;
  if (p.n_gaits < 1 || p.n_gaits > MPCQ_GAIT_MAX)
    return fail(MPCQ_E_INVALID, "the gait library needs n_gaits in 1..%d (got %d)", MPCQ_GAIT_MAX, p.n_gaits);
  if (p.select != MPCQ_GAIT_MANUAL && p.select != MPCQ_GAIT_BY_SPEED)
    return fail(MPCQ_E_INVALID, "the gait stage's select must be MPCQ_GAIT_MANUAL or MPCQ_GAIT_BY_SPEED (got %d)", p.select);
  if (p.align != 0 && p.align != 1) return fail(MPCQ_E_INVALID, "the gait stage's align must be 0 or 1 (got %d)", p.align);
  for (int i = 0; i < p.n_gaits - 1; ++i) {
    if (isnan(p.thresholds[i])) return fail(MPCQ_E_INVALID, "the gait stage's thresholds[%d] is NaN", i);
    if (i > 0 && p.thresholds[i] < p.thresholds[i - 1])
      return fail(MPCQ_E_INVALID, "the gait stage's thresholds[%d] is below thresholds[%d]", i, i - 1);
  }
  if (!(isfinite(p.hysteresis) && p.hysteresis >= 0)) return fail(MPCQ_E_INVALID, "the gait stage needs a finite hysteresis >= 0");
  if (!(isfinite(p.yaw_weight) && p.yaw_weight >= 0)) return fail(MPCQ_E_INVALID, "the gait stage needs a finite yaw_weight >= 0");
  if (p.reserved0) return fail(MPCQ_E_INVALID, "the gait stage's reserved fields must be zero");
  for (int i = 0; i < 5; ++i)
    if (p.reserved[i]) return fail(MPCQ_E_INVALID, "the gait stage's reserved fields must be zero");
  mpcq::GaitArgs packed{};
  for (int g = 0; g < MPCQ_GAIT_MAX; ++g) packed.period[g] = 1;
  for (int g = 0; g < p.n_gaits; ++g) {
    const double* cy = cycles + (size_t)g * 100;
    int rows = 0, period = 0;
    while (rows < 20 && cy[5 * rows] != 0.0) {
      const double cnt = cy[5 * rows];
      if (!(cnt >= 1 && cnt <= 64) || cnt != (double)(int)cnt)
        return fail(MPCQ_E_INVALID, "gait %d, row %d: the count %g is not an integer in 1..64", g, rows, cnt);
      int bits = 0;
      for (int q = 0; q < 4; ++q) {
        const double v = cy[5 * rows + 1 + q];
        if (v != 0.0 && v != 1.0)
          return fail(MPCQ_E_INVALID, "gait %d, row %d: the contact %d is %g, neither 0 nor 1", g, rows, q, v);
        if (v == 1.0) bits |= 1 << q;
      }
      packed.lib[g * 20 + rows] = mpcq::gait_pack((int)cnt, bits);
      period += (int)cnt;
      ++rows;
    }
    if (rows < 1) return fail(MPCQ_E_INVALID, "gait %d, row 0: the count is 0 (a cycle has 1 to 19 rows)", g);
    if (rows > 19) return fail(MPCQ_E_INVALID, "gait %d, row 19: the count is not 0 (a cycle has 1 to 19 rows)", g);
    for (int e = 5 * rows; e < 100; ++e) {  // the terminator row too (bitwise: a NaN or a -0.0 is not zero)
      uint64_t bits;
      memcpy(&bits, cy + e, 8);
      if (bits != 0)
        return fail(MPCQ_E_INVALID, "gait %d, row %d: the %s in or after the terminator row is not zero", g, e / 5,
                    e % 5 ? "contact" : "count");
    }
    packed.period[g] = period;
  }
  *out = p;
  *lib = packed;
  return MPCQ_OK;
}

int mpcq::check_ctx(mpcq_ctx* c, int64_t batch) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  if (batch < 0 || batch > (int64_t)0x7fffffff) return fail(MPCQ_E_INVALID, "bad batch %lld", (long long)batch);
  return MPCQ_OK;
}

int mpcq::ensure_work(mpcq_ctx* c, int64_t B, double** out) {
  *out = nullptr;
  const size_t bytes = (size_t)mpcq::work_doubles(c->N) * 8 * (size_t)B;
  if (bytes == 0) return MPCQ_OK;
  if (bytes > c->work_bytes) {
    if (c->work) {
      HIP_TRY(hipStreamSynchronize(c->stream));  // a queued launch may still use it
      HIP_TRY(hipFree(c->work));
    }
    c->work = nullptr;
    c->work_bytes = 0;
    if (hipMalloc(&c->work, bytes) != hipSuccess) {
      c->work = nullptr;
      return fail(MPCQ_E_NOMEM, "hipMalloc(%zu) for the engine workspace failed", bytes);
    }
    // zeroed once, as a guard only: no kernel reads a workspace slot it has not
    // written earlier in the same launch (DESIGN.md §4.1 "LDS hygiene"; the suite
    // passes on a build without the LDS zeroing either)
    HIP_TRY(hipMemsetAsync(c->work, 0, bytes, c->stream));
    c->work_bytes = bytes;
  }
  *out = (double*)c->work;
  return MPCQ_OK;
}

int mpcq::set_table(mpcq_ctx* c, RobotTable& t, int64_t count, const mpcq_robot* robots, uint32_t flags) {
  return set_table_t(c, t, count, robots, flags, "robot", check_robots);
}

int mpcq::set_table(mpcq_ctx* c, WeightsTable& t, int64_t count, const mpcq_weights* weights, uint32_t flags) {
  return set_table_t(c, t, count, weights, flags, "weights", check_weights);
}

int mpcq::set_table(mpcq_ctx* c, DisturbTable& t, int64_t count, const mpcq_disturbance* rows, uint32_t flags) {
  return set_table_t(c, t, count, rows, flags, "disturbance", check_disturbance);
}

int mpcq::launch_tables(mpcq_ctx* c, const RobotTable& robots, const WeightsTable* weights,
                        const DisturbTable& disturb, FillTables& fill, int64_t batch, LaunchArgs* a) {
  const mpcq_robot* r = nullptr;
  const mpcq_weights* w = nullptr;
  const mpcq_disturbance* d = nullptr;
  a->robots = nullptr;
  a->weights = nullptr;
  a->disturb = nullptr;
  int rc = launch_table(robots, "robot", batch, &r);
  if (rc) return rc;
  if (weights) rc = launch_table(*weights, "weights", batch, &w);
  if (rc) return rc;
  rc = launch_table(disturb, "disturbance", batch, &d);
  if (rc) return rc;
  if (!r && !w && !d) return MPCQ_OK;
  if (!r) {
    mpcq_robot rec;
    mpcq_default_robot(&c->p, &rec);
    rc = ensure_fill(c, fill.robots, batch, rec);
    if (rc) return rc;
    r = fill.robots.dev;
  }
  if (!w && weights) {
    mpcq_weights rec;
    mpcq_default_weights(&c->p, &rec);
    rc = ensure_fill(c, fill.weights, batch, rec);
    if (rc) return rc;
    w = fill.weights.dev;
  }
  if (!d) {
    mpcq_disturbance rec;
    memset(&rec, 0, sizeof(rec));
    rc = ensure_fill(c, fill.disturb, batch, rec);
    if (rc) return rc;
    d = fill.disturb.dev;
  }
  a->robots = r;
  a->weights = w;
  a->disturb = d;
  return MPCQ_OK;
}

void mpcq::free_tables(FillTables& fill) {
  if (fill.robots.dev) (void)hipFree(fill.robots.dev);
  if (fill.weights.dev) (void)hipFree(fill.weights.dev);
  if (fill.disturb.dev) (void)hipFree(fill.disturb.dev);
  fill = FillTables{};
}

extern "C" {

int mpcq_abi_version(void) { return MPCQ_ABI_VERSION; }

// Reference constants: MPC.py:25-39 (dt from main.py:20, mass, gI, mu), 67-70
// (footholds), 201 (g), 228 (fz_max), 255-275 (weights); OSQP settings
// MPC.py:414-416 + osqp 0.6 defaults.
void mpcq_default_params(mpcq_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->dt = 0.02;
  p->mass = 2.50000279;
  const double gI[9] = {3.09249e-2, -8.00101e-7, 1.865287e-5, -8.00101e-7, 5.106100e-2,
                        1.245813e-4, 1.865287e-5, 1.245813e-4, 6.939757e-2};
  memcpy(p->gI, gI, sizeof(gI));
  p->mu = 0.9;
  p->fz_max = 25.0;
  p->gravity = 9.81;
  const double w[12] = {0.1, 0.1, 1.0, 0.11, 0.11, 0.11, 2.0 * sqrt(0.1), 2.0 * sqrt(0.1),
                        2.0 * sqrt(1.0), 0.05 * sqrt(0.11), 0.05 * sqrt(0.11), 0.05 * sqrt(0.11)};
  memcpy(p->state_weights, w, sizeof(w));
  p->force_weight = 1.0e-5;
  const double fh[12] = {0.19, 0.19, -0.19, -0.19, 0.15005, -0.15005,
                         0.15005, -0.15005, 0.0, 0.0, 0.0, 0.0};
  memcpy(p->footholds, fh, sizeof(fh));
  p->rho = 0.1;
  p->sigma = 1e-6;
  p->alpha = 1.6;
  p->eps_abs = 1e-7;
  p->eps_rel = 1e-7;
  p->adaptive_rho_tolerance = 5.0;
  p->delta = 1e-6;
  p->eps_prim_inf = 1e-4;
  p->eps_dual_inf = 1e-4;
  p->max_iter = 4000;
  p->check_termination = 25;
  p->adaptive_rho = 1;
  p->adaptive_rho_interval = 100;
  p->scaling = 10;
  p->polish = 0;
  p->polish_refine_iter = 3;
  p->polish_rounds = 1;
  p->dual_warm = 0;
}

int mpcq_dims(int N, int32_t* n, int32_t* m, int32_t* nnz) {
  if (N < 2) return fail(MPCQ_E_INVALID, "n_steps must be >= 2");
  if (n) *n = 24 * N;
  if (m) *m = 44 * N;
  if (nnz) *nnz = 126 * N - 18;
  return MPCQ_OK;
}

// CSC pattern of the dense matrix built by MPC.create_ML (MPC.py:103-151):
// state columns (-I of dynamics row k, A of dynamics row k+1), then per stage,
// foot and component the force column (dt/m row, B rows 9-11, swing row,
// friction rows).
int mpcq_pattern(int N, int32_t* indptr, int32_t* indices) {
  if (N < 2 || !indptr || !indices) return fail(MPCQ_E_INVALID, "bad arguments");
  int pos = 0;
  for (int c = 0; c < 12 * N; ++c) {
    const int k = c / 12, i = c % 12;
    indptr[c] = pos;
    indices[pos++] = c;
    if (k < N - 1) {
      if (i >= 6) indices[pos++] = 12 * (k + 1) + i - 6;
      indices[pos++] = 12 * (k + 1) + i;
    }
  }
  for (int k = 0; k < N; ++k)
    for (int f = 0; f < 4; ++f)
      for (int c = 0; c < 3; ++c) {
        indptr[12 * N + 12 * k + 3 * f + c] = pos;
        indices[pos++] = 12 * k + 6 + c;
        for (int r = 9; r < 12; ++r) indices[pos++] = 12 * k + r;
        indices[pos++] = 12 * N + 12 * k + 3 * f + c;
        const int fr = 24 * N + 20 * k + 5 * f;
        if (c == 0) { indices[pos++] = fr; indices[pos++] = fr + 1; }
        else if (c == 1) { indices[pos++] = fr + 2; indices[pos++] = fr + 3; }
        else for (int t = 0; t < 5; ++t) indices[pos++] = fr + t;
      }
  indptr[24 * N] = pos;
  return MPCQ_OK;
}

void mpcq_default_robot(const mpcq_params* p, mpcq_robot* r) {
  if (!r) return;
  mpcq_params d;
  if (!p) {
    mpcq_default_params(&d);
    p = &d;
  }
  memset(r, 0, sizeof(*r));
  r->mass = p->mass;
  memcpy(r->gI, p->gI, sizeof(r->gI));
  r->mu = p->mu;
  r->fz_max = p->fz_max;
}

void mpcq_default_weights(const mpcq_params* p, mpcq_weights* w) {
  if (!w) return;
  mpcq_params d;
  if (!p) {
    mpcq_default_params(&d);
    p = &d;
  }
  memset(w, 0, sizeof(*w));
  memcpy(w->state, p->state_weights, sizeof(w->state));
  w->force = p->force_weight;
}

int mpcq_supported_horizons(int32_t* out, int cap) { return mpcq::supported_horizons(out, cap); }

const char* mpcq_last_error(void) { return g_err.c_str(); }

int mpcq_create(int device, int n_steps, const mpcq_params* params, mpcq_ctx** out) {
  if (!out) return fail(MPCQ_E_INVALID, "out is NULL");
  *out = nullptr;
  if (!mpcq::horizon_supported(n_steps))
    return fail(MPCQ_E_UNSUPPORTED, "horizon N=%d not compiled in (supported: 4 <= N <= 64)", n_steps);
  mpcq_params p;
  if (params) p = *params;
  else mpcq_default_params(&p);
  int rc = check_params(&p);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MPCQ_E_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(MPCQ_E_INVALID, "device %d out of range (%d)", device, ndev);
  DeviceGuard g(device);
  mpcq_ctx* c = new mpcq_ctx();
  c->device = device;
  c->N = n_steps;
  c->p = p;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(MPCQ_E_DEVICE, "hipStreamCreate failed");
  }
  c->stream = c->own_stream;
  for (auto& e : c->ev)
    if (hipEventCreate(&e) != hipSuccess) {
      mpcq_destroy(c);
      return fail(MPCQ_E_DEVICE, "hipEventCreate failed");
    }
  *out = c;
  return MPCQ_OK;
}

int mpcq_destroy(mpcq_ctx* c) {
  if (!c) return MPCQ_OK;
  DeviceGuard g(c->device);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  if (c->arena) (void)hipFree(c->arena);
  if (c->work) (void)hipFree(c->work);
  if (c->cls_sum) (void)hipFree(c->cls_sum);
  if (c->ord_buf) (void)hipFree(c->ord_buf);
  if (c->res) (void)hipFree(c->res);
  if (c->sl_buf) (void)hipFree(c->sl_buf);
  if (c->sl_count) (void)hipFree(c->sl_count);
  if (c->robots.dev) (void)hipFree(c->robots.dev);
  if (c->weights.dev) (void)hipFree(c->weights.dev);
  if (c->disturb.dev) (void)hipFree(c->disturb.dev);
  mpcq::free_tables(c->fill);
  for (auto& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
  return MPCQ_OK;
}

int mpcq_set_stream(mpcq_ctx* c, void* stream) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  c->stream = stream ? (hipStream_t)stream : c->own_stream;
  return MPCQ_OK;
}

int mpcq_set_slice(mpcq_ctx* c, int32_t slice_iters) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  if (slice_iters < 0) return fail(MPCQ_E_INVALID, "slice_iters must be >= 0");
  c->slice_iters = slice_iters;
  return MPCQ_OK;
}

int mpcq_set_robots(mpcq_ctx* c, int64_t count, const mpcq_robot* robots, uint32_t flags) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  return set_table(c, c->robots, count, robots, flags);
}

int mpcq_set_weights(mpcq_ctx* c, int64_t count, const mpcq_weights* weights, uint32_t flags) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  return set_table(c, c->weights, count, weights, flags);
}

int mpcq_set_disturbance(mpcq_ctx* c, int64_t count, const mpcq_disturbance* table, uint32_t flags) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  return set_table(c, c->disturb, count, table, flags);
}

int mpcq_last_kernel_ms(mpcq_ctx* c, double* fms, double* sms) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  DeviceGuard g(c->device);
  float ms = 0.f;
  if (fms) {
    *fms = -1.0;
    if (c->have_form) {
      HIP_TRY(hipEventSynchronize(c->ev[1]));
      HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
      *fms = ms;
    }
  }
  if (sms) {
    *sms = -1.0;
    if (c->have_solve) {
      HIP_TRY(hipEventSynchronize(c->ev[3]));
      HIP_TRY(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
      *sms = ms;
    }
  }
  return MPCQ_OK;
}

int mpcq_formulate_batch(mpcq_ctx* c, int64_t B, const double* xref, const double* fsteps, int mode,
                         double* Ax, double* l, double* u, int32_t* status, uint32_t flags) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (!xref || !fsteps || !Ax || !l || !u) return fail(MPCQ_E_INVALID, "NULL array");
  if (mode != MPCQ_MODE_UPDATE && mode != MPCQ_MODE_SETUP) return fail(MPCQ_E_INVALID, "bad mode");
  if (B == 0) return MPCQ_OK;
  DeviceGuard g(c->device);
  const int N = c->N;
  const size_t n12 = 12 * (N + 1), nnz = 126 * N - 18, m = 44 * N;
  mpcq::LaunchArgs a{};
  a.batch = B;
  a.mode = mode;
  // (no P here: the weights table is not looked at)
  rc = mpcq::launch_tables(c, c->robots, nullptr, c->disturb, c->fill, B, &a);
  if (rc) return rc;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  Xfer xs[6] = {{xref, nullptr, B * n12 * 8, nullptr}, {fsteps, nullptr, (size_t)B * 260 * 8, nullptr},
                {nullptr, Ax, B * nnz * 8, nullptr},   {nullptr, l, B * m * 8, nullptr},
                {nullptr, u, B * m * 8, nullptr},      {nullptr, status, (size_t)B * 4, nullptr}};
  rc = stage(c, xs, 6, dev);
  if (rc) return rc;
  a.xref = xs[0]; a.fsteps = xs[1]; a.Ax_out = xs[2]; a.l_out = xs[3]; a.u_out = xs[4]; a.status = xs[5];
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  HIP_TRY(mpcq::launch_formulate(N, c->p, a, c->stream));
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  c->have_form = true;
  return finish(c, xs, 6, flags);
}

static int solve_common(mpcq_ctx* c, int64_t B, bool fused, const double* xref, const double* fsteps,
                        int mode, const double* Ax, const double* l, const double* u,
                        const double* warm_x, const double* warm_y, const double* rho_in, double* f0,
                        double* x, double* y, int32_t* status, int32_t* iters, double* rho_out,
                        int32_t* info, uint32_t flags) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (B == 0) return MPCQ_OK;
  DeviceGuard g(c->device);
  const int N = c->N;
  const size_t n = 24 * N, m = 44 * N, nnz = 126 * N - 18, n12 = 12 * (N + 1);
  mpcq::LaunchArgs a{};
  a.batch = B;
  a.mode = mode;
  if (fused) {  // (the qp path has formulated already)
    rc = mpcq::launch_tables(c, c->robots, &c->weights, c->disturb, c->fill, B, &a);
    if (rc) return rc;
  }
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  enum { XR, FS, AX, L, U, WX, WY, RI, F0, X, Y, ST, IT, RO, IN, NX };
  Xfer xs[NX] = {
      {xref, nullptr, B * n12 * 8, nullptr},      {fsteps, nullptr, (size_t)B * 260 * 8, nullptr},
      {Ax, nullptr, B * nnz * 8, nullptr},        {l, nullptr, B * m * 8, nullptr},
      {u, nullptr, B * m * 8, nullptr},           {warm_x, nullptr, B * n * 8, nullptr},
      {warm_y, nullptr, B * m * 8, nullptr},      {rho_in, nullptr, (size_t)B * 8, nullptr},
      {nullptr, f0, (size_t)B * 12 * 8, nullptr}, {nullptr, x, B * n * 8, nullptr},
      {nullptr, y, B * m * 8, nullptr},           {nullptr, status, (size_t)B * 4, nullptr},
      {nullptr, iters, (size_t)B * 4, nullptr},   {nullptr, rho_out, (size_t)B * 8, nullptr},
      {nullptr, info, (size_t)B * 16, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.xref = xs[XR]; a.fsteps = xs[FS]; a.Ax = xs[AX]; a.l = xs[L]; a.u = xs[U]; a.warm_x = xs[WX]; a.warm_y = xs[WY];
  a.rho_in = xs[RI]; a.f0 = xs[F0]; a.x = xs[X]; a.y = xs[Y]; a.status = xs[ST]; a.iters = xs[IT];
  a.rho_out = xs[RO]; a.info = xs[IN];
  a.stamps = c->stamps;
  rc = ensure_work(c, B, &a.work);
  if (rc) return rc;
  const bool by_class = fused && (flags & MPCQ_FLAG_ORDER_BY_CLASS);
  int32_t *cls = nullptr, *its = a.iters;
  if (by_class) {
    if (B > INT32_MAX) return fail(MPCQ_E_INVALID, "MPCQ_FLAG_ORDER_BY_CLASS: batch > INT32_MAX");
    rc = ensure_order(c, B);
    if (rc) return rc;
    cls = c->ord_buf;
    int32_t* order = c->ord_buf + B;
    if (!its) its = a.iters = c->ord_buf + 2 * B;  // (the engine writes them; the caller asked for none)
    HIP_TRY(mpcq::launch_class_order(a.fsteps, B, cls, c->cls_sum, c->cls_cnt, order, c->stream));
    a.order = order;
  }
  // sliced (mpcq_set_slice, beyond 16 stages): the first launch suspends every instance still
  // running after slice_iters iterations; a second launch resumes the suspended ones, the
  // farthest from convergence (the iterations left, extrapolated from the residuals' decay)
  // first, and runs them to their end.  (Re-slicing the second launch too was slower: C3 39.0 k
  // against 44.1 k QP/s at 1200, profiles/r06r_*.)
  // Only where the engine holds the suspend / resume code (slice_supported: beyond 16 stages):
  // a unit without it ignores the count on the device and would take the resumed launch's
  // unwritten list for instance indices.
  const bool sliced = c->slice_iters > 0 && c->slice_iters < c->p.max_iter && mpcq::slice_supported(N);
  c->last_B = B;
  c->last_by_class = by_class;
  c->last_sliced = sliced;
  if (sliced) {
    rc = ensure_slice(c, B);
    if (rc) return rc;
    a.slice_iters = c->slice_iters;
    a.res = c->res;
    a.res_rho = c->res_rho;
    a.res_key = c->res_key;
    a.res_i = c->res_i;
    if (!a.status) a.status = c->sl_buf + 2 * B;  // (the slices' statuses; the caller asked for none)
  }
  HIP_TRY(hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(mpcq::launch_solve(N, fused, c->p, a, c->stream));
  if (sliced) {  // the suspended instances, farthest from convergence first, resumed once to their end
    // (the resumed launch is sized for the whole batch and reads the count from the device:
    // workgroups past it return at once -- no host round trip, the call stays asynchronous)
    int32_t* list = c->sl_buf;
    HIP_TRY(mpcq::launch_suspended(a.order, B, a.status, c->res_key, list, c->sl_count, c->res_i, c->stream));
    mpcq::LaunchArgs r = a;
    r.order = list;
    r.batch_dev = c->sl_count;
    r.resume = 1;
    r.slice_iters = 0;
    HIP_TRY(mpcq::launch_solve(N, fused, c->p, r, c->stream));
  }
  HIP_TRY(hipEventRecord(c->ev[3], c->stream));
  if (by_class) HIP_TRY(mpcq::launch_class_learn(cls, its, B, c->cls_sum, c->cls_cnt, c->stream));
  c->have_solve = true;
  return finish(c, xs, NX, flags);
}

int mpcq_qp_solve_batch(mpcq_ctx* c, int64_t B, const double* Ax, const double* l, const double* u,
                        const double* warm_x, const double* warm_y, const double* rho_in, double* x,
                        double* y, int32_t* status, int32_t* iters, double* rho_out, int32_t* info,
                        uint32_t flags) {
  if (!Ax || !l || !u) return fail(MPCQ_E_INVALID, "Ax, l, u are required");
  return solve_common(c, B, false, nullptr, nullptr, 0, Ax, l, u, warm_x, warm_y, rho_in, nullptr, x,
                      y, status, iters, rho_out, info, flags);
}

int mpcq_solve_batch(mpcq_ctx* c, int64_t B, const double* xref, const double* fsteps, int mode,
                     const double* warm_x, const double* warm_y, const double* rho_in, double* f0,
                     double* x, double* y, double* rho_out, int32_t* status, int32_t* iters,
                     int32_t* info, uint32_t flags) {
  if (!xref || !fsteps) return fail(MPCQ_E_INVALID, "xref, fsteps are required");
  if (mode != MPCQ_MODE_UPDATE && mode != MPCQ_MODE_SETUP) return fail(MPCQ_E_INVALID, "bad mode");
  return solve_common(c, B, true, xref, fsteps, mode, nullptr, nullptr, nullptr, warm_x, warm_y,
                      rho_in, f0, x, y, status, iters, rho_out, info, flags);
}

// FootstepPlanner constants (FootstepPlanner.py:18-52, 316-322, 376; processing.py:131).
void mpcq_default_planner_params(mpcq_planner_params* pp) {
  if (!pp) return;
  memset(pp, 0, sizeof(*pp));
  pp->dt = 0.02;
  pp->T_gait = 0.32;
  pp->h_ref = 0.2027682;
  pp->k_feedback = 0.03;
  pp->L = 0.12;
  pp->g = 9.81;
  pp->t_stance = 0.16;
  pp->cmd_threshold = 0.05;
  const double sh[8] = {0.19, 0.19, -0.19, -0.19, 0.15005, -0.15005, 0.15005, -0.15005};
  memcpy(pp->shoulders, sh, sizeof(sh));
  const double ro[8] = {0.14, 0.14, -0.14, -0.14, 0.12, -0.12, 0.12, -0.12};
  memcpy(pp->reduced_offset, ro, sizeof(ro));
}

int mpcq_plan_batch(mpcq_ctx* c, const mpcq_planner_params* pp, int64_t B, uint32_t ops, int k,
                    const double* state, const double* v_cur, const double* h, const double* l_feet,
                    const double* v_ref, const int32_t* reduced, double* gait, int32_t* rot_flag,
                    double* h_rot, double* xref, double* fsteps, int32_t* status, uint32_t flags) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (ops == 0 || (ops & ~(uint32_t)MPCQ_PLAN_TICK)) return fail(MPCQ_E_INVALID, "ops must be MPCQ_PLAN_* bits");
  if (!gait || !v_ref || !state) return fail(MPCQ_E_INVALID, "gait, state and v_ref are required");
  if ((ops & MPCQ_PLAN_FOOTSTEPS) && (!l_feet || !fsteps))
    return fail(MPCQ_E_INVALID, "MPCQ_PLAN_FOOTSTEPS needs l_feet and fsteps");
  if ((ops & MPCQ_PLAN_REFSTATES) && (!rot_flag || !h_rot || !xref))
    return fail(MPCQ_E_INVALID, "MPCQ_PLAN_REFSTATES needs rot_flag, h_rot and xref");
  mpcq_planner_params P;
  if (pp) P = *pp;
  else mpcq_default_planner_params(&P);
  if (!(P.dt > 0) || !(P.g > 0) || !(P.T_gait > P.dt)) return fail(MPCQ_E_INVALID, "planner needs dt > 0, g > 0, T_gait > dt");
  if (B == 0) return MPCQ_OK;
  DeviceGuard g(c->device);
  const int N = c->N;
  const size_t n12 = 12 * (N + 1);
  mpcq::PlanArgs a{};
  a.batch = B;
  a.N = N;
  a.ops = ops;
  a.k = k;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  const bool fo = ops & MPCQ_PLAN_FOOTSTEPS, rs = ops & MPCQ_PLAN_REFSTATES;
  enum { ST, VC, H, LF, VR, RD, GA, RF, HR, XR, FS, SS, NX };
  // in/out buffers are staged both ways (host_in and host_out both set).  The arrays of a pass
  // that `ops` leaves out are null in both pointer modes: planner_kernel reads l_feet and writes
  // fsteps under MPCQ_PLAN_FOOTSTEPS only, reads and writes rot_flag, h_rot and xref under
  // MPCQ_PLAN_REFSTATES only (do_fs / do_ref guard every access).
  Xfer xs[NX] = {{state, nullptr, (size_t)B * 96, nullptr},
                 {v_cur, nullptr, (size_t)B * 48, nullptr},
                 {h, nullptr, (size_t)B * 8, nullptr},
                 {fo ? l_feet : nullptr, nullptr, (size_t)B * 96, nullptr},
                 {v_ref, nullptr, (size_t)B * 48, nullptr},
                 {reduced, nullptr, (size_t)B * 4, nullptr},
                 {gait, gait, (size_t)B * 800, nullptr},
                 {rs ? rot_flag : nullptr, rs ? rot_flag : nullptr, (size_t)B * 4, nullptr},
                 {rs ? h_rot : nullptr, rs ? h_rot : nullptr, (size_t)B * 8, nullptr},
                 {rs ? xref : nullptr, rs ? xref : nullptr, B * n12 * 8, nullptr},
                 // fsteps: staged in as well so a BAD_GAIT instance keeps the caller's values
                 {fo ? fsteps : nullptr, fo ? fsteps : nullptr, (size_t)B * 260 * 8, nullptr},
                 {nullptr, status, (size_t)B * 4, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.state = xs[ST]; a.v_cur = xs[VC]; a.h = xs[H]; a.l_feet = xs[LF]; a.v_ref = xs[VR]; a.reduced = xs[RD];
  a.gait = xs[GA]; a.rot_flag = xs[RF]; a.h_rot = xs[HR]; a.xref = xs[XR]; a.fsteps = xs[FS]; a.status = xs[SS];
  HIP_TRY(mpcq::launch_plan(P, a, c->stream));
  return finish(c, xs, NX, flags);
}

// Swing-foot constants (TSID_Debug_controller_four_legs_fb_vel.py:96-97, 107; Interface.py:91;
// main.py:21).
void mpcq_default_swing_params(mpcq_swing_params* sp) {
  if (!sp) return;
  memset(sp, 0, sizeof(*sp));
  sp->dt = 0.001;
  sp->max_height = 0.05;
  sp->t_lock = 0.05;
  sp->feet_z = 0.0;
  sp->k_mpc = 20;
}

int mpcq_swing_step_batch(mpcq_ctx* c, const mpcq_swing_params* sp, int64_t B, const double* in, double* state,
                          double* out, uint32_t flags) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (!in || !state || !out) return fail(MPCQ_E_INVALID, "in, state and out are required");
  mpcq_swing_params P;
  rc = swing_params(sp, &P);
  if (rc) return rc;
  if (B == 0) return MPCQ_OK;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  enum { IN, ST, OUT, NX };
  Xfer xs[NX] = {{in, nullptr, (size_t)B * 40 * 8, nullptr},
                 {state, state, (size_t)B * 4 * MPCQ_SWING_STATE * 8, nullptr},
                 {nullptr, out, (size_t)B * 44 * 8, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  HIP_TRY(mpcq::launch_swing_step(P, B, xs[IN], xs[ST], xs[OUT], c->stream));
  return finish(c, xs, NX, flags);
}

int mpcq_swing_batch(mpcq_ctx* c, const mpcq_swing_params* sp, int64_t B, int k_sub0, int n_sub,
                     const double* gait, const double* fsteps, const double* frame, const double* feet0,
                     double* state, double* ref, double* t0_out, int32_t* status, uint32_t flags) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (!gait || !fsteps || !frame || !state || !ref)
    return fail(MPCQ_E_INVALID, "gait, fsteps, frame, state and ref are required");
  mpcq_swing_params P;
  rc = swing_params(sp, &P);
  if (rc) return rc;
  if (k_sub0 < 0 || n_sub < 1 || (int64_t)k_sub0 + n_sub > P.k_mpc)
    return fail(MPCQ_E_INVALID, "need 0 <= k_sub0, 1 <= n_sub, k_sub0 + n_sub <= k_mpc (%d)", P.k_mpc);
  if (B == 0) return MPCQ_OK;
  DeviceGuard g(c->device);
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  mpcq::SwingArgs a{};
  a.batch = B;
  a.k_sub0 = k_sub0;
  a.n_sub = n_sub;
  enum { GA, FS, FR, F0, ST, RF, T0, SS, NX };
  Xfer xs[NX] = {{gait, nullptr, (size_t)B * 800, nullptr},
                 {fsteps, nullptr, (size_t)B * 260 * 8, nullptr},
                 {frame, nullptr, (size_t)B * 24, nullptr},
                 {feet0, nullptr, (size_t)B * 24 * 8, nullptr},
                 {state, state, (size_t)B * 4 * MPCQ_SWING_STATE * 8, nullptr},
                 {nullptr, ref, (size_t)B * n_sub * 36 * 8, nullptr},
                 {nullptr, t0_out, (size_t)B * n_sub * 4 * 8, nullptr},
                 {nullptr, status, (size_t)B * 4, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.gait = xs[GA]; a.fsteps = xs[FS]; a.frame = xs[FR]; a.feet0 = xs[F0]; a.state = xs[ST]; a.ref = xs[RF];
  a.t0_out = xs[T0]; a.status = xs[SS];
  HIP_TRY(mpcq::launch_swing(P, a, c->stream));
  return finish(c, xs, NX, flags);
}

// Rigid-body plant: one MPC tick of dt, k_mpc substeps (main.py:21), the Coulomb clamp on.
void mpcq_default_plant_params(mpcq_plant_params* pl) {
  if (!pl) return;
  memset(pl, 0, sizeof(*pl));
  pl->dt = 0.02;
  pl->gravity = 9.81;
  pl->n_sub = 20;
  pl->integrator = MPCQ_PLANT_RIGID;
  pl->clamp = 1;
}

int mpcq_plant_step_batch(mpcq_ctx* c, const mpcq_plant_params* pl, int64_t B, const double* state,
                          const double* feet, const double* f, const double* wrench, const mpcq_robot* robots,
                          double* state_out, double* f_eff, uint32_t flags) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (!state || !feet || !f || !state_out) return fail(MPCQ_E_INVALID, "state, feet, f and state_out are required");
  mpcq_plant_params P;
  rc = plant_params(pl, 0.0, &P);
  if (rc) return rc;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  if (robots && !dev) {
    rc = check_robots(robots, B);
    if (rc) return rc;
  }
  if (B == 0) return MPCQ_OK;
  DeviceGuard g(c->device);
  mpcq::PlantArgs a{};
  a.batch = B;
  mpcq_default_robot(&c->p, &a.dflt);
  enum { ST, FT, FF, WR, RB, SO, FE, NX };
  Xfer xs[NX] = {{state, nullptr, (size_t)B * 96, nullptr},
                 {feet, nullptr, (size_t)B * 96, nullptr},
                 {f, nullptr, (size_t)B * 96, nullptr},
                 {wrench, nullptr, (size_t)B * 48, nullptr},
                 {robots, nullptr, (size_t)B * sizeof(mpcq_robot), nullptr},
                 {nullptr, state_out, (size_t)B * 96, nullptr},
                 {nullptr, f_eff, (size_t)B * 96, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.state = xs[ST]; a.feet = xs[FT]; a.f = xs[FF]; a.wrench = xs[WR]; a.robots = xs[RB]; a.state_out = xs[SO];
  a.f_eff = xs[FE];
  HIP_TRY(mpcq::launch_plant(P, a, c->stream));
  return finish(c, xs, NX, flags);
}

// Episode monitor: tilt beyond 0.5 rad or the base below half of h_ref ends an episode.
void mpcq_default_monitor_params(mpcq_monitor_params* mp) {
  if (!mp) return;
  memset(mp, 0, sizeof(*mp));
  mp->max_tilt = 0.5;
  mp->min_height = 0.10;
  mp->max_ticks = 0;
  mp->auto_reset = 0;
}

int mpcq_monitor_step_batch(mpcq_ctx* c, const mpcq_monitor_params* mp, int64_t B, const double* q_w,
                            const int32_t* status, const int32_t* iters, const double* f0, const double* cost,
                            const double* state, const double* v_ref, double* ep, int32_t* ep_ticks,
                            int32_t* episodes, double* last, int32_t* done, uint64_t* totals, double* trace,
                            uint32_t flags) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (!q_w || !status || !iters || !f0 || !cost || !state || !v_ref || !ep || !ep_ticks || !done)
    return fail(MPCQ_E_INVALID, "q_w, status, iters, f0, cost, state, v_ref, ep, ep_ticks and done are required");
  mpcq_monitor_params P;
  rc = monitor_params(mp, &P);
  if (rc) return rc;
  if (B == 0) return MPCQ_OK;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  DeviceGuard g(c->device);
  mpcq::MonitorArgs a{};
  a.batch = B;
  const size_t b = (size_t)B;
  enum { QW, ST, IT, F0, CO, SA, VR, EP, ET, ES, LA, DO, TO, TR, NX };
  Xfer xs[NX] = {{q_w, nullptr, b * 48, nullptr},      {status, nullptr, b * 4, nullptr},
                 {iters, nullptr, b * 4, nullptr},     {f0, nullptr, b * 96, nullptr},
                 {cost, nullptr, b * 104, nullptr},    {state, nullptr, b * 96, nullptr},
                 {v_ref, nullptr, b * 48, nullptr},    {ep, ep, b * 64, nullptr},
                 {ep_ticks, ep_ticks, b * 4, nullptr}, {episodes, episodes, b * 4, nullptr},
                 {last, last, b * 128, nullptr},       {nullptr, done, b * 4, nullptr},
                 {totals, totals, 64, nullptr},        {trace, trace, b * MPCQ_TRACE * 8, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.q_w = xs[QW]; a.status = xs[ST]; a.iters = xs[IT]; a.f0 = xs[F0]; a.cost = xs[CO]; a.state = xs[SA];
  a.v_ref = xs[VR]; a.ep = xs[EP]; a.ep_ticks = xs[ET]; a.episodes = xs[ES]; a.last = xs[LA]; a.done = xs[DO];
  a.totals = xs[TO]; a.trace = xs[TR];
  HIP_TRY(mpcq::launch_monitor(P, a, c->stream));
  return finish(c, xs, NX, flags);
}

// Scenario: the reference's predefined joystick at MPC ticks (Joystick.py:82-83), no pushes,
// the model's own robot.
void mpcq_default_scenario_params(mpcq_scenario_params* sc) {
  if (!sc) return;
  memset(sc, 0, sizeof(*sc));
  sc->commands = 1;
  sc->v_lo[0] = sc->v_hi[0] = 1.0;
  sc->cmd_start = 48;
  sc->cmd_ramp = 175;
  sc->push_prob = 1.0;
  sc->push_ticks = 10;
  sc->mass_scale_lo = sc->mass_scale_hi = 1.0;
  sc->mu_lo = sc->mu_hi = 0.9;
}

int mpcq_scenario_step_batch(mpcq_ctx* c, const mpcq_scenario_params* sc, int64_t B, const int32_t* first,
                             int all_first, int32_t* epoch, int32_t* tick, const mpcq_robot* base,
                             const double* wrench_in, double* v_ref, double* push, double* wrench_out,
                             mpcq_robot* robots_out, double* draw, uint32_t flags) {
  mpcq_scenario_params P;
  int rc = scenario_params(sc, &P);  // first: what is wrong with the parameters needs no context
  if (rc) return rc;
  rc = check_ctx(c, B);
  if (rc) return rc;
  if (!epoch || !tick || !v_ref || !push || !wrench_out)
    return fail(MPCQ_E_INVALID, "epoch, tick, v_ref, push and wrench_out are required");
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  if (base && !dev) {
    rc = check_robots(base, B);
    if (rc) return rc;
  }
  if (B == 0) return MPCQ_OK;
  DeviceGuard g(c->device);
  mpcq::ScenarioArgs a{};
  a.batch = B;
  a.all_first = all_first != 0;
  mpcq_default_robot(&c->p, &a.dflt);
  const size_t b = (size_t)B;
  enum { FI, EP, TI, BA, WI, VR, PU, WO, RO, DR, NX };
  Xfer xs[NX] = {{first, nullptr, b * 4, nullptr},
                 {epoch, epoch, b * 4, nullptr},
                 {tick, tick, b * 4, nullptr},
                 {base, nullptr, b * sizeof(mpcq_robot), nullptr},
                 {wrench_in, nullptr, b * 48, nullptr},
                 {nullptr, v_ref, b * 48, nullptr},
                 {nullptr, push, b * 48, nullptr},
                 {nullptr, wrench_out, b * 48, nullptr},
                 {robots_out, robots_out, b * sizeof(mpcq_robot), nullptr},
                 {draw, draw, b * 64, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.first = xs[FI]; a.epoch = xs[EP]; a.tick = xs[TI]; a.base = xs[BA]; a.wrench_in = xs[WI]; a.v_ref = xs[VR];
  a.push = xs[PU]; a.wrench_out = xs[WO]; a.robots_out = xs[RO]; a.draw = xs[DR];
  HIP_TRY(mpcq::launch_scenario(P, a, c->stream));
  return finish(c, xs, NX, flags);
}

// Channel: everything zero, a channel that changes nothing.
void mpcq_default_channel_params(mpcq_channel_params* ch) {
  if (!ch) return;
  memset(ch, 0, sizeof(*ch));
}

int mpcq_channel_observe_batch(mpcq_ctx* c, const mpcq_channel_params* ch, int64_t B, const int32_t* first,
                               int all_first, const double* truth, int32_t* clock, double* obs, double* draw,
                               double* s_ring, double* f_ring, uint32_t flags) {
  mpcq_channel_params P;
  int rc = channel_params(ch, &P);  // first: what is wrong with the parameters needs no context
  if (rc) return rc;
  rc = check_ctx(c, B);
  if (rc) return rc;
  if (!truth || !clock || !obs || !draw || !s_ring || !f_ring)
    return fail(MPCQ_E_INVALID, "truth, clock, obs, draw, s_ring and f_ring are required");
  if (B == 0) return MPCQ_OK;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  DeviceGuard g(c->device);
  mpcq::ObserveArgs a{};
  a.batch = B;
  a.all_first = all_first != 0;
  const size_t b = (size_t)B;
  enum { FI, TR, CL, OB, DR, SR, FR, NX };
  Xfer xs[NX] = {{first, nullptr, b * 4, nullptr},
                 {truth, nullptr, b * 96, nullptr},
                 {clock, clock, b * 8, nullptr},
                 {obs, obs, b * 96, nullptr},
                 {draw, draw, b * 128, nullptr},
                 {s_ring, s_ring, b * MPCQ_CHANNEL_MAX_DELAY * 96, nullptr},
                 {f_ring, f_ring, b * MPCQ_CHANNEL_MAX_LATENCY * 96, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.first = xs[FI]; a.truth = xs[TR]; a.clock = xs[CL]; a.obs = xs[OB]; a.draw = xs[DR]; a.s_ring = xs[SR];
  a.f_ring = xs[FR];
  HIP_TRY(mpcq::launch_observe(P, a, c->stream));
  return finish(c, xs, NX, flags);
}

int mpcq_channel_actuate_batch(mpcq_ctx* c, const mpcq_channel_params* ch, int64_t B, const double* f0,
                               const int32_t* clock, double* draw, double* f_ring, double* f_cmd, uint32_t flags) {
  mpcq_channel_params P;
  int rc = channel_params(ch, &P);
  if (rc) return rc;
  rc = check_ctx(c, B);
  if (rc) return rc;
  if (!f0 || !clock || !draw || !f_ring || !f_cmd)
    return fail(MPCQ_E_INVALID, "f0, clock, draw, f_ring and f_cmd are required");
  if (B == 0) return MPCQ_OK;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  DeviceGuard g(c->device);
  mpcq::ActuateArgs a{};
  a.batch = B;
  const size_t b = (size_t)B;
  enum { F0, CL, DR, FR, FC, NX };
  Xfer xs[NX] = {{f0, nullptr, b * 96, nullptr},
                 {clock, nullptr, b * 8, nullptr},
                 {draw, draw, b * 128, nullptr},
                 {f_ring, f_ring, b * MPCQ_CHANNEL_MAX_LATENCY * 96, nullptr},
                 {nullptr, f_cmd, b * 96, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.f0 = xs[F0]; a.clock = xs[CL]; a.draw = xs[DR]; a.f_ring = xs[FR]; a.f_cmd = xs[FC];
  HIP_TRY(mpcq::launch_actuate(P, a, c->stream));
  return finish(c, xs, NX, flags);
}

// Estimator: starting values, not tuned (include/mpcq.h).
void mpcq_default_estimator_params(mpcq_estimator_params* ep) {
  if (!ep) return;
  memset(ep, 0, sizeof(*ep));
  ep->skip_repeats = 1;
  for (int i = 0; i < 12; ++i) {
    ep->q[i] = i < 6 ? 1e-6 : 1e-4;
    ep->r[i] = 1e-4;
    ep->p0[i] = 1e-2;
  }
}

int mpcq_estimator_step_batch(mpcq_ctx* c, const mpcq_estimator_params* ep, int64_t B, const int32_t* first,
                              int all_first, const double* obs, const double* f_prev, const double* feet_prev,
                              const int32_t* failed_prev, const mpcq_robot* robots, double* row, double* est,
                              uint32_t flags) {
  mpcq_estimator_params P;
  int rc = estimator_params(ep, &P);  // first: what is wrong with the parameters needs no context
  if (rc) return rc;
  const size_t b = B > 0 ? (size_t)B : 0;
  Xfer xs[MI_NX + 2] = {};
  xs[MI_NX] = {row, row, b * MPCQ_EST_ROW * 8, nullptr};
  xs[MI_NX + 1] = {nullptr, est, b * 96, nullptr};
  mpcq::EstimateArgs a{};
  rc = model_inputs(c, B, first, all_first, "obs", obs, f_prev, feet_prev, failed_prev, robots, "est", flags, xs,
                    MI_NX + 2, &a);
  if (rc || B == 0) return rc;
  DeviceGuard g(c->device);
  a.row = xs[MI_NX]; a.est = xs[MI_NX + 1];
  HIP_TRY(mpcq::launch_estimate(P, a, c->stream));
  return finish(c, xs, MI_NX + 2, flags);
}

// Disturbance stage: starting values, not tuned (include/mpcq.h).
void mpcq_default_disturb_params(mpcq_disturb_params* dp) {
  if (!dp) return;
  memset(dp, 0, sizeof(*dp));
  for (int i = 0; i < 6; ++i) {
    dp->alpha[i] = 0.2;
    dp->d_max[i] = i < 3 ? 5.0 : 30.0;
  }
  dp->compensate = 1;
  dp->skip_repeats = 1;
}

int mpcq_disturb_step_batch(mpcq_ctx* c, const mpcq_disturb_params* dp, int64_t B, const int32_t* first,
                            int all_first, const double* meas, const double* f_prev, const double* feet_prev,
                            const int32_t* failed_prev, const mpcq_robot* robots, double* row,
                            mpcq_disturbance* dist, double* resid, uint32_t flags) {
  mpcq_disturb_params P;
  int rc = disturb_params(dp, &P);  // first: what is wrong with the parameters needs no context
  if (rc) return rc;
  const size_t b = B > 0 ? (size_t)B : 0;
  Xfer xs[MI_NX + 3] = {};
  xs[MI_NX] = {row, row, b * MPCQ_DIST_ROW * 8, nullptr};
  xs[MI_NX + 1] = {nullptr, dist, b * sizeof(mpcq_disturbance), nullptr};
  xs[MI_NX + 2] = {nullptr, resid, b * 48, nullptr};  // (optional: null stays null)
  mpcq::DisturbArgs a{};
  rc = model_inputs(c, B, first, all_first, "meas", meas, f_prev, feet_prev, failed_prev, robots, "dist", flags, xs,
                    MI_NX + 3, &a);
  if (rc || B == 0) return rc;
  DeviceGuard g(c->device);
  a.row = xs[MI_NX]; a.dist = xs[MI_NX + 1]; a.resid = xs[MI_NX + 2];
  HIP_TRY(mpcq::launch_disturb(P, a, c->stream));
  return finish(c, xs, MI_NX + 3, flags);
}

// Gait stage: requests by hand, switches at phase boundaries, no speed bands; yaw_weight = the
// distance of the default planner's shoulders (0.19, 0.15005) from the centre.
void mpcq_default_gait_params(mpcq_gait_params* gp) {
  if (!gp) return;
  memset(gp, 0, sizeof(*gp));
  gp->select = MPCQ_GAIT_MANUAL;
  gp->align = 1;
  for (int i = 0; i < MPCQ_GAIT_MAX - 1; ++i) gp->thresholds[i] = INFINITY;
  gp->yaw_weight = 0.2421053541332781;
}

int mpcq_gait_roll_batch(mpcq_ctx* c, const mpcq_gait_params* gp, const double* cycles, int64_t B,
                         const double* v_ref, double* gait, int32_t* gstate, uint32_t flags) {
  mpcq_gait_params P;
  mpcq::GaitArgs a{};
  int rc = gait_params(gp, cycles, &P, &a);  // first: what is wrong with the parameters needs no context
  if (rc) return rc;
  rc = check_ctx(c, B);
  if (rc) return rc;
  if (!gait || !gstate) return fail(MPCQ_E_INVALID, "gait and gstate are required");
  if (!v_ref && P.select == MPCQ_GAIT_BY_SPEED) return fail(MPCQ_E_INVALID, "v_ref is required with MPCQ_GAIT_BY_SPEED");
  if (B == 0) return MPCQ_OK;
  const bool dev = flags & MPCQ_FLAG_DEVICE_PTRS;
  DeviceGuard g(c->device);
  a.batch = B;
  const size_t b = (size_t)B;
  enum { VR, GA, GS, NX };
  Xfer xs[NX] = {{v_ref, nullptr, b * 48, nullptr}, {gait, gait, b * 800, nullptr}, {gstate, gstate, b * 16, nullptr}};
  rc = stage(c, xs, NX, dev);
  if (rc) return rc;
  a.v_ref = xs[VR]; a.gait = xs[GA]; a.gstate = xs[GS];
  HIP_TRY(mpcq::launch_gait(P, a, c->stream));
  return finish(c, xs, NX, flags);
}

int mpcq_debug_set_stamps(mpcq_ctx* c, void* buf) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  c->stamps = (uint64_t*)buf;
  return MPCQ_OK;
}

// The dispatch-order kernels on their own (include/mpcq.h "diagnostics"): host arrays staged
// through the arena, one launch, blocking.  None touches the scratch of the last solve.

int mpcq_debug_class_table_slots(void) { return mpcq::class_table_slots(); }

int mpcq_debug_suspended_status(void) { return mpcq::kStatusSuspended; }

int mpcq_debug_class_table_read(mpcq_ctx* c, uint64_t* sum, uint64_t* cnt) {
  if (!c || !sum || !cnt) return fail(MPCQ_E_INVALID, "NULL argument");
  DeviceGuard g(c->device);
  int rc = ensure_class_table(c);
  if (rc) return rc;
  const size_t tb = (size_t)mpcq::class_table_slots() * 8;
  HIP_TRY(hipMemcpyAsync(sum, c->cls_sum, tb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(cnt, c->cls_cnt, tb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

int mpcq_debug_class_table_write(mpcq_ctx* c, const uint64_t* sum, const uint64_t* cnt) {
  if (!c || !sum || !cnt) return fail(MPCQ_E_INVALID, "NULL argument");
  DeviceGuard g(c->device);
  int rc = ensure_class_table(c);
  if (rc) return rc;
  const size_t tb = (size_t)mpcq::class_table_slots() * 8;
  HIP_TRY(hipMemcpyAsync(c->cls_sum, sum, tb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->cls_cnt, cnt, tb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPCQ_OK;
}

int mpcq_debug_class_order(mpcq_ctx* c, int64_t B, const double* fsteps, int32_t* cls, int32_t* order) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (B < 1 || !fsteps || !cls || !order) return fail(MPCQ_E_INVALID, "batch >= 1 and every array are required");
  DeviceGuard g(c->device);
  rc = ensure_class_table(c);
  if (rc) return rc;
  Xfer xs[3] = {{fsteps, nullptr, (size_t)B * 260 * 8, nullptr}, {nullptr, cls, (size_t)B * 4, nullptr},
                {nullptr, order, (size_t)B * 4, nullptr}};
  rc = stage(c, xs, 3);
  if (rc) return rc;
  HIP_TRY(mpcq::launch_class_order((const double*)xs[0].dev, B, (int32_t*)xs[1].dev, c->cls_sum, c->cls_cnt,
                                   (int32_t*)xs[2].dev, c->stream));
  return unstage(c, xs, 3);
}

int mpcq_debug_class_learn(mpcq_ctx* c, int64_t B, const int32_t* cls, const int32_t* iters) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (B < 1 || !cls || !iters) return fail(MPCQ_E_INVALID, "batch >= 1 and every array are required");
  const int slots = mpcq::class_table_slots();
  for (int64_t i = 0; i < B; ++i)  // (the kernel indexes its LDS table by them)
    if (cls[i] < 0 || cls[i] >= slots) return fail(MPCQ_E_INVALID, "cls[%lld] = %d is no slot", (long long)i, cls[i]);
  DeviceGuard g(c->device);
  rc = ensure_class_table(c);
  if (rc) return rc;
  Xfer xs[2] = {{cls, nullptr, (size_t)B * 4, nullptr}, {iters, nullptr, (size_t)B * 4, nullptr}};
  rc = stage(c, xs, 2);
  if (rc) return rc;
  HIP_TRY(mpcq::launch_class_learn((const int32_t*)xs[0].dev, (const int32_t*)xs[1].dev, B, c->cls_sum, c->cls_cnt,
                                   c->stream));
  return unstage(c, xs, 2);
}

int mpcq_debug_suspended(mpcq_ctx* c, int64_t n, int64_t n_inst, const int32_t* prev, const int32_t* status,
                         const double* key, int32_t* list, int32_t* count) {
  int rc = check_ctx(c, n);
  if (!rc) rc = check_ctx(c, n_inst);
  if (rc) return rc;
  if (n < 1 || !status || !key || !list || !count) return fail(MPCQ_E_INVALID, "n >= 1 and every array but prev are required");
  if (!prev && n_inst < n) return fail(MPCQ_E_INVALID, "n_inst < n without prev");
  if (prev)  // (the kernel indexes status and key by them)
    for (int64_t i = 0; i < n; ++i)
      if (prev[i] < 0 || prev[i] >= n_inst) return fail(MPCQ_E_INVALID, "prev[%lld] = %d is no instance", (long long)i, prev[i]);
  DeviceGuard g(c->device);
  Xfer xs[5] = {{prev, nullptr, (size_t)n * 4, nullptr},
                {status, nullptr, (size_t)n_inst * 4, nullptr},
                {key, nullptr, (size_t)n_inst * 16, nullptr},
                {nullptr, list, (size_t)n * 4, nullptr},
                {nullptr, count, 4, nullptr}};
  rc = stage(c, xs, 5);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(xs[3].dev, 0xff, (size_t)n * 4, c->stream));  // (entries past the count: -1)
  HIP_TRY(mpcq::launch_suspended((const int32_t*)xs[0].dev, n, (const int32_t*)xs[1].dev, (const double*)xs[2].dev,
                                 (int32_t*)xs[3].dev, (int32_t*)xs[4].dev, nullptr, c->stream));
  return unstage(c, xs, 5);
}

int mpcq_debug_session_order(mpcq_ctx* c, int64_t B, const int32_t* iters, int32_t* order) {
  int rc = check_ctx(c, B);
  if (rc) return rc;
  if (B < 1 || !iters || !order) return fail(MPCQ_E_INVALID, "batch >= 1 and every array are required");
  DeviceGuard g(c->device);
  Xfer xs[2] = {{iters, nullptr, (size_t)B * 4, nullptr}, {nullptr, order, (size_t)B * 4, nullptr}};
  rc = stage(c, xs, 2);
  if (rc) return rc;
  HIP_TRY(mpcq::launch_order((const int32_t*)xs[0].dev, nullptr, B, (int32_t*)xs[1].dev, c->stream));
  return unstage(c, xs, 2);
}

int mpcq_debug_last_dispatch(mpcq_ctx* c, int64_t* batch, int32_t* sliced, int32_t* by_class, int32_t* cls,
                             int32_t* order, int32_t* list, int32_t* count, double* key) {
  if (!c) return fail(MPCQ_E_INVALID, "ctx is NULL");
  DeviceGuard g(c->device);
  const int64_t B = c->last_B;
  if (batch) *batch = B;
  if (sliced) *sliced = c->last_sliced;
  if (by_class) *by_class = c->last_by_class;
  if (count) *count = 0;
  if (B < 1) return MPCQ_OK;
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (c->last_by_class) {  // (solve_common: ord_buf = the slots, then the order)
    if (cls) HIP_TRY(hipMemcpyAsync(cls, c->ord_buf, (size_t)B * 4, d2h, c->stream));
    if (order) HIP_TRY(hipMemcpyAsync(order, c->ord_buf + B, (size_t)B * 4, d2h, c->stream));
  }
  int32_t cnt = 0;
  if (c->last_sliced) {
    HIP_TRY(hipMemcpyAsync(&cnt, c->sl_count, 4, d2h, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (cnt < 0 || cnt > B) return fail(MPCQ_E_DEVICE, "the suspended count %d is outside 0..%lld", cnt, (long long)B);
    if (list && cnt) HIP_TRY(hipMemcpyAsync(list, c->sl_buf, (size_t)cnt * 4, d2h, c->stream));
    if (key) HIP_TRY(hipMemcpyAsync(key, c->res_key, (size_t)B * 16, d2h, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (list)
    for (int64_t i = cnt; i < B; ++i) list[i] = -1;
  if (count) *count = cnt;
  return MPCQ_OK;
}

}  // extern "C"
