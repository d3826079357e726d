// mpcq_session_layout.cpp — the table of a session's parts and the snapshot blob's header
// (mpcq_session_layout.h).
#include "mpcq_session_layout.h"

#include <stdio.h>
#include <string.h>

namespace mpcq {

namespace {

// Bytes of the arrays of each part (layouts: include/mpcq.h).
constexpr size_t main_bytes(int w, size_t b, int N, int) {
  switch (w) {
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
  return 0;  // (the swing ids: the swing part's arrays, from mpcq_session_enable_swing on)
}
constexpr size_t swing_bytes(int w, size_t B, int, int k_mpc) {  // MPCQ_SV_SWING_REF, _SWING_STATE, _FRAME
  const size_t m[3] = {B * k_mpc * 36 * 8, B * 4 * MPCQ_SWING_STATE * 8, B * 24};
  return m[w];
}
constexpr size_t plant_bytes(int w, size_t B, int, int) {  // STATE_END, F_EFF, WRENCH, qw_prev
  const size_t m[PP_COUNT] = {B * 96, B * 96, B * 48, B * 48};
  return m[w];
}
constexpr size_t monitor_bytes(int w, size_t B, int, int) {  // DONE, EP, EP_TICKS, EPISODES, LAST, TOTALS
  const size_t m[MPCQ_MV_COUNT] = {B * 4, B * 64, B * 4, B * 4, B * 128, 64};
  return m[w];
}
constexpr size_t scenario_bytes(int w, size_t B, int, int) {  // EPOCH, TICK, V_REF, PUSH, WRENCH, ROBOTS, DRAW
  const size_t m[MPCQ_CV_COUNT] = {B * 4, B * 4, B * 48, B * 48, B * 48, B * sizeof(mpcq_robot), B * 64};
  return m[w];
}
constexpr size_t table_bytes(int, size_t B, int, int) { return B * sizeof(mpcq_robot); }
constexpr size_t channel_bytes(int w, size_t B, int, int) {  // CLOCK, OBS, F_CMD, DRAW, S_RING, F_RING
  const size_t m[MPCQ_HV_COUNT] = {B * 8, B * 96, B * 96, B * 128, B * MPCQ_CHANNEL_MAX_DELAY * 96,
                                   B * MPCQ_CHANNEL_MAX_LATENCY * 96};
  return m[w];
}
constexpr size_t estimator_bytes(int w, size_t B, int, int) {  // EST, ROW
  const size_t m[MPCQ_EV_COUNT] = {B * 96, B * MPCQ_EST_ROW * 8};
  return m[w];
}
constexpr size_t gait_bytes(int, size_t B, int, int) { return B * 16; }  // STATE
constexpr size_t disturb_bytes(int w, size_t B, int, int) {  // DIST, ROW, RESID
  const size_t m[MPCQ_DV_COUNT] = {B * sizeof(mpcq_disturbance), B * MPCQ_DIST_ROW * 8, B * 48};
  return m[w];
}

constexpr uint32_t bit(int w) { return 1u << w; }
constexpr uint32_t all(int n) { return (1u << n) - 1u; }
constexpr size_t group_bytes_at(int gi) { return offsetof(BlobHeader, group_bytes) + 8 * (size_t)gi; }
// The main part's arrays a snapshot holds: not the staging of host inputs (every tick rewrites it
// before reading), not MPCQ_SV_ORDER (a permutation: rebuilt, never copied by rows), not the
// swing ids (a part of their own).
constexpr uint32_t kMainHeld = all(SP_COUNT) & ~(bit(MPCQ_SV_ORDER) | bit(MPCQ_SV_SWING_REF) | bit(MPCQ_SV_SWING_STATE) |
                                                 bit(MPCQ_SV_FRAME) | bit(SP_IN_STATE) | bit(SP_IN_LFEET) |
                                                 bit(SP_IN_VREF) | bit(SP_IN_REDUCED) | bit(SP_IN_GAIT));

}  // namespace

// Not held besides: PP_QW_PREV (a tick with the plant takes it before its retrieve), MPCQ_EV_EST,
// MPCQ_DV_DIST and MPCQ_DV_RESID (derived: every tick rewrites them before anything reads them).
constexpr Part kParts[G_COUNT] = {
    {"session", "swing", "the session", "the snapshot's session arrays", nullptr,
     MPCQ_SV_COUNT, SP_COUNT, main_bytes, kMainHeld, all(SP_COUNT), 0, 1, group_bytes_at(G_MAIN), -1, 0},
    {"swing", "swing", "the swing arrays", "the snapshot's swing arrays", "the swing arrays exist on one side only",
     0, 3, swing_bytes, all(3), all(3), 4, 1, group_bytes_at(G_SWING), G_MAIN, MPCQ_SV_SWING_REF},
    {"plant", "plant", "the plant arrays", "the snapshot's plant arrays", "the plant arrays exist on one side only",
     MPCQ_PV_COUNT, PP_COUNT, plant_bytes, all(MPCQ_PV_COUNT), all(PP_COUNT), 8, 1, group_bytes_at(G_PLANT), -1, 0},
    {"monitor", "monitor", "the monitor arrays", "the snapshot's monitor arrays",
     "the monitor arrays exist on one side only",
     MPCQ_MV_COUNT, MPCQ_MV_COUNT, monitor_bytes, all(MPCQ_MV_COUNT), all(MPCQ_MV_COUNT) & ~bit(MPCQ_MV_TOTALS), 16, 1,
     group_bytes_at(G_MONITOR), -1, 0},
    {"scenario", "scenario", "the scenario arrays", "the snapshot's scenario arrays",
     "the scenario arrays exist on one side only",
     MPCQ_CV_COUNT, MPCQ_CV_COUNT, scenario_bytes, all(MPCQ_CV_COUNT), all(MPCQ_CV_COUNT), 32, 1,
     group_bytes_at(G_SCENARIO), -1, 0},
    {"robots table", "robots", "the robots table", "the snapshot's robots table",
     "the robots table is in force on one side only",
     0, 1, table_bytes, 1, 1, 64, 1, group_bytes_at(G_ROBOTS), -1, 0},
    {"plant robots table", "plant_robots", "the plant robots table", "the snapshot's plant robots table",
     "the plant robots table is in force on one side only",
     0, 1, table_bytes, 1, 1, 128, 1, group_bytes_at(G_PLANT_ROBOTS), -1, 0},
    {"channel", "channel", "the channel arrays", "the snapshot's channel arrays",
     "the channel arrays exist on one side only",
     MPCQ_HV_COUNT, MPCQ_HV_COUNT, channel_bytes, all(MPCQ_HV_COUNT), all(MPCQ_HV_COUNT), 256, 2,
     offsetof(BlobHeader, channel_bytes), -1, 0},
    {"estimator", "estimator", "the estimator arrays", "the snapshot's estimator row",
     "the estimator arrays exist on one side only",
     MPCQ_EV_COUNT, MPCQ_EV_COUNT, estimator_bytes, bit(MPCQ_EV_ROW), all(MPCQ_EV_COUNT), 512, 3,
     offsetof(BlobHeader, estimator_bytes), -1, 0},
    {"gait", "gait", "the gait array", "the snapshot's gait rows", "the gait arrays exist on one side only",
     MPCQ_GV_COUNT, MPCQ_GV_COUNT, gait_bytes, all(MPCQ_GV_COUNT), all(MPCQ_GV_COUNT), 1024, 4,
     offsetof(BlobHeader, gait_bytes), -1, 0},
    {"disturb", "disturb", "the disturb arrays", "the snapshot's disturb rows",
     "the disturb arrays exist on one side only",
     MPCQ_DV_COUNT, MPCQ_DV_COUNT, disturb_bytes, bit(MPCQ_DV_ROW), all(MPCQ_DV_COUNT), 2048, 5,
     offsetof(BlobHeader, disturb_bytes), -1, 0},
};

static_assert(sizeof(BlobHeader) == 160 && offsetof(BlobHeader, gait_bytes) == 128 &&
                  offsetof(BlobHeader, disturb_bytes) == 144 && G_CHANNEL == 7 && G_ESTIMATOR == 8 && G_GAIT == 9 &&
                  G_DISTURB == 10 && G_COUNT == 11,
              "the blob's header is 128 bytes, 144 in format version 4, 160 from version 5 on");
static_assert(SP_COUNT <= 32, "a part's masks are 32 bits");

void part_sizes(int gi, size_t B, int N, int k_mpc, bool held_only, size_t nb[kPartArrays]) {
  const Part& p = kParts[gi];
  for (int w = 0; w < kPartArrays; ++w)
    nb[w] = w < p.count && (!held_only || (p.held >> w & 1u)) ? p.bytes(w, B, N, k_mpc) : 0;
}

void snap_sizes(const SnapShape& sh, int N, size_t nb[G_COUNT][kPartArrays]) {
  memset(nb, 0, sizeof(size_t) * G_COUNT * kPartArrays);
  for (int gi = 0; gi < G_COUNT; ++gi)
    if (sh.has[gi]) part_sizes(gi, (size_t)sh.B, N, sh.k_mpc, true, nb[gi]);
}

const char* shape_difference(const SnapShape& a, const SnapShape& b, bool batch_too) {
  if (batch_too && a.B != b.B) return "the batch sizes differ (a restore without a map needs the same batch)";
  for (int gi = 0; gi < G_COUNT; ++gi) {
    if (a.has[gi] != b.has[gi]) return kParts[gi].one_side;
    // the parameters a part's arrays were filled under, behind the part
    if (gi == G_SWING && a.k_mpc != b.k_mpc) return "the swing k_mpc differs";
    if (gi == G_CHANNEL && a.delay != b.delay) return "the channel's delay differs (the rings were filled under another)";
    if (gi == G_CHANNEL && a.latency != b.latency)
      return "the channel's latency differs (the rings were filled under another)";
    if (gi == G_GAIT && a.n_gaits != b.n_gaits) return "the gait library sizes differ (the rows index another library)";
  }
  return nullptr;
}

size_t header_bytes(uint32_t version) {
  return version >= 5 ? sizeof(BlobHeader) : version == 4 ? offsetof(BlobHeader, disturb_bytes)
                                                          : offsetof(BlobHeader, gait_bytes);
}

int64_t& part_bytes(BlobHeader& h, int gi) { return *(int64_t*)((char*)&h + kParts[gi].header); }

namespace {

const char kMagic[8] = {'M', 'P', 'C', 'Q', 'S', 'N', 'P', '1'};
constexpr uint32_t kHaveOrder = 1u, kResets = 2u;  // the flags bits below the parts'

// The format version a set of parts forces, and the set as flags.
uint32_t version_of(const bool has[G_COUNT]) {
  uint32_t v = 1;
  for (int gi = 0; gi < G_COUNT; ++gi)
    if (has[gi] && kParts[gi].version > v) v = kParts[gi].version;
  return v;
}

}  // namespace

void blob_header(const SnapShape& sh, int N, bool have_order, bool resets, BlobHeader* h) {
  size_t nb[G_COUNT][kPartArrays];
  snap_sizes(sh, N, nb);
  memset(h, 0, sizeof(*h));
  memcpy(h->magic, kMagic, 8);
  h->version = version_of(sh.has); h->N = N; h->B = sh.B; h->k_mpc = sh.k_mpc;
  h->flags = (have_order ? kHaveOrder : 0u) | (resets ? kResets : 0u);
  h->delay = sh.delay; h->latency = sh.latency;
  h->n_gaits = sh.n_gaits;
  h->total = (int64_t)header_bytes(h->version);
  for (int gi = 0; gi < G_COUNT; ++gi) {
    if (sh.has[gi]) h->flags |= kParts[gi].flag;
    int64_t& gb = part_bytes(*h, gi);
    for (int w = 0; w < kPartArrays; ++w) gb += (int64_t)nb[gi][w];
    h->total += gb;
  }
}

bool parse_blob_header(const void* src, int64_t bytes, int N, SnapShape* sh, bool* have_order, bool* resets,
                       char* msg, size_t msg_bytes) {
#define REFUSE(...) return snprintf(msg, msg_bytes, __VA_ARGS__), false
  BlobHeader h;
  memset(&h, 0, sizeof(h));
  if (bytes < (int64_t)header_bytes(1)) REFUSE("%lld bytes are less than a header", (long long)bytes);
  memcpy(&h, src, header_bytes(1));
  if (memcmp(h.magic, kMagic, 8) != 0) REFUSE("not a snapshot blob (magic)");
  if (h.version < 1 || h.version > 5) REFUSE("blob format version %u, this library reads 1 to 5", h.version);
  if (bytes < (int64_t)header_bytes(h.version))
    REFUSE("%lld bytes are less than a version-%u header", (long long)bytes, h.version);
  memcpy(&h, src, header_bytes(h.version));
  if (h.N != N) REFUSE("the blob is of a context with N = %d, this one has N = %d", h.N, N);
  SnapShape s;
  uint32_t known = kHaveOrder | kResets;
  for (int gi = 0; gi < G_COUNT; ++gi) {
    s.has[gi] = !kParts[gi].flag || (h.flags & kParts[gi].flag);
    known |= kParts[gi].flag;
  }
  // the fields beside the byte counts: in range where their part is there, zero where it is not
  const bool swing_ok = s.has[G_SWING] == (h.k_mpc > 0);
  const bool channel_ok = s.has[G_CHANNEL] ? h.delay >= 0 && h.delay <= MPCQ_CHANNEL_MAX_DELAY && h.latency >= 0 &&
                                                 h.latency <= MPCQ_CHANNEL_MAX_LATENCY
                                           : h.delay == 0 && h.latency == 0 && h.channel_bytes == 0;
  const bool estimator_ok = s.has[G_ESTIMATOR] || h.estimator_bytes == 0;
  const bool gait_ok = h.pad == 0 && (s.has[G_GAIT] ? h.n_gaits >= 1 && h.n_gaits <= MPCQ_GAIT_MAX : h.n_gaits == 0);
  if (h.B < 1 || h.B > (int64_t)0x7fffffff || h.k_mpc < 0 || h.k_mpc > 65536 || (h.flags & ~known) || !swing_ok ||
      h.version != version_of(s.has) || !estimator_ok || !gait_ok || h.pad5 != 0 || !channel_ok)
    REFUSE("the blob's header is inconsistent (B %lld, k_mpc %d, flags %#x)", (long long)h.B, h.k_mpc, h.flags);
  s.B = h.B; s.k_mpc = h.k_mpc;
  s.delay = h.delay; s.latency = h.latency;
  s.n_gaits = h.n_gaits;
  BlobHeader want;
  blob_header(s, N, h.flags & kHaveOrder, h.flags & kResets, &want);
  for (int gi = 0; gi < G_COUNT; ++gi) {
    const int64_t have = part_bytes(h, gi), need = part_bytes(want, gi);
    if (have != need)
      REFUSE("the blob's part %d has %lld bytes, its shape says %lld", gi, (long long)have, (long long)need);
  }
  if (h.total != want.total || bytes != want.total)
    REFUSE("the blob says %lld bytes, its shape %lld, the caller %lld (truncated?)", (long long)h.total,
           (long long)want.total, (long long)bytes);
#undef REFUSE
  *sh = s;
  *have_order = h.flags & kHaveOrder;
  *resets = h.flags & kResets;
  return true;
}

}  // namespace mpcq
