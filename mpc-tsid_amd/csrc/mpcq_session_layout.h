// mpcq_session_layout.h — the array groups of a session, once: what each part of a session (and
// of a snapshot, and of a snapshot's blob) is called, which arrays it has and how large they are,
// which of them a snapshot holds, and where the blob's header says so.  No HIP: the unit builds
// and runs on a machine without a GPU (tests/host/session_layout_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mpcq.h"

namespace mpcq {

// The parts, in the blob's order; each is one allocation.
enum { G_MAIN, G_SWING, G_PLANT, G_MONITOR, G_SCENARIO, G_ROBOTS, G_PLANT_ROBOTS, G_CHANNEL, G_ESTIMATOR,
       G_GAIT, G_DISTURB, G_COUNT };

// Private arrays, behind the named ones of their part: the warm start, the planner's status, the
// engine's info, the staging of host inputs (tick: state, l_feet, v_ref, reduced; reset: mask in
// IN_REDUCED, q_w0 in IN_VREF, gait0 in IN_GAIT), the gait table every robot was created with;
// the copy of q_w a tick with the plant takes before its retrieve.
enum { SP_WARM_X = MPCQ_SV_COUNT, SP_PLAN_STATUS, SP_INFO, SP_IN_STATE, SP_IN_LFEET, SP_IN_VREF, SP_IN_REDUCED,
       SP_GAIT_INIT, SP_IN_GAIT, SP_COUNT };
enum { PP_QW_PREV = MPCQ_PV_COUNT, PP_COUNT };
constexpr int kPartArrays = SP_COUNT;  // the arrays of the widest part

// What a snapshot's allocations follow from, with the context's N.
struct SnapShape {
  int64_t B = 0;
  int k_mpc = 0;               // of the swing arrays (0 without)
  int delay = 0, latency = 0;  // the depths the channel's rings were primed under
  int n_gaits = 0;             // the cycles of the library the gait rows index (the library itself is not held)
  bool has[G_COUNT] = {};      // the parts that exist (G_MAIN: always)
};

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
  int64_t channel_bytes;    // format version 2: the eighth part,
  int32_t delay, latency;   // and the depths its rings were filled under
  int64_t estimator_bytes;  // format version 3: the ninth part
  // format version 4 only, behind the 128 bytes of versions 1 to 3: the tenth part and the size
  // of the library its rows index
  int64_t gait_bytes;
  int32_t n_gaits, pad;
  // format version 5 only, behind the 144 bytes of version 4: the eleventh part
  int64_t disturb_bytes;
  int64_t pad5;
};

// One part.  Masks have bit w for array w.
struct Part {
  const char *kind, *enable;  // "<kind> array %d needs mpcq_session_enable_<enable>"
  const char *live, *snap;    // what an allocation failure calls it, in a session and in a snapshot
  const char* one_side;       // what a restore across sessions that differ in it answers
  int named;                  // the ids the _read / _write / _device_ptr entry points reach
  int count;                  // all arrays, the private ones included
  size_t (*bytes)(int w, size_t B, int N, int k_mpc);  // of array w in a session
  uint32_t held;              // the arrays a snapshot holds
  uint32_t rows;              // the arrays with one row per robot (a mapped restore gathers them)
  uint32_t flag;              // the blob's flags bit (0: always there)
  uint32_t version;           // the least blob format version with this part
  size_t header;              // offset of its byte count in BlobHeader
  int alias, alias_at;        // its arrays are also ids alias_at, alias_at + 1, ... of part `alias` (-1: no)
};
extern const Part kParts[G_COUNT];

// Bytes of every array of part gi in a session (held_only: in a snapshot; 0: not held).
void part_sizes(int gi, size_t B, int N, int k_mpc, bool held_only, size_t nb[kPartArrays]);
// Bytes of every array of every part of a snapshot of this shape (0: not held).
void snap_sizes(const SnapShape& sh, int N, size_t nb[G_COUNT][kPartArrays]);
// The first difference between a snapshot's shape and a session's, as text; or null.
const char* shape_difference(const SnapShape& a, const SnapShape& b, bool batch_too);

size_t header_bytes(uint32_t version);
int64_t& part_bytes(BlobHeader& h, int gi);
void blob_header(const SnapShape& sh, int N, bool have_order, bool resets, BlobHeader* h);
// Everything an import checks before it touches the device: the shape and flags the blob of
// `bytes` bytes at src describes for a context of horizon N (true), or the refusal's text in msg.
bool parse_blob_header(const void* src, int64_t bytes, int N, SnapShape* sh, bool* have_order, bool* resets,
                       char* msg, size_t msg_bytes);

}  // namespace mpcq
