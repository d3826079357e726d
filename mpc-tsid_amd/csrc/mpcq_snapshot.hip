// mpcq_snapshot.hip — the row gather behind mpcq_session_snapshot_restore / mpcq_session_fork
// on MI355X: robot b of a session takes row map[b] of every per-robot array of a snapshot, in
// one launch however many arrays there are (include/mpcq.h).  No reference
// counterpart: the reference runs one robot forward.
//
// The arrays' table (source base, destination base, row bytes, access width) travels in the
// kernel arguments, the wide arrays first.  The grid has two parts:
//   blocks [0, ceil(rows_dst / 4)): one wave64 per destination robot.  The wave walks the wide
//     arrays' rows (more than kGatherNarrow bytes: 48 B .. 5.6 KB here) in steps of 64 accesses
//     of the array's width.  The host sorts the wide arrays by width (16 B wherever row size and
//     bases allow, then 8, then 4) and the wave runs one loop per width, the width a template
//     parameter: every access is one instruction of that width.  A loop loads kInFlight steps
//     before it stores the first, across array boundaries: a wave keeps that many rows or row
//     parts in flight.
//   the blocks behind them: one lane per destination robot over consecutive b, for the narrow
//     arrays (4 .. 32 B per robot): a wave's stores to an array are one contiguous run, where a
//     wave per robot would issue one 4-byte access per array.  These lanes also set first[b].
// A robot whose map entry is outside [0, rows_src), or b >= rows_dst, touches nothing: no
// address is formed from such an entry.  Plain vector loads and stores; no LDS, no atomics.
#include <stdint.h>

#include "mpcq_internal.h"

namespace mpcq {
namespace {

constexpr int kInFlight = 4;  // wave steps loaded before the first store
// the access widths as native vectors (a local array of them stays in registers)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// The source row of destination robot b, or -1: nothing to do.
__device__ __forceinline__ int64_t source_row(const GatherArgs& a, int64_t b) {
  if (b >= a.rows_dst) return -1;
  const int64_t r = a.map ? (int64_t)a.map[b] : b;
  return r >= 0 && r < a.rows_src ? r : -1;
}

// The wide arrays d[lo .. hi) of one access width (T: u32x4, u32x2 or uint32_t), row r -> row b.
template <class T>
__device__ __forceinline__ void walk_wide(const GatherArgs& a, int lo, int hi, int64_t r, int64_t b, int lane) {
  int arr = lo, c = 0;  // the next step: pieces c .. c + 63 of array arr (wave-uniform)
  while (arr < hi) {
    // Every step loads without a branch around it, so that the four loads issue back to back: a
    // lane past the row's end, or a step past the last array, re-reads the last piece of the
    // step's row (an address inside the row; the line is in flight anyway) and stores nothing.
    T v[kInFlight];
    T* q[kInFlight];
    GatherDesc d = a.d[arr];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const bool step = arr < hi;
      if (step) d = a.d[arr];
      const int pieces = d.row_bytes / (int)sizeof(T);
      const int i = c + lane;
      const int j = i < pieces ? i : pieces - 1;
      v[u] = ((const T*)((const char*)d.src + r * d.row_bytes))[j];
      q[u] = step && i < pieces ? (T*)((char*)d.dst + b * d.row_bytes) + j : nullptr;
      c += 64;
      if (step && c >= pieces) {
        ++arr;
        c = 0;
      }
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u)
      if (q[u]) *q[u] = v[u];
  }
}

// One narrow row by one lane.
template <class T>
__device__ __forceinline__ void copy_row(const void* sp, void* dp, int row_bytes) {
  for (int i = 0; i < row_bytes / (int)sizeof(T); ++i) ((T*)dp)[i] = ((const T*)sp)[i];
}

__global__ __launch_bounds__(256) void gather_rows_kernel(GatherArgs a, unsigned wide_blocks) {
  if (blockIdx.x < wide_blocks) {
    // ---- one wave per destination robot: the wide rows, by access width
    const int lane = threadIdx.x & 63;
    const int64_t b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const int64_t r = source_row(a, b);
    if (r < 0) return;
    walk_wide<u32x4>(a, 0, a.n_wide16, r, b, lane);
    walk_wide<u32x2>(a, a.n_wide16, a.n_wide8, r, b, lane);
    walk_wide<uint32_t>(a, a.n_wide8, a.n_wide, r, b, lane);
    return;
  }
  // ---- one lane per destination robot: the narrow rows and the first flag
  const int64_t b = (int64_t)(blockIdx.x - wide_blocks) * 256 + threadIdx.x;
  const int64_t r = source_row(a, b);
  if (r < 0) return;
  for (int arr = a.n_wide; arr < a.n; ++arr) {
    const GatherDesc d = a.d[arr];
    const char* sp = (const char*)d.src + r * d.row_bytes;
    char* dp = (char*)d.dst + b * d.row_bytes;
    if (d.vec == 16) copy_row<u32x4>(sp, dp, d.row_bytes);
    else if (d.vec == 8) copy_row<u32x2>(sp, dp, d.row_bytes);
    else copy_row<uint32_t>(sp, dp, d.row_bytes);
  }
  if (a.first) a.first[b] = 1;
}

}  // namespace

int gather_vec(const void* src, const void* dst, int64_t row_bytes) {
  const uint64_t bits = (uint64_t)(uintptr_t)src | (uint64_t)(uintptr_t)dst | (uint64_t)row_bytes;
  return bits % 16 == 0 ? 16 : bits % 8 == 0 ? 8 : bits % 4 == 0 ? 4 : 0;
}

hipError_t launch_gather_rows(const GatherArgs& a, hipStream_t s) {
  if (a.rows_dst <= 0 || a.rows_src <= 0) return hipSuccess;
  if (a.rows_dst > INT32_MAX - 4 || a.rows_src > INT32_MAX) return hipErrorInvalidValue;
  if (a.n < 0 || a.n > kGatherMax || a.n_wide16 < 0 || a.n_wide16 > a.n_wide8 || a.n_wide8 > a.n_wide ||
      a.n_wide > a.n)
    return hipErrorInvalidValue;
  for (int i = 0; i < a.n; ++i) {
    const GatherDesc& d = a.d[i];
    if (!d.src || !d.dst || d.row_bytes < 4 || d.vec == 0 || (i < a.n_wide) != (d.row_bytes > kGatherNarrow) ||
        d.vec != gather_vec(d.src, d.dst, d.row_bytes))
      return hipErrorInvalidValue;
    if (i < a.n_wide && d.vec != (i < a.n_wide16 ? 16 : i < a.n_wide8 ? 8 : 4)) return hipErrorInvalidValue;
  }
  const unsigned wide = a.n_wide ? (unsigned)((a.rows_dst + 3) / 4) : 0u;
  const unsigned narrow = (a.n > a.n_wide || a.first) ? (unsigned)((a.rows_dst + 255) / 256) : 0u;
  if (wide + narrow == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(wide + narrow), dim3(256), 0, s, a, wide);
  return hipGetLastError();
}

}  // namespace mpcq
