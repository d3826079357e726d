// mpcq_engine_lanes.h — the engine's lane primitives: address-space views, DPP moves and
// broadcasts, broadcast dot products, gathers, row / pair / wave reductions, value holds and
// uniform pointers.  Device code (gfx950), included by mpcq_engine.hip alone.
#pragma once
#include <utility>

#include "mpcq_engine_layout.h"

namespace mpcq {
namespace {

// LDS views used by the loops.  Reads of loop-invariant data (the scaled A,
// the sweep matrices) go through these pointers, which the loops launder with
// an empty asm so the compiler re-reads LDS instead of hoisting dozens of
// invariant values into registers.
typedef __attribute__((address_space(3))) const double lds_cd;
typedef __attribute__((address_space(3))) double lds_d;
typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const dbl2 lds_cd2;
// the per-instance workspace (N > 32) in the global address space: generic (flat)
// loads would also count in lgkmcnt, so every LDS wait behind them would wait for L2
typedef __attribute__((address_space(1))) const double g_cd;
typedef __attribute__((address_space(1))) double g_d;
typedef __attribute__((address_space(1))) const dbl2 g_cd2;

// ---------------------------------------------------------------------------
// cross-lane helpers

__device__ __forceinline__ void wave_sync() {
  // LDS is processed in order per wave, so a hand-off inside one wave needs no
  // hardware barrier; the asm memory clobber stops the compiler from moving
  // LDS accesses across this point.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void sync_all() { __syncthreads(); }

template <int CTRL>
__device__ __forceinline__ double dppd(double v) {
  // one v_mov_b64_dpp for row_newbcast (DPP64); other controls split in two.
  // Every lane of every row is active wherever these run, so no "old" value.
  return __longlong_as_double(__builtin_amdgcn_mov_dpp(__double_as_longlong(v), CTRL, 0xF, 0xF, false));
}
// broadcast lane J of each 16-lane row (DPP row_newbcast, gfx90a+)
template <int J>
__device__ __forceinline__ double rbc(double v) { return dppd<0x150 + J>(v); }
// broadcast lane J of each quad (quad_perm J,J,J,J)
template <int J>
__device__ __forceinline__ double qbc(double v) { return dppd<85 * J>(v); }
// lane i of each quad takes the quad's lane Ji (quad_perm [J0, J1, J2, J3]): a select between
// quad broadcasts on the lane's place in its quad, as one move
template <int J0, int J1, int J2, int J3>
__device__ __forceinline__ double qperm(double v) { return dppd<J0 + 4 * J1 + 16 * J2 + 64 * J3>(v); }

// Every element of a[] in a register at one point: one empty asm reads and redefines them
// all, so the loads that produce them are all issued ahead of it and waited for once.  Left
// to itself the compiler put some of the check's LDS reads one behind the other through the
// same registers, each with its own s_waitcnt lgkmcnt(0) in front of its use (N = 16: twelve
// round trips in a row in the residuals' primal side).  Values and
// arithmetic are untouched.
#define MPCQ_HV(i) "+v"(a[i])
#define MPCQ_HV4(i) MPCQ_HV(i), MPCQ_HV(i + 1), MPCQ_HV(i + 2), MPCQ_HV(i + 3)
template <int n>
__device__ __forceinline__ void hold_all(double (&a)[n]) {
  static_assert((n >= 1 && n <= 8) || n == 15 || n == 21, "hold_all: spell this count out");
  if constexpr (n == 1) asm volatile("" : MPCQ_HV(0));
  if constexpr (n == 2) asm volatile("" : MPCQ_HV(0), MPCQ_HV(1));
  if constexpr (n == 3) asm volatile("" : MPCQ_HV(0), MPCQ_HV(1), MPCQ_HV(2));
  if constexpr (n == 4) asm volatile("" : MPCQ_HV4(0));
  if constexpr (n == 5) asm volatile("" : MPCQ_HV4(0), MPCQ_HV(4));
  if constexpr (n == 6) asm volatile("" : MPCQ_HV4(0), MPCQ_HV(4), MPCQ_HV(5));
  if constexpr (n == 7) asm volatile("" : MPCQ_HV4(0), MPCQ_HV(4), MPCQ_HV(5), MPCQ_HV(6));
  if constexpr (n == 8) asm volatile("" : MPCQ_HV4(0), MPCQ_HV4(4));
  if constexpr (n == 15) asm volatile("" : MPCQ_HV4(0), MPCQ_HV4(4), MPCQ_HV4(8), MPCQ_HV(12), MPCQ_HV(13), MPCQ_HV(14));
  if constexpr (n == 21) asm volatile("" : MPCQ_HV4(0), MPCQ_HV4(4), MPCQ_HV4(8), MPCQ_HV4(12), MPCQ_HV4(16), MPCQ_HV(20));
}
#undef MPCQ_HV4
#undef MPCQ_HV

// i0 + sum_{j<12} g_j * v_j, v_j broadcast from lane j of the row (v_fmac_f64_dpp).
// One dependent chain: the fmac issue interval exceeds its latency.  s_nop 1: a VALU
// write of v then a DPP read of it needs two wait states.
__device__ __forceinline__ double bdot12(const double (&g)[12], double v, double i0) {
  double a0 = i0;
  asm volatile("s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %5 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %6 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %7 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %8 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %9 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %10 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %11 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %12 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %13 row_newbcast:11 row_mask:0xf bank_mask:0xf"
      : "+v"(a0)
      : "v"(v), "v"(g[0]), "v"(g[1]), "v"(g[2]), "v"(g[3]), "v"(g[4]), "v"(g[5]), "v"(g[6]), "v"(g[7]),
        "v"(g[8]), "v"(g[9]), "v"(g[10]), "v"(g[11]));
  return a0;
}
// i0 + sum_psi g_psi * v(lane LN(psi)) over a stage's 12 force / state slots, the
// broadcasts folded into v_fmac_f64_dpp (one chain; s_nop 1 covers the DPP read hazard).
__device__ __forceinline__ double bdot_ln12(const double (&g)[12], double v, double i0) {
  double a0 = i0;
  asm("s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %5 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %6 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %7 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %8 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %9 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %10 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %11 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %12 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %13 row_newbcast:14 row_mask:0xf bank_mask:0xf"
      : "+v"(a0)
      : "v"(v), "v"(g[0]), "v"(g[1]), "v"(g[2]), "v"(g[3]), "v"(g[4]), "v"(g[5]), "v"(g[6]), "v"(g[7]),
        "v"(g[8]), "v"(g[9]), "v"(g[10]), "v"(g[11]));
  return a0;
}
// i0 + sum_{j<6} g_j * v_j, v_j broadcast from lane j of the row: half of a
// 12-term row product (the split sweep, ph_sweep)
__device__ __forceinline__ double bdot6(const double (&g)[6], double v, double i0) {
  double a0 = i0;
  asm volatile("s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %5 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %6 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %7 row_newbcast:5 row_mask:0xf bank_mask:0xf"
      : "+v"(a0)
      : "v"(v), "v"(g[0]), "v"(g[1]), "v"(g[2]), "v"(g[3]), "v"(g[4]), "v"(g[5]));
  return a0;
}
// i0 + sum_i g_i * v(lane LN(6 + i)), i < 6: the velocity slots
__device__ __forceinline__ double bdot_ln6v(const double (&g)[6], double v, double i0) {
  double a0 = i0;
  asm("s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %1, %2 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %3 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %4 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %5 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %6 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %0, %1, %7 row_newbcast:14 row_mask:0xf bank_mask:0xf"
      : "+v"(a0)
      : "v"(v), "v"(g[0]), "v"(g[1]), "v"(g[2]), "v"(g[3]), "v"(g[4]), "v"(g[5]));
  return a0;
}
// (a + b) * m, rounded as the two C operations, issued where the statement stands relative
// to the other volatile asm blocks (the sweeps' chains)
__device__ __forceinline__ double add_mul_here(double a, double b, double m) {
  double r;
  asm volatile("v_add_f64 %0, %1, %2\n\t"
               "v_mul_f64 %0, %0, %3" : "=&v"(r) : "v"(a), "v"(b), "v"(m));
  return r;
}
// lower half: keep a; upper half: b of lane l - 32 (one permlane32_swap per dword)
__device__ __forceinline__ double keep_lo_take_lo(double a, double b) {
  const long long x = __double_as_longlong(a), y = __double_as_longlong(b);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)y, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(x >> 32), (unsigned)(y >> 32), false, false);
  return __longlong_as_double(((long long)hi[0] << 32) | lo[0]);
}

template <int... J>
__device__ __forceinline__ void gather_seq(double v, double (&all)[12], std::integer_sequence<int, J...>) {
  ((all[J] = rbc<LN(J)>(v)), ...);
}
// the stage's 12-vector from the column lanes
__device__ __forceinline__ void gather12(double v, double (&all)[12]) {
  gather_seq(v, all, std::make_integer_sequence<int, 12>{});
}
template <int... J>
__device__ __forceinline__ void gatherd_seq(double v, double (&all)[12], std::integer_sequence<int, J...>) {
  ((all[J] = rbc<J>(v)), ...);
}
// lanes 0..11 of the row, in lane order
__device__ __forceinline__ void gather_direct12(double v, double (&all)[12]) {
  gatherd_seq(v, all, std::make_integer_sequence<int, 12>{});
}
// sum_j a_j b_j over 12 terms in three interleaved chains (shorter dependency path)
__device__ __forceinline__ double dot12(const double (&a)[12], const double (&b)[12]) {
  double s0 = a[0] * b[0], s1 = a[1] * b[1], s2 = a[2] * b[2];
#pragma unroll
  for (int j = 3; j < 12; j += 3) {
    s0 += a[j] * b[j];
    s1 += a[j + 1] * b[j + 1];
    s2 += a[j + 2] * b[j + 2];
  }
  return (s0 + s1) + s2;
}
// v(lane l) + v(lane l +- 16): rows 0 + 1 and rows 2 + 3, the same sum order in both rows
__device__ __forceinline__ double row_pair_sum(double v) {
  const long long b = __double_as_longlong(v);
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  const double a0 = __longlong_as_double(((long long)hi[0] << 32) | lo[0]);
  const double a1 = __longlong_as_double(((long long)hi[1] << 32) | lo[1]);
  return a0 + a1;
}
// v(lane l) + v(lane l +- 32): rows 0 + 2 and rows 1 + 3 (one add of the same two values
// in both lanes of a pair: the sum is bit-identical in both)
__device__ __forceinline__ double pair_sum32(double v) {
  const long long b = __double_as_longlong(v);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  const double a0 = __longlong_as_double(((long long)hi[0] << 32) | lo[0]);
  const double a1 = __longlong_as_double(((long long)hi[1] << 32) | lo[1]);
  return a0 + a1;
}
// max(a, b) as the hardware instruction, for operands the compiler cannot prove canonical
// (DPP / permlane moves, LDS loads): C's fmax would canonicalize each of them first (see
// clamp_hw); the engine's values are never signalling NaNs
__device__ __forceinline__ double fmax_hw(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double row_pair_max(double v) {
  const long long b = __double_as_longlong(v);
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  return fmax_hw(__longlong_as_double(((long long)hi[0] << 32) | lo[0]),
                 __longlong_as_double(((long long)hi[1] << 32) | lo[1]));
}
__device__ __forceinline__ double pair_max(double v) {
  const long long b = __double_as_longlong(v);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  return fmax_hw(__longlong_as_double(((long long)hi[0] << 32) | lo[0]),
                 __longlong_as_double(((long long)hi[1] << 32) | lo[1]));
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// Launder an LDS base pointer: the pointer round-trips a VGPR through an empty asm
// (opaque to the optimiser, so loads through it are not hoisted out of loops)
// and comes back uniform in an SGPR via readfirstlane, costing no VGPR.
template <typename P>
__device__ __forceinline__ void lds_uniform(P*& q) {
  asm volatile("" : "+v"(q));
  if constexpr (sizeof(P*) == 4) {  // an LDS pointer
    q = reinterpret_cast<P*>(static_cast<unsigned long>(
        __builtin_amdgcn_readfirstlane(static_cast<int>(reinterpret_cast<unsigned long>(q)))));
  } else {  // a global-workspace pointer (horizons beyond 32 stages)
    const unsigned long long v = reinterpret_cast<unsigned long long>(q);
    const unsigned lo = __builtin_amdgcn_readfirstlane((int)v), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    q = reinterpret_cast<P*>(((unsigned long long)hi << 32) | lo);
  }
}
// a wave-uniform double kept in SGPRs
__device__ __forceinline__ double uni(double v) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)bits);
  const int hi = __builtin_amdgcn_readfirstlane((int)(bits >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// min(max(v, lo), hi) as the two hardware instructions.  C's fmax / fmin on values the
// compiler cannot prove canonical (loads, held registers) make it canonicalize each operand
// first (v_max_f64 x, x: IEEE mode quiets a signalling NaN), one extra FP64 instruction per
// bound and use; the engine's values are never signalling NaNs, and for every other input
// (quiet NaNs included: maxNum / minNum) the result is the same.
__device__ __forceinline__ double clamp_hw(double v, double lo, double hi) {
  double r;
  asm("v_max_f64 %0, %1, %2\n\tv_min_f64 %0, %0, %3" : "=&v"(r) : "v"(v), "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ double sel3(int i, double a0, double a1, double a2) {
  return i == 0 ? a0 : (i == 1 ? a1 : a2);
}

// f(integral_constant<int, J>) for J in the sequence, in order
template <typename F, int... J>
__device__ __forceinline__ void for_each_j(F&& f, std::integer_sequence<int, J...>) {
  (f(std::integral_constant<int, J>{}), ...);
}
// a0 += v(lane J) g0, a1 += v(lane J) g1, a2 += v(lane J) g2, v broadcast from lane J of the
// row (v_fmac_f64_dpp; s_nop 1 covers a VALU write of v just before)
template <int J>
__device__ __forceinline__ void fmac3_bc(double& a0, double& a1, double& a2, double v, double g0, double g1, double g2) {
  asm("s_nop 1\n\t"
      "v_fmac_f64_dpp %0, %3, %4 row_newbcast:%7 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %1, %3, %5 row_newbcast:%7 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f64_dpp %2, %3, %6 row_newbcast:%7 row_mask:0xf bank_mask:0xf"
      : "+v"(a0), "+v"(a1), "+v"(a2)
      : "v"(v), "v"(g0), "v"(g1), "v"(g2), "n"(J));
}

}  // namespace
}  // namespace mpcq
