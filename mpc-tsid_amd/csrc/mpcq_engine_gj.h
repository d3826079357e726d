// mpcq_engine_gj.h — the factorisation's dense steps on a 12x12 block held one row per column
// lane: the Gauss-Jordan inverse (gj12) and the Schur update by a coupling block (schur_cols).
#pragma once
#include "mpcq_engine_lanes.h"

namespace mpcq {
namespace {

// Gauss-Jordan inverse of a 12x12 SPD matrix held one row per column lane
// (row psi in lane LN(psi)); pivots broadcast by row_newbcast, no pivoting.
// gj_fmac<PV>: the pivot's eleven row updates c[j] += a * R[j](lane LN(PV)), j != PV, as
// v_fmac_f64_dpp (the broadcast folded into the FMA: one instruction per entry instead of
// a DPP move and an FMA; fma(a, b, c) and c += b a round alike, so the same bits)
#define MPCQ_GJ11(J)                                                                         \
  asm("s_nop 1\n\t"                                                                          \
      "v_fmac_f64_dpp %0, %11, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %1, %12, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %2, %13, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %3, %14, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %4, %15, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %5, %16, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %6, %17, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %7, %18, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %8, %19, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %9, %20, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %10, %21, %22 row_newbcast:" #J " row_mask:0xf bank_mask:0xf"          \
      : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]), "+v"(o[4]), "+v"(o[5]), "+v"(o[6]),  \
        "+v"(o[7]), "+v"(o[8]), "+v"(o[9]), "+v"(o[10])                                      \
      : "v"(r[0]), "v"(r[1]), "v"(r[2]), "v"(r[3]), "v"(r[4]), "v"(r[5]), "v"(r[6]), "v"(r[7]), \
        "v"(r[8]), "v"(r[9]), "v"(r[10]), "v"(a))
template <int PV>
__device__ __forceinline__ void gj_fmac(double (&c)[12], const double (&R)[12], double a) {
  constexpr int J = LN(PV);
  double o[11], r[11];  // the entries j != PV in order (register renames, no moves)
#pragma unroll
  for (int q = 0; q < 11; ++q) {
    o[q] = c[q < PV ? q : q + 1];
    r[q] = R[q < PV ? q : q + 1];
  }
  if constexpr (J == 0) MPCQ_GJ11(0);
  else if constexpr (J == 1) MPCQ_GJ11(1);
  else if constexpr (J == 2) MPCQ_GJ11(2);
  else if constexpr (J == 4) MPCQ_GJ11(4);
  else if constexpr (J == 5) MPCQ_GJ11(5);
  else if constexpr (J == 6) MPCQ_GJ11(6);
  else if constexpr (J == 8) MPCQ_GJ11(8);
  else if constexpr (J == 9) MPCQ_GJ11(9);
  else if constexpr (J == 10) MPCQ_GJ11(10);
  else if constexpr (J == 12) MPCQ_GJ11(12);
  else if constexpr (J == 13) MPCQ_GJ11(13);
  else if constexpr (J == 14) MPCQ_GJ11(14);
  else static_assert(J < 0, "a column lane LN(i)");
#pragma unroll
  for (int q = 0; q < 11; ++q) c[q < PV ? q : q + 1] = o[q];
}
#undef MPCQ_GJ11
// FOLD = false (beyond 32 stages): the DPP move + FMA form -- the folded blocks hold all
// their operands at once, which the 168 / 128-VGPR budgets there pay for in spills inside
// the ADMM loop (N = 48: 6 -> 15 scratch reloads per iteration in the gfx950 assembly)
// Lazy pivot rows (round 5): the pivot row is not normalised when it is used -- its lane's
// multiplier is 0, so its row stays p and its diagonal becomes 1 -- and each row is scaled
// by its own pivot's 1/d once, after the twelfth step.  A row that has been a pivot is then
// d times the textbook (normalised) row; every later update of it is linear in the row, so
// it stays d times the textbook row, and the final scaling gives the same inverse.  It saves
// the selects that gave the pivot lane a zero base (22 v_cndmask_b32 per pivot, about 40 %
// of the Gauss-Jordan instructions) for 12 multiplies at the end; the rounding differs from
// the normalised form in the last bits.  Up to 32 stages (FOLD); beyond, the normalised
// form stays: the lazy one measured 12-14 % fewer factorisation cycles (N = 16 84.8 k ->
// 74.1 k, N = 32 124 k -> 108 k, profiles/r05h_factime*) with the statuses and iterations
// of the oracle kept, but at N = 48 its (2-3x larger, ~1e-12) first-solve rounding grew to
// 2.1e-7 after five warm-started ticks (8.1e-8 normalised; tools/drift.py,
// profiles/r05j_drift_*).  -DMPCQ_GJ_NORM: the normalised form everywhere.
#ifdef MPCQ_GJ_NORM
template <bool FOLD>
constexpr bool kGjLazy = false;
#else
template <bool FOLD>
constexpr bool kGjLazy = FOLD;
#endif
template <int PV, bool FOLD>
__device__ __forceinline__ void gj_step(double (&R)[12], int me, bool& ok, double& sc) {
  constexpr bool LAZY = kGjLazy<FOLD>;
  const double d = rbc<LN(PV)>(R[PV]);
#ifdef MPCQ_DEBUG_PIVOT
  if (!(d > 0.0) && me == PV) printf("pivot fail blk %d thr %d PV %d d %g\n", (int)blockIdx.x, (int)threadIdx.x, PV, d);
#endif
  if (!(d > 0.0)) ok = false;
  // 1/d: v_rcp_f64 and two Newton steps (the pivots are positive and far from the
  // denormal / overflow range, so the IEEE division's scaling and fix-up are not needed)
  double id = __builtin_amdgcn_rcp(d);
  double e_ = fma(-d, id, 1.0);
  id = fma(id, e_, id);
  e_ = fma(-d, id, 1.0);
  id = fma(id, e_, id);
  // one multiplier per row: every other row R - (R[PV] / d) p, so each entry is a single
  // FMA on the broadcast pivot row; the pivot row itself: p / d (normalised form) or p
  // (lazy: multiplier 0, scaled by sc = 1/d at the end)
  const bool isp = me == PV;
  const double a = isp ? (LAZY ? 0.0 : id) : -(R[PV] * id);
  if constexpr (FOLD) {
    double c[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) c[j] = (isp && !LAZY) ? 0.0 : R[j];
    gj_fmac<PV>(c, R, a);
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j != PV) R[j] = c[j];
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      if (j == PV) continue;
      const double base = (isp && !LAZY) ? 0.0 : R[j];
      R[j] = fma(a, rbc<LN(PV)>(R[j]), base);
    }
  }
  if constexpr (LAZY) {
    R[PV] = isp ? 1.0 : a;
    if (isp) sc = id;
  } else {
    R[PV] = a;
  }
}
template <bool FOLD, int... P>
__device__ __forceinline__ void gj_seq(double (&R)[12], int me, bool& ok, double& sc, std::integer_sequence<int, P...>) {
  (gj_step<P, FOLD>(R, me, ok, sc), ...);
}
template <bool FOLD>
__device__ __forceinline__ void gj12(double (&R)[12], int me, bool& ok) {
  double sc = 1.0;
  gj_seq<FOLD>(R, me, ok, sc, std::make_integer_sequence<int, 12>{});
  if constexpr (kGjLazy<FOLD>) {
#pragma unroll
    for (int j = 0; j < 12; ++j) R[j] *= sc;
  }
}

// Ro -= G C' for one 12x12 coupling block C held one row per column lane in
// compact form (ca on column CI mod 6, c6 on the velocity columns): column CI of
// the product takes row CI of C from lane LN(CI) by row broadcast
// The broadcasts fold into v_fmac_f64_dpp (one instruction per term instead of a DPP
// move and an FMA); the two chains start from -0 (x + -0 = x for every x, so the first
// term is the plain product, as a multiply) and keep their order: the same bits.
#define MPCQ_SCHUR2_LANE(J)                                                                  \
  asm("s_nop 1\n\t"                                                                          \
      "v_fmac_f64_dpp %0, %2, %8 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"        \
      "v_fmac_f64_dpp %1, %3, %9 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"        \
      "v_fmac_f64_dpp %0, %4, %10 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %1, %5, %11 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %0, %6, %12 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %1, %7, %13 row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"       \
      "v_fmac_f64_dpp %0, %14, %15 row_newbcast:" #J " row_mask:0xf bank_mask:0xf"           \
      : "+v"(a0), "+v"(a1)                                                                   \
      : "v"(ca), "v"(c6[0]), "v"(c6[1]), "v"(c6[2]), "v"(c6[3]), "v"(c6[4]), "v"(ga), "v"(G[6]), \
        "v"(G[7]), "v"(G[8]), "v"(G[9]), "v"(G[10]), "v"(c6[5]), "v"(G[11]))
template <int CI, bool FOLD>
__device__ __forceinline__ void schur_col(double (&Ro)[12], const double (&G)[12], double ca,
                                          const double (&c6)[6]) {
  constexpr int J = LN(CI);
  if constexpr (!FOLD) {  // (beyond 32 stages, as gj_step)
    double a0 = G[CI < 6 ? CI : CI - 6] * rbc<J>(ca), a1 = G[6] * rbc<J>(c6[0]);
    a0 = fma(G[7], rbc<J>(c6[1]), a0);
    a1 = fma(G[8], rbc<J>(c6[2]), a1);
    a0 = fma(G[9], rbc<J>(c6[3]), a0);
    a1 = fma(G[10], rbc<J>(c6[4]), a1);
    a0 = fma(G[11], rbc<J>(c6[5]), a0);
    Ro[CI] -= a0 + a1;
    return;
  }
  const double ga = G[CI < 6 ? CI : CI - 6];
  // a0 = ga ca + G7 c1 + G9 c3 + G11 c5, a1 = G6 c0 + G8 c2 + G10 c4 (c broadcast from lane J)
  double a0 = -0.0, a1 = -0.0;
  if constexpr (J == 0) MPCQ_SCHUR2_LANE(0);
  else if constexpr (J == 1) MPCQ_SCHUR2_LANE(1);
  else if constexpr (J == 2) MPCQ_SCHUR2_LANE(2);
  else if constexpr (J == 4) MPCQ_SCHUR2_LANE(4);
  else if constexpr (J == 5) MPCQ_SCHUR2_LANE(5);
  else if constexpr (J == 6) MPCQ_SCHUR2_LANE(6);
  else if constexpr (J == 8) MPCQ_SCHUR2_LANE(8);
  else if constexpr (J == 9) MPCQ_SCHUR2_LANE(9);
  else if constexpr (J == 10) MPCQ_SCHUR2_LANE(10);
  else if constexpr (J == 12) MPCQ_SCHUR2_LANE(12);
  else if constexpr (J == 13) MPCQ_SCHUR2_LANE(13);
  else if constexpr (J == 14) MPCQ_SCHUR2_LANE(14);
  else static_assert(J < 0, "a column lane LN(i)");
  Ro[CI] -= a0 + a1;
}
#undef MPCQ_SCHUR2_LANE
template <bool FOLD, int... C>
__device__ __forceinline__ void schur_cols(double (&Ro)[12], const double (&G)[12], double ca,
                                           const double (&c6)[6], std::integer_sequence<int, C...>) {
  (schur_col<C, FOLD>(Ro, G, ca, c6), ...);
}

}  // namespace
}  // namespace mpcq
