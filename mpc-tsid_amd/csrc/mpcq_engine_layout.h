// mpcq_engine_layout.h — where the engine keeps what: the CSC offsets of the constraint matrix,
// the step-ordered slots of the sweep arrays, the per-horizon layout switches, and the LDS
// (Smem<N>), workspace (Work<N>) and prologue (Prologue<N>) layouts of one instance.
// Plain C++17, no HIP: tests/host/engine_layout_check.cpp instantiates it for every horizon on
// the CPU; the engine units check their own horizon at the end (MPCQ_ENGINE_N).
#pragma once
#ifndef __HIPCC__  // off the device compiler the attributes mean nothing
#ifndef __host__
#define __host__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#endif

namespace mpcq {
namespace {

// ---------------------------------------------------------------------------
// CSC offsets of MPC.create_ML's pattern (see mpcq_pattern in mpcq_api.cpp).
template <int N>
__host__ __device__ __forceinline__ constexpr int XO(int k, int i) {  // state column X_{k+1}[i]
  return (k < N - 1) ? 30 * k + (i < 6 ? 2 * i : 12 + 3 * (i - 6)) : 30 * (N - 1) + i;
}
template <int N>
__host__ __device__ __forceinline__ constexpr int FO(int k, int f, int c) {  // force column f_k[3f+c]
  return 30 * N - 18 + 96 * k + 24 * f + 7 * c;
}
// lane (within the stage row) that owns force / state index psi = 3f + c
__host__ __device__ constexpr int LN(int psi) { return 4 * (psi / 3) + psi % 3; }

// Step-ordered slots of the sweep arrays.  The top chain walks stages 0, 1, ..
// upwards and the bottom chain N-1, N-2, .. downwards; storing the bottom
// stages in reverse (stage k > MID at slot N + MID - k) makes both chains walk
// their slots in the same direction, so every lane of the sweep wave addresses
// step j as (its own base) + j * (a uniform stride): an immediate offset, no
// per-step pointer arithmetic.  SIG: G/H, S^-1 and the right-hand sides
// (stages 0..N-1); SIGX: the state vectors xs[q] = X_q, q = 0..N.
template <int N>
__host__ __device__ constexpr int SIG(int k) { return k <= N / 2 ? k : N + N / 2 - k; }
template <int N>
__host__ __device__ constexpr int SIGX(int q) { return q <= N / 2 ? q : N + N / 2 + 1 - q; }

// Stage rows of the layout: a wave64 holds four 16-lane rows, so the workgroup
// has N rounded up to a multiple of 4 rows.  The rows past N ("phantom" rows)
// run as copies of stage N-1: they read what row N-1 reads and store the same
// values to the same places (identical stores), are left out of the in-place
// updates and the sums, and their maxima duplicate row N-1's.
template <int N>
constexpr int kRows = (N + 3) & ~3;

// ---------------------------------------------------------------------------
// Shared memory of one instance (N=16: 78.6 KB -> 2 instances per CU; N=32:
// 156.7 KB -> 1; N=48: 140 KB with S^{-1} / F W / R^{-1} Q in global memory).

// The sweep matrices (G / H / M^{-1} in GH, S^{-1} in Sm) are 12 x 12, row-major
// with a row stride of RS = 12 doubles (96 B).  Column reads (the outward sweep:
// 12 lanes, consecutive doubles) are conflict-free; the inward sweep's b128 row
// reads (lane r at 96 r) collide 2-3 ways inside a 16-lane group.  A 13-double
// stride removes that but needs 3 KB more LDS than two instances per CU leave at
// N = 16.  GS = one stage's slot.
constexpr int RS = 12, GS = 12 * RS;
// Offset of slot q in GH / Sm: the slots of the bottom chain (q > N/2) sit two
// doubles (16 B) further on.  The sweep's b128 row reads put 4 lanes of one chain
// and 8 of the other in each 16-lane bank group; rows 96 B apart cover only the
// eight 4-bank slots at multiples of 8 dwords, so without the shift the two
// chains' rows met in the same banks (2-way conflicts), with it they interleave.
template <int N>
constexpr int kSlotPad = 2;
template <int N>
__host__ __device__ constexpr int SLOT(int q) { return GS * q + (q > N / 2 ? kSlotPad<N> : 0); }

// Rejected round-4 solve variants (block cyclic reduction of the state system; the
// termination check deferred into the next iteration) were measured slower and removed
// in round 5; their code is kept as a patch, tools/attic/engine_cr_dc_round4.patch, and
// their measurements in DESIGN.md section 8 (round 4) items 3-4.
// Four more were measured slower and removed later, their code kept as
// tools/attic/engine_variants_round6.patch: three or four 16-stage instances per CU in the
// beyond-32-stage layout (round 5: C2 62.0 k / 35.3 k against 127.6 k QP/s; DESIGN.md section
// 8b item 4), the explicit state-system inverse at 16 stages (round 5: 1.92 against 1.85 us per
// iteration and one instance per CU, C2 86 k against 126 k QP/s; section 8b item 6), the
// nested-dissection state solve (round 6: N = 32 2.976 against 2.875 us per iteration; section
// 8 item 1) and slicing at 16 stages (kSlice, mpcq_engine.hip).
// Horizons beyond 32 stages do not fit a CU's LDS (N = 48: 236 KB): S^{-1}, F W and
// R^{-1} Q move to a per-instance global workspace (LaunchArgs::work, work_doubles(N)
// doubles per instance, L2-resident), the rest stays in LDS (N = 48: 140 KB).
template <int N>
constexpr bool kBig = N > 32;
// F W stays in LDS at every N (the ADMM loop reads it every iteration: from L2 at
// N = 48 it cost the right-hand-side phase ~14 k cycles per iteration, r03d
// stamps); beyond 49 stages the scaled constraint values (126 N - 18 doubles) leave
// LDS instead (N = 64: 197 KB with them, 133 KB without); the engine reads them
// through the same accessors, the stage-parallel phases from L2.
template <int N>
constexpr bool kAbG = N > 49;
// Beyond 48 stages (13-16 waves: 128 VGPRs) the F_k row is read from the workspace in
// the loop and the z update's constants are batch-loaded from private memory instead
// of being held; from 33 to 48 stages (168 VGPRs) holding them is faster.  Measured at
// every horizon 33..64 with both, either and neither (tools/bigsweep.py,
// profiles/r03o_bigsweep.txt: N = 48 9.05 us per iteration held vs 10.37 not; N = 56
// 19.27 not held vs 20.06).  -DMPCQ_FR_HELD / -DMPCQ_ZC_HELD: held everywhere (experiments).
#ifdef MPCQ_FR_HELD
template <int N> constexpr bool kFrWork = false;
#else
template <int N> constexpr bool kFrWork = N > 48;
#endif
#ifdef MPCQ_ZC_HELD
template <int N> constexpr bool kZcMem = false;
#else
template <int N> constexpr bool kZcMem = N > 48;
#endif
// The outward sweep of ph_sweep_split (33..48 stages) as ph_sweep_lag's: full 12-term
// column products per lane (the outward sweep needs no S^{-1}, which is what sent the
// split sweep's inward half to the stage-parallel S^{-1} phase).  Round 4 (r04h, per
// iteration alone / 256 in flight): N = 40 6.07 -> 5.93 / 6.94 -> 6.73 us, N = 48 6.89 ->
// 6.79 / 7.69 -> 7.62; beyond 48 stages mixed (N = 64 14.96 -> 14.78 / 18.73 -> 19.55), so
// the split products stay there.  -DMPCQ_SPLIT_OUT: the split outward products everywhere.
#ifdef MPCQ_SPLIT_OUT
template <int N> constexpr bool kLagOut = false;
#else
template <int N> constexpr bool kLagOut = N <= 48;
#endif
// Stage stride of F W in LDS (doubles).  ph_recover reads row ph of F_k W_k as three
// ds_read_b128 per lane (16-B units 36 k + 3 ph at a 72-double stride): within each
// 16-lane bank group of that instruction (two stages' lanes), ph 0/1/2 of one stage met
// ph 6/7/8 of the next in the same banks (2-way conflicts); at a 96-double stride (256 B
// x 3, stages 0 mod 16 units apart) the twelve rows of each group land in distinct banks.
// Up to 32 stages, where the LDS has the 24 N doubles (N = 16: 80,048 B, still two
// instances per CU).
template <int N>
constexpr int kFWS = kBig<N> ? 72 : 96;
// Up to 16 stages the ADMM loop's exit status goes through LDS (Smem::flag[4]) instead of
// a register carried across the loop: the N = 16 kernel then spills 27 instead of 43
// VGPRs (scratch 256 -> 224 B per lane) and its C2 HBM traffic falls 127 -> 88 MB per
// launch, per-iteration time unchanged (same box, r04u).  At N = 32 the same change made
// the iteration 1.3 % slower and doubled the traffic through the rho-update path's spills,
// so the status stays a register there.
template <int N>
constexpr bool kXstLds = N <= 16;
// From 17 to 48 stages (round 5) the exit status is not carried at all: after the loop it is
// re-derived from what the loop leaves -- a failed factorisation sets sh.flag[2], and an
// early exit stops with iter <= max_iter after the same tests, in the same order, on the
// residuals and infeasibility bits that stay live after the loop anyway.  Carried in a
// register, it was spilled and stored once per check segment at N = 32 (round 4).
// Beyond 48 stages (128 VGPRs) the re-derivation cost the iteration 8 % (N = 64 15.2 -> 16.5
// us alone, 19.7 -> 21.2 at 256 in flight, r05v): there the status is carried as in round 4.
template <int N>
constexpr bool kXstRe = !kXstLds<N> && N <= 48;
template <int N>
struct Work {  // offsets (doubles) inside one instance's workspace
  // SM starts two slots in (a pad kept from round 2; the sweep no longer reads it)
  // FR: each lane's row of F_k (12 doubles, lane-interleaved: entry i of thread t at 16 kRows i + t)
  static constexpr int SM = 2 * GS, FW = SM + N * GS + 2, QL = FW + 72 * N, ZERO = QL + 36 * N, AB = ZERO + 72,
                       FR = AB + (kAbG<N> ? ((126 * N - 18 + 1) & ~1) : 0), SIZE = FR + (N > 48 ? 12 * 16 * kRows<N> : 0);
};

template <int N>
struct Smem {
  double Ab[kAbG<N> ? 2 : 126 * N - 18];  // scaled constraint values, CSC order (N > 49: Work<N>::AB)
  // GH[0] = M^{-1}, GH[SIG(k)] = G_k (1 <= k <= m), GH[SIG(k+1)] = H_k (m <= k < N-1),
  // row-major (the sweeps' step order, see SIG).
  // During the factorisation slot k holds Q_k [0,36), F_k W_k [36,108) and the
  // dynamics-row rho of stage k [108,120); during scaling the row factors; in
  // the prologue xref / fsteps / the gait walk.
  alignas(16) double GH[N][GS];
  double GHpad[2];  // the bottom slots' shift (SLOT)
  // (N > 32: these three live in the global workspace, Work<N>)
  alignas(16) double Sm[kBig<N> ? 1 : N][GS];  // S_k^{-1} / U_k^{-1} of stage k at SLOT(SIG(k)), row-major (row stride RS)
  double Smpad[2];
  // F_k W_k (12x6, row psi at [6 psi]); W_k = B_k' R on rows 6..11: here beyond 32 stages
  // (stage stride 72), FWs at the end up to 32 stages (stride kFWS = 96)
  alignas(16) double FWb[kBig<N> ? N : 1][72];
  double QL[kBig<N> ? 1 : N][36];   // B_k F_k W_k = R^{-1} W_k' F_k W_k (6x6)
  union {
    struct {
      // sweep right-hand side of stage k's states = bo[k] + na[k]: bo from stage k
      // itself, na from stage k+1's dynamics rows (Hd (w - beta) + H6 w, summed by
      // ph_rhs); nb is scratch of the checks
      double bo[N][12];
      double na[N][12];
      double nb[N][12];
      double yv[N][12];      // w = S^{-1} y of the inward sweep (states / duals during the checks)
      double xs[N + 1][12];  // X_k (xs[k+1] = X_{k+1}, stage k's states)
    } it;
    struct {
      alignas(16) double St[144];  // sweep hand-offs of the factorisation (16-B aligned: the
      alignas(16) double Sb[144];  // couplings read them as column pairs)
      // (32 unused bytes, where the nested-dissection variant's two placeholders sat: at N = 4
      // fa is the union's larger member, so they keep every later array's LDS offset there)
      alignas(16) double fapad_[4];
    } fa;
  } u;
  // per-wave partial reductions (32 per wave); during the sweeps the sink of lanes
  // whose store is void (lane (t & 31) + 12 j, j <= N/2 + 1)
  double red[(8 * kRows<N> + 32 > 12 * (N / 2 + 2) + 32) ? 8 * kRows<N> + 32 : 12 * (N / 2 + 2) + 32];
  double dump[64];  // sink of predicated stores (never read): lane & 63
  // (13 unused doubles: where round 4's deferred-check arrays sat; they keep every later
  // array's LDS offset, and with it the compiler's register allocation, as measured)
  double pad13_[13];
  alignas(16) double zero[72];  // zeros: masked coefficient reads point here instead of selecting
  // flag[4] (kXstLds): the ADMM loop's exit status, written by thread 0 at the (uniform)
  // exits and read by every thread after the loop
  int flag[kXstLds<N> ? 5 : 4];
  // (up to 32 stages) F W at its 96-double stride, last: its round-4 growth leaves every
  // other array's LDS offset -- and the compiler's register allocation -- as before
  alignas(16) double FWs[kBig<N> ? 1 : N][kBig<N> ? 2 : kFWS<N>];
};

// prologue aliases inside GH
template <int N>
struct Prologue {
  static constexpr int XR = 0;             // xref, 12(N+1) doubles
  static constexpr int FS = 12 * (N + 1);  // fsteps, 260 doubles
  static constexpr int INTS = FS + 260;    // phase_of_stage[N], contact[20][4] as ints
};

#ifdef MPCQ_ENGINE_N
// the unit's own horizon (Work<N>::SIZE against work_doubles(N): mpcq_engine.hip, which sees both)
static_assert(MPCQ_ENGINE_N >= 4 && kRows<MPCQ_ENGINE_N> <= 64, "horizons 4..64 (1024 threads at most)");
static_assert(sizeof(Smem<MPCQ_ENGINE_N>) <= 160 * 1024, "Smem<N> exceeds the CU's LDS");
static_assert(kRows<MPCQ_ENGINE_N> > 16 || sizeof(Smem<MPCQ_ENGINE_N>) <= 80 * 1024,
              "Smem<N> must fit twice in a CU for N <= 16");
#endif

}  // namespace
}  // namespace mpcq
