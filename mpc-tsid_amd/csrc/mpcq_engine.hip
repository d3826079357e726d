// mpcq_engine.hip — batched convex-MPC QP engine for MI355X (gfx950, CDNA4).
//
// One workgroup of N/4 wave64s owns one QP instance for its whole life:
// formulation (MPC.py:98-378), Ruiz scaling, KKT factorisation and the
// OSQP-0.6 ADMM iterations run out of registers + LDS.  HBM sees only the
// compulsory inputs (xref, fsteps) and outputs (f0 / x / y / status).
//
// Lane layout: a stage k is one 16-lane DPP row (so a wave holds 4 stages);
// lane s = 4f + c of row k is foot f, component c.  Lanes c < 3 own the
// column pair (force f_k[3f+c], state X_{k+1}[3f+c]) and three rows: the
// dynamics row 3f+c, the swing row 3f+c and friction row c of foot f; lane
// c = 3 owns friction rows 3 and 4 of foot f (its column work is a discarded
// shadow of lane c = 2).  Stage-wide vectors move by DPP row_newbcast,
// foot-wide ones by quad_perm; only stage-to-stage hand-offs go through LDS.
//
// KKT solve (P + sigma I + A' R A) w = b.  In stage order the matrix is block
// tridiagonal; the forces only couple inside a stage, so they are eliminated
// first (every stage in parallel: F_k = K_ff,k^{-1}, one row per lane), which
// leaves a block-tridiagonal system in the states with 12x12 blocks
//   D_k = K_XX,k - Xd Q_k Xd - Hd_{k+1} Q_{k+1} Hd_{k+1},   Q_k = W_k' F_k W_k (6x6)
//   L_k = C_X,k  - Xd Q_k Hd_k                              (W_k = R B_k on rows 6..11)
// factored two-ended ("twisted"): top-down for stages < m, bottom-up for
// stages > m, meeting at m = N/2, so each substitution sweep is N/2 steps deep:
//   y_k = b_k - G_k y_{k-1}   (k < m)      v_k = b_k - H_k v_{k+1}   (k > m)
//   x_m = M^{-1}(y_m + v_m - b_m)
//   x_k = S_k^{-1} y_k - G_{k+1}' x_{k+1}  x_k = U_k^{-1} v_k - H_{k-1}' x_{k-1}
// The two sweeps run at once in rows 0 and 1 of wave 0 (one instruction
// stream), reading G / H from LDS; S^{-1}, U^{-1}, M^{-1} rows stay in the
// stage lanes' registers.
//
// Files: mpcq_engine_layout.h (CSC offsets, slots, per-horizon
// switches, Smem / Work / Prologue), mpcq_engine_lanes.h (lane primitives),
// mpcq_engine_gj.h (Gauss-Jordan and Schur steps), mpcq_engine_form.h (formulation
// pieces); here the kernel, in numbered sections, its launcher and the per-horizon entry.
#include <math.h>

#include <type_traits>
#include <utility>

#include "mpcq_internal.h"
#include "mpcq_engine_layout.h"
#include "mpcq_engine_lanes.h"
#include "mpcq_engine_gj.h"
#include "mpcq_engine_form.h"

namespace mpcq {
namespace {

constexpr double kInf = 1e30;  // OSQP_INFTY
constexpr double kMinScaling = 1e-4, kMaxScaling = 1e4;
constexpr double kRhoMin = 1e-6, kRhoMax = 1e6, kRhoEq = 1e3, kRhoTol = 1e-4;
constexpr double kDivTol = 1e-30;

// constraint classes (OSQP set_rho_vec)
enum : unsigned { RC_LOOSE = 0, RC_INEQ = 1, RC_EQ = 2 };

#ifndef MPCQ_STAMP_WAVE
#define MPCQ_STAMP_WAVE 0
#endif
#if defined(MPCQ_STAMPS) && defined(MPCQ_STAMPS_LEAN)
// lean variant: only the uniform points after the loop's barriers (1 prologue, 2 factor,
// 3 P1-P4, 7 sweeps, 10 P8-P9, 11 checks, 12 epilogue), accumulated in SGPRs without a
// lane branch, so the measured code stays close to the production build
#define STAMP_DECL uint64_t st_acc[16] = {}; uint64_t st_last = __builtin_amdgcn_s_memtime();
#define STAMP(i) do { if constexpr ((i) == 1 || (i) == 2 || (i) == 3 || (i) == 7 || (i) == 10 || (i) == 11 || (i) == 12) { \
    const uint64_t nw_ = __builtin_amdgcn_s_memtime(); st_acc[i] += nw_ - st_last; st_last = nw_; } } while (0)
#elif defined(MPCQ_STAMPS)
// (MPCQ_STAMP_WAVE = w: the stamps of wave w's first lane instead of wave 0's, clamped
// to the workgroup's last wave: kStampT)
#define STAMP_DECL uint64_t st_acc[16] = {}; uint64_t st_last = __builtin_amdgcn_s_memtime();
#define STAMP(i) do { if (threadIdx.x == kStampT) { const uint64_t nw_ = __builtin_amdgcn_s_memtime(); st_acc[i] += nw_ - st_last; st_last = nw_; } } while (0)
#else
#define STAMP_DECL
#define STAMP(i) do {} while (0)
#endif

// Sliced solves (LaunchArgs::slice_iters / resume, mpcq_set_slice) beyond 16 stages: one
// instance per CU there, so a long solve dispatched in a late round ends the launch late
// (DESIGN.md section 8).  Up to 16 stages two instances share a CU and slicing does not
// shorten the modelled launch (section 8b item 9): the code is compiled out and the ADMM
// loop's allocation stays the unsliced one.  Slicing at 16 stages was built and measured
// (round 6): slower than unsliced, as the model said, and removed; patch in
// tools/attic/engine_variants_round6.patch, measurements in DESIGN.md section 8 item 1b.
template <int N>
constexpr bool kSlice = slice_supported(N);

// Timing experiments only (> 1: the state sweep, or the factorisation, repeated in place)
#ifndef MPCQ_REP_SWEEP
#define MPCQ_REP_SWEEP 1
#endif
#ifndef MPCQ_REP_FACTOR
#define MPCQ_REP_FACTOR 1
#endif

// ---------------------------------------------------------------------------
// Function-body macros of engine_kernel: they name its locals, and are #undef-ed after it.

// The lane's offsets (LaneOffs) as local names: the held O0, or (RECOMP) re-derived from
// freshly laundered coordinates.
#define MPCQ_LANE_OFFS(RECOMP)                                                                              \
  if constexpr (RECOMP) launder();                                                                         \
  const LaneOffs O_ = (RECOMP) ? offs() : O0;                                                              \
  [[maybe_unused]] const int oXd = O_.oXd, oHd = O_.oHd, oH6 = O_.oH6, oF = O_.oF, oFa = O_.oFa,           \
                             oFb = O_.oFb, oF4 = O_.oF4, oFW = O_.oFW, oQL = O_.oQL, oXSp = O_.oXSp,       \
                             oXSp6 = O_.oXSp6, rXS = O_.rXS, rXSpm = O_.rXSpm, rXSp6m = O_.rXSp6m,         \
                             oHdm = O_.oHdm, oH6m = O_.oH6m, oFWcm = O_.oFWcm, oQLm = O_.oQLm, oB0 = O_.oB0; \
  [[maybe_unused]] const bool ta0 = O_.ta0;                                                                \
  [[maybe_unused]] double* const Wbo = O_.Wbo;                                                             \
  [[maybe_unused]] double* const Wna = O_.Wna
// The check's lane ids, re-derived from a laundered thread index: the red[] addresses
// built from them would otherwise be hoisted out of the ADMM loop and spilled too.
#define MPCQ_CHECK_IDS()                                           \
  int tl_ = t;                                                     \
  asm volatile("" : "+v"(tl_));                                    \
  [[maybe_unused]] const int wv = tl_ >> 6, lane = tl_ & 63, s = tl_ & 15
// the ADMM loop's exit status: LDS (kXstLds; read after the loop's closing barrier) or status
#define MPCQ_SET_XST(v_) do { if constexpr (kXstLds<N>) { if (t == 0) sh.flag[4] = (v_); } else if constexpr (!kXstRe<N>) { status = (v_); } } while (0)

// ---------------------------------------------------------------------------
// The engine kernel.  FUSED: formulate from (xref, fsteps) then solve.
// !FUSED: solve the given (Ax, l, u).  SOLVE=false: formulation only.

// ROB: the per-instance tables, all not null: LaunchArgs::robots in place of p.mass / gI / mu /
// fz_max, LaunchArgs::weights in place of p.state_weights / force_weight (the solving kernels
// only), LaunchArgs::disturb beside gravity in the dynamics rows' constants (the host fills a
// table that is not set with the context's values, the disturbance's with zeros).
// An instantiation of its own, so that the kernels of a launch without a table are instruction
// for instruction what they were before the table existed (the formulation's kernels only: the
// qp path takes Ax, l, u as given).
template <int N, bool FUSED, bool SOLVE, bool POLISH, bool ROB = false>
__global__ __launch_bounds__(16 * kRows<N>, 2)
void engine_kernel(mpcq_params p, LaunchArgs a) {
  constexpr int NR = kRows<N>, NW = NR / 4, T = 16 * NR, n = 24 * N, m = 44 * N, nnz = 126 * N - 18,
                MID = N / 2;
  [[maybe_unused]] constexpr int kStampT = 64 * (MPCQ_STAMP_WAVE < T / 64 ? MPCQ_STAMP_WAVE : T / 64 - 1);
  // the two chains of the state sweeps: top stages 0..MID-1, bottom N-1..MID+1
  // (BOT stages: MID - 1 for even N, MID for odd N), meeting at stage MID
  constexpr int BOT = N - 1 - MID;
  // ---- 1. pointers and lane coordinates ---------------------------------------------------------
  __shared__ Smem<N> sh;
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  // lane coordinates; the loops launder them (launder, at the end of this section) so that the
  // compiler recomputes the many LDS offsets derived from them instead of
  // hoisting each one into a register of its own
  const bool phantom = (t >> 4) >= N;  // a row past the horizon: a copy of stage N-1 (kRows)
  int k = phantom ? N - 1 : t >> 4, s = t & 15, f = s >> 2, c = s & 3;
  const bool cl = c < 3;          // column lane (c == 3: friction rows 3, 4 only)
  int cc = cl ? c : 2;            // column component; c == 3 shadows c == 2
  int ph = 3 * f + cc;            // own force / state index in the stage
  if ((int64_t)blockIdx.x >= a.batch) return;
  if constexpr (kSlice<N>) {  // (a resumed slice: its count is on the device, no host round trip)
    if (a.batch_dev && (int64_t)blockIdx.x >= (int64_t)*a.batch_dev) return;
  }
  const int64_t b = a.order ? (int64_t)a.order[blockIdx.x] : (int64_t)blockIdx.x;  // the instance
  // a session's robot with a pending reset (uniform per workgroup): the first tick's
  // formulation and a cold start, whatever a.mode and the warm pointers say.  The warm loads
  // are skipped, not fed zeros: row_A of a zero vector may leave -0 where the cold point holds +0.
  const bool first = a.first && a.first[b] != 0;
  [[maybe_unused]] double fz_rob = 0.0;
  if constexpr (ROB) fz_rob = uni(a.robots[b].fz_max);
  auto fz_max = [&]() __attribute__((always_inline)) -> double {
    if constexpr (ROB) return fz_rob;
    else return p.fz_max;
  };
  STAMP_DECL
  constexpr bool BIG = kBig<N>, ABG = kAbG<N>;
  // the scaled constraint values: LDS, or (N > 49) this instance's workspace (the
  // formulation-only launch builds them straight into its Ax output)
  using acd = std::conditional_t<ABG, g_cd, lds_cd>;
  double* AbW;
  if constexpr (ABG) AbW = SOLVE ? a.work + b * Work<N>::SIZE + Work<N>::AB : a.Ax_out + b * nnz;
  else AbW = sh.Ab;
  acd* Ab = (acd*)AbW;
  lds_cd* GHr = (lds_cd*)&sh.GH[0][0];
  // S^{-1}, R^{-1} Q: LDS, or (N > 32) this instance's global workspace; F W: LDS
  using wcd = std::conditional_t<BIG, g_cd, lds_cd>;
  using wdd = std::conditional_t<BIG, g_d, lds_d>;
  wcd* SmR;
  g_d* FRg = nullptr;  // (kFrWork: N > 48) this lane's F_k row in the workspace, stride 16 kRows
  lds_cd* FWr;
  wcd* QLr;
  wdd* SmW;
  lds_d* FWW;
  wdd* QLW;
  int zFW, zQL;  // offsets of a zero block from FWr / QLr (masked reads)
  if constexpr (BIG) {
    double* const wk = SOLVE ? a.work + b * Work<N>::SIZE : nullptr;  // (formulation only: unused)
    SmW = (wdd*)(wk + Work<N>::SM);
    FWW = (lds_d*)&sh.FWb[0][0];  // (Work<N>::FW stays reserved, unused)
    QLW = (wdd*)(wk + Work<N>::QL);
    if (SOLVE) FRg = (g_d*)(wk + Work<N>::FR + t);
    zFW = (int)(sh.zero - &sh.FWb[0][0]);
    zQL = Work<N>::ZERO - Work<N>::QL;
    if (SOLVE && t < 72) wk[Work<N>::ZERO + t] = 0.0;
  } else {
    SmW = (wdd*)&sh.Sm[0][0];
    FWW = (wdd*)&sh.FWs[0][0];
    QLW = (wdd*)&sh.QL[0][0];
    zFW = (int)(sh.zero - &sh.FWs[0][0]);
    zQL = (int)(sh.zero - &sh.QL[0][0]);
  }
  SmR = (wcd*)SmW;
  FWr = (lds_cd*)FWW;
  QLr = (wcd*)QLW;
  double* const gh0 = &sh.GH[0][0];
  int fo = FO<N>(k, f, cc), xo = XO<N>(k, ph);  // own force / state column in Ab
  int cr = (t >> 4) & 1;            // sweep row (wave 0): 0 top-down, 1 bottom-up
  // sweep lane's state index; lanes 12..15 (no state) repeat lanes 0..3, which sit in
  // their bank group, so their reads broadcast instead of conflicting (measured: -2 %
  // per iteration at N <= 16; at N = 32, round 4, same box: SQ_LDS_BANK_CONFLICT per C3
  // launch 1.375e9 -> 0.718e9, 1.57 -> 0.82 of SQ_ACTIVE_INST_LDS, 3.169 -> 3.128 us per
  // iteration, C3 33.85 -> 33.35 ms, profiles/r04e_*; round 2's +2 % there is not
  // reproduced).  Beyond 32 stages (the split sweep) lane 11's row, unmeasured.
  int rr_ = s < 12 ? s : (N <= 32 ? s - 12 : 11);
  // the base pointers and the lane coordinates, opaque to the optimiser from here on
  auto launder = [&]() __attribute__((always_inline)) {
    lds_uniform(Ab); lds_uniform(GHr); lds_uniform(SmR); lds_uniform(FWr); lds_uniform(QLr);
    asm volatile("" : "+v"(k), "+v"(f), "+v"(c), "+v"(cc), "+v"(ph), "+v"(fo), "+v"(xo),
                 "+v"(cr), "+v"(rr_));
  };
  (void)lane;

  // ---- 2. scaled-A accessors, own rows and columns, bounds --------------------------------------
  auto Xd = [&](int kk, int i) __attribute__((always_inline)) { return Ab[XO<N>(kk, i)]; };
  // dynamics row i of stage kk on X_kk[i] / on X_kk[i+6] (i < 6), kk >= 1
  // (loads stay in bounds for kk == 0 / i >= 6; callers mask those values)
  auto Hd = [&](int kk, int i) __attribute__((always_inline)) {
    return Ab[XO<N>(kk > 0 ? kk - 1 : 0, i) + (i < 6 ? 1 : 2)];
  };
  auto H6 = [&](int kk, int i) __attribute__((always_inline)) {
    return Ab[XO<N>(kk > 0 ? kk - 1 : 0, i < 6 ? i + 6 : 11) + 1];
  };
  // coefficient of force psi = 3fp + cp on dynamics row r (6..11) of stage kk
  auto Bc = [&](int kk, int r, int fp, int cp) __attribute__((always_inline)) -> double {
    const bool nz = r >= 9 || (r >= 6 && cp == r - 6);
    const double v = Ab[FO<N>(kk, fp, cp) + (r >= 9 ? r - 8 : 0)];
    return nz ? v : 0.0;
  };
  // coefficient of force component cp of foot fp on friction row t of that foot
  auto Frc = [&](int kk, int fp, int t_, int cp) __attribute__((always_inline)) -> double {
    const double v = Ab[FO<N>(kk, fp, cp) + (cp == 2 ? 5 + t_ : 5 + (t_ & 1))];
    return (cp == 2 || (t_ < 4 && (t_ >> 1) == cp)) ? v : 0.0;
  };
  // friction row t of foot f at stage k applied to the foot's forces (g0, g1, g2)
  auto fric_row = [&](int t_, double g0, double g1, double g2) __attribute__((always_inline)) {
    const int ta = t_ < 4 ? t_ : 0;
    const double cb = Ab[FO<N>(k, f, 2) + 5 + t_];
    const double ca = Ab[FO<N>(k, f, ta >> 1) + 5 + (ta & 1)];
    const double v = cb * g2;
    return t_ < 4 ? v + ca * ((ta >> 1) == 0 ? g0 : g1) : v;
  };

  // own rows: slot 0 dyn(k, ph) | fric t=3; slot 1 swing(k, ph) | fric t=4; slot 2 fric t=c | none
  auto nat_row = [&](int slot) __attribute__((always_inline)) -> int {
    if (slot == 0) return cl ? 12 * k + ph : 24 * N + 20 * k + 5 * f + 3;
    if (slot == 1) return cl ? 12 * N + 12 * k + ph : 24 * N + 20 * k + 5 * f + 4;
    return cl ? 24 * N + 20 * k + 5 * f + c : -1;
  };
  const int colF = 12 * N + 12 * k + ph, colX = 12 * k + ph;

  // P diagonal of the own columns (MPC.py:255-275).  ROB: row b of the weights table
  // (LaunchArgs::weights, mpcq_set_weights), read here once -- the lane's own state weight as one
  // global load, the workgroup-uniform force weight into SGPRs -- and held like the params'
  // values: q, the Ruiz passes, the cost scaling, K's diagonal and polish read these two.
  // (The formulation-only kernel has no P and does not touch the table.)
  const double P0f = weight_f<ROB && SOLVE>(a, b, p.force_weight);
  double P0X = p.state_weights[0];
#pragma unroll
  for (int e = 1; e < 12; ++e)
    if (ph == e) P0X = p.state_weights[e];
  P0X = weight_x<ROB && SOLVE>(a, b, ph, P0X);

  // Bounds.  FUSED: the dynamics row keeps one value (l = u, MPC.py:410); swing
  // rows are 0 = 0; friction rows u = 0, l = -inf (-OSQP_INFTY) or -fz_max.
  // !FUSED: the caller's l / u for every own row.
  double bnd = 0.0;
  [[maybe_unused]] double dacc = 0.0;  // (ROB && FUSED: the lane's disturbance acceleration)
  double lo_g[FUSED ? 1 : 3], hi_g[FUSED ? 1 : 3];
  if (t == 0) { sh.flag[0] = 0; sh.flag[1] = 0; sh.flag[2] = 0; sh.flag[3] = 0; }
  for (int e = t; e < 72; e += T) sh.zero[e] = 0.0;  // N = 4: one wave of 64 lanes
  // The sweep arrays start at zero.  No read depends on it (round 3): the steps a
  // sweep chain does not take re-read slots the chain wrote, and stage 0 reads its
  // absent X_0 terms from sh.zero; the zeroing stays as a guard against LDS left
  // over from an earlier workgroup (NaN / Inf).  -DMPCQ_NO_LDS_ZERO builds without
  // it (tools/build_variant.sh nozero ...: the GPU suite must pass on that build).
#ifndef MPCQ_NO_LDS_ZERO
  for (int e = t; e < (int)(sizeof(sh.u.it) / sizeof(double)); e += T) (&sh.u.it.bo[0][0])[e] = 0.0;
#endif

  // ---- 3. prologue: formulation (FUSED) or the caller's QP --------------------------------------
  if (FUSED || !SOLVE) {
    double* xr = gh0 + Prologue<N>::XR;
    double* fs = gh0 + Prologue<N>::FS;
    int* pos_ = (int*)(gh0 + Prologue<N>::INTS);  // phase_of_stage[N]
    int* con_ = pos_ + N;                         // contact[20][4]
    const double* gx = a.xref + b * 12 * (N + 1);
    const double* gf = a.fsteps + b * 260;
    for (int e = t; e < 12 * (N + 1); e += T) xr[e] = gx[e];
    for (int e = t; e < 260; e += T) fs[e] = gf[e];
    sync_all();
    if (t == 0) {  // construct_gait + phase walk (MPC.py:635-652, 336-352, 626-631)
      int idx = -1;
      for (int j = 0; j < 20; ++j)
        if (fs[13 * j] == 0.0) { idx = j; break; }
      int bad = idx < 0, kk = 0;
      for (int j = 0; j < (idx < 0 ? 0 : idx) && !bad; ++j) {
        const double d = fs[13 * j];
        if (!(fabs(d) < 1e6)) { bad = 1; break; }
        const int di = (int)d;
        if (di < 0) { bad = 1; break; }
        for (int q = 0; q < 4; ++q) {
          const double xv = fs[13 * j + 1 + 3 * q];
          con_[4 * j + q] = !(isnan(xv) || xv == 0.0);
        }
        for (int s_ = 0; s_ < di; ++s_, ++kk)
          if (kk < N) pos_[kk] = j;
      }
      if (kk != N) bad = 1;
      sh.flag[0] = bad ? MPCQ_STATUS_BAD_GAIT : 0;
    }
    sync_all();
    if (sh.flag[0] == 0) {
      for (int e = t; e < 12 * N; e += T) {  // state columns: -I / A (MPC.py:107-115)
        const int kk = e / 12, i = e % 12, xo = XO<N>(kk, i);
        AbW[xo] = -1.0;
        if (kk < N - 1) {
          if (i >= 6) { AbW[xo + 1] = p.dt; AbW[xo + 2] = 1.0; }
          else AbW[xo + 1] = 1.0;
        }
      }
      [[maybe_unused]] RobotK rb;
      if constexpr (ROB) load_robot(a.robots + b, rb);
      for (int e = t; e < 4 * N; e += T) {  // foot q of stage kk
        const int kk = e >> 2, q = e & 3;
        const int j = pos_[kk];
        double lv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          double ft;
          if (first || a.mode == MPCQ_MODE_SETUP)
            ft = q == 0 ? p.footholds[4 * r] : (q == 1 ? p.footholds[4 * r + 1]
                                              : (q == 2 ? p.footholds[4 * r + 2] : p.footholds[4 * r + 3]));
          else {
            ft = fs[13 * j + 1 + 3 * q + r];
            if (isnan(ft)) ft = 0.0;  // MPC.py:327
          }
          lv[r] = ft - xr[r * (N + 1) + kk];
        }
        if constexpr (ROB)
          form_foot(p, rb.mass, rb.gI, rb.mu, xr[5 * (N + 1) + kk], lv[0], lv[1], lv[2],
                    1.0 - (double)con_[4 * j + q], AbW + FO<N>(kk, q, 0));
        else
          form_foot(p, p.mass, p.gI, p.mu, xr[5 * (N + 1) + kk], lv[0], lv[1], lv[2],
                    1.0 - (double)con_[4 * j + q], AbW + FO<N>(kk, q, 0));
      }
      // ROB: row b of the disturbance table, the lane's own component, loaded here once
      if constexpr (ROB) {
        dacc = disturb_a<true>(a, b, ph);
        bnd = dyn_bound<N, true>(p, xr, k, ph, dacc);
      } else {
        bnd = dyn_bound<N>(p, xr, k, ph);
      }
    }
    if (!SOLVE) {
      sync_all();
      if (t == 0 && a.status) a.status[b] = sh.flag[0];
      if (sh.flag[0] != 0) return;
      double* go = a.Ax_out + b * nnz;
      if constexpr (!ABG)
        for (int e = t; e < nnz; e += T) go[e] = sh.Ab[e];
#pragma unroll
      for (int slot = 0; slot < 3; ++slot) {
        const int r = nat_row(slot);
        if (r < 0) continue;
        double l, u;
        if (cl) {
          if (slot == 0) { l = bnd; u = bnd; }
          else if (slot == 1) { l = 0.0; u = 0.0; }
          else { l = -INFINITY; u = 0.0; }
        } else {
          u = 0.0;
          l = slot == 1 ? -fz_max() : -INFINITY;  // l[24N+4::5] = -25 (MPC.py:228)
        }
        a.l_out[b * m + r] = l;
        a.u_out[b * m + r] = u;
      }
      return;
    }
  } else {
    const double* ga = a.Ax + b * nnz;
    for (int e = t; e < nnz; e += T) AbW[e] = ga[e];
    if constexpr (!FUSED) {
#pragma unroll
      for (int slot = 0; slot < 3; ++slot) {
        const int r = nat_row(slot);
        lo_g[slot] = r >= 0 ? a.l[b * m + r] : -kInf;
        hi_g[slot] = r >= 0 ? a.u[b * m + r] : kInf;
      }
    }
  }
  if constexpr (SOLVE) {
    sync_all();
    int status = sh.flag[0];
    {  // non-finite data -> NONFINITE (the problem is always feasible otherwise)
      int bad = 0;
      for (int e = t; e < nnz; e += T)
        if (!isfinite(AbW[e])) bad = 1;
      // (a device weights table is not validated on the way in, unlike mpcq_params' P)
      if constexpr (ROB) {
        if (!(isfinite(P0X) && isfinite(P0f))) bad = 1;
        // (nor a device disturbance table: an Inf would leave bnd infinite, not NaN)
        if (ph >= 6 && !isfinite(dacc)) bad = 1;
      }
      int lgu = 0;  // l > u on an own row (osqp rejects the data)
      if constexpr (FUSED) {
        if (cl && isnan(bnd)) bad = 1;
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (isnan(lo_g[j]) || isnan(hi_g[j])) bad = 1;
          lo_g[j] = lo_g[j] < -kInf ? -kInf : lo_g[j];  // python osqp clamps to +-OSQP_INFTY
          hi_g[j] = hi_g[j] > kInf ? kInf : hi_g[j];
          if (lo_g[j] > hi_g[j]) lgu = 1;
        }
      }
      if (status == 0 && (bad || lgu)) atomicOr(&sh.flag[1], bad ? 1 : 2);
      sync_all();
      if (status == 0 && sh.flag[1]) status = (sh.flag[1] & 1) ? MPCQ_STATUS_NONFINITE : MPCQ_STATUS_BAD_BOUNDS;
    }

    // ---- 4. the iterate, rho and the bounds -----------------------------------------------------
    // persistent per-lane state (column values of c == 3 lanes are shadows)
    double xf = 0.0, xX = 0.0, Df = 1.0, DX = 1.0;
    double z[3] = {0.0, 0.0, 0.0}, y[3] = {0.0, 0.0, 0.0}, E[3] = {1.0, 1.0, 1.0};
    double Fr[12];  // row ph of F_k (S_k^{-1} rows live in LDS: sh.Sm)
#pragma unroll
    for (int j = 0; j < 12; ++j) Fr[j] = 0.0;
    unsigned cls = 0u;
    double cscale = 1.0;
    int it_done = 0, n_upd = 0, pol_st = 0, pol_rounds = 0, admm_st = 0;
#ifdef MPCQ_FACTIME
    uint64_t fac_cycles = 0;
#endif
    // (a resumed slice: the rho and the update count it was suspended with)
    double rho_s = kSlice<N> && a.resume ? a.res_rho[b] : (a.rho_in && !first ? a.rho_in[b] : p.rho);
    rho_s = fmin(fmax(rho_s, kRhoMin), kRhoMax);
    if (kSlice<N> && a.resume) n_upd = a.res_i[8 * b + 3];

    // per-row rho / 1/rho from the row's class and the (uniform) rho values
    double r_in = 0.0, r_eq = 0.0, ri_in = 0.0, ri_eq = 0.0;
    double rr[3], ri[3];  // per-row rho and 1/rho (refreshed with rho)
    auto set_rho = [&]() __attribute__((always_inline)) {
      r_in = uni(rho_s);
      r_eq = uni(kRhoEq * rho_s);
      ri_in = uni(1.0 / r_in);
      ri_eq = uni(1.0 / r_eq);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned cj = (cls >> (2 * j)) & 3u;
        rr[j] = cj == RC_EQ ? r_eq : (cj == RC_INEQ ? r_in : kRhoMin);
        ri[j] = cj == RC_EQ ? ri_eq : (cj == RC_INEQ ? ri_in : 1.0 / kRhoMin);
      }
    };
    auto rho_of_cls = [&](int j) __attribute__((always_inline)) -> double {
      const unsigned cj = (cls >> (2 * j)) & 3u;
      return cj == RC_EQ ? r_eq : (cj == RC_INEQ ? r_in : kRhoMin);
    };
    auto lo_of = [&](int j) __attribute__((always_inline)) -> double {
      if constexpr (FUSED) {
        if (j == 0) return cl ? bnd : -kInf * E[0];
        if (j == 1) return cl ? 0.0 : -fz_max() * E[1];
        return cl ? -kInf * E[2] : -kInf;
      } else {
        return lo_g[j];
      }
    };
    auto hi_of = [&](int j) __attribute__((always_inline)) -> double {
      if constexpr (FUSED) {
        if (j == 0) return cl ? bnd : 0.0;
        if (j == 1) return 0.0;
        return cl ? 0.0 : kInf;
      } else {
        return hi_g[j];
      }
    };

    // Beyond 48 stages (kZcMem: 128 VGPRs) the ADMM loop spills, and the z / y update's
    // per-row constants (bounds, rho, 1/rho) came back as one scratch reload per use,
    // each waited for before the next.  There they are kept in private memory explicitly
    // and read in one batch per use site (zc_ptr: a laundered pointer, so the loads are
    // neither forwarded nor hoisted).
    using pdbl = __attribute__((address_space(5))) double;
    enum { ZC_LO = 0, ZC_HI = 3, ZC_RR = 6, ZC_RI = 9, ZC_COUNT = 12 };
    double zc_mem_[kZcMem<N> ? ZC_COUNT : 1];
    auto zc_ptr = [&]() __attribute__((always_inline)) -> pdbl* {
      pdbl* q = (pdbl*)&zc_mem_[0];
      asm volatile("" : "+v"(q));
      return q;
    };
    auto zc_store = [&]() __attribute__((always_inline)) {
      if constexpr (kZcMem<N>) {
        pdbl* const q = zc_ptr();
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          q[ZC_LO + j] = lo_of(j);
          q[ZC_HI + j] = hi_of(j);
          q[ZC_RR + j] = rr[j];
          q[ZC_RI + j] = ri[j];
        }
      }
    };

    // ---- 5. row and column operators, lane offsets ----------------------------------------------
    // A v for own rows from own forces vf (column lanes), own states vX and the
    // previous stage's states in xs[k]; also returns the force gather.
    auto row_A = [&](double vf, double vX, double (&out)[3]) __attribute__((always_inline)) {
      double fall[12];
      gather12(vf, fall);
      const double* xp = sh.u.it.xs[k];  // xs[0] is never read unmasked
      const double hd = Hd(k, ph), h6 = H6(k, ph);
      const double xa = xp[ph], xb = xp[ph < 6 ? ph + 6 : ph];
      double dyn = Xd(k, ph) * vX;
      const double d1 = dyn + hd * xa;
      const double d2 = d1 + h6 * xb;
      dyn = k >= 1 ? (ph < 6 ? d2 : d1) : dyn;
      double bcf[12];
#pragma unroll
      for (int psi = 0; psi < 12; ++psi) bcf[psi] = Bc(k, ph, psi / 3, psi % 3);
      const double bf = dot12(bcf, fall);
      dyn = ph >= 6 ? dyn + bf : dyn;
      const double g0 = qbc<0>(vf), g1 = qbc<1>(vf), g2 = qbc<2>(vf);
      const double swg = Ab[fo + 4] * vf;
      out[0] = cl ? dyn : fric_row(3, g0, g1, g2);
      out[1] = cl ? swg : fric_row(4, g0, g1, g2);
      out[2] = cl ? fric_row(c, g0, g1, g2) : 0.0;
    };
    auto Pbf = [&]() __attribute__((always_inline)) { return cscale * (Df * P0f * Df); };
    auto PbX = [&]() __attribute__((always_inline)) { return cscale * (DX * P0X * DX); };
    // per-lane constants of the ADMM loop and the residuals: LDS offsets, flags
    const bool hp = k >= 1, isv = ph >= 6;
    const int zXS = (int)(sh.zero - &sh.u.it.xs[0][0]);  // X_0 is not stored: stage 0 reads zeros
    const double m2 = cc == 2 ? 1.0 : 0.0;
    // masked variants for the loop: a lane whose term is structurally absent reads a
    // zero (stage 0 has no previous stage; H6 only on the position rows; the force Schur
    // terms beta, (R^-1 Q) g only on the velocity rows), so no selects are needed
    int zAb;  // offset of a zero block from Ab (masked reads)
    if constexpr (ABG) zAb = Work<N>::ZERO - Work<N>::AB;
    else zAb = (int)(sh.zero - sh.Ab);
    lds_cd* XSr = (lds_cd*)&sh.u.it.xs[0][0];
    double* const Wdump = &sh.dump[t & 63];
    // The LDS offsets of the lane's coefficients, derived from its coordinates.  O0
    // is derived once and held (the loop phases up to 32 stages, where the ADMM loop
    // has the registers); a phase run between long stretches of other work -- the
    // termination check at every N, every loop phase beyond 32 stages (168 VGPRs) --
    // re-derives them from freshly laundered coordinates (MPCQ_LANE_OFFS(true)), a
    // few integer ops each: held across the ADMM loop, the compiler spills them, and
    // each use then waits on its own scratch round trip (the reloads sit right in
    // front of their LDS reads, one after another).
    struct LaneOffs {
      int oXd, oHd, oH6, oF, oFa, oFb, oF4, oFW, oQL, oXSp, oXSp6, rXS, rXSpm, rXSp6m, oHdm, oH6m, oFWcm, oQLm,
          oB0;
      bool ta0;
      double* Wbo;
      double* Wna;
    };
    auto offs = [&]() __attribute__((always_inline)) -> LaneOffs {
      const bool hp_ = k >= 1, isv_ = ph >= 6;
      LaneOffs o;
      o.oXd = xo;                                                 // Xd(k, ph)
      o.oHd = XO<N>(hp_ ? k - 1 : 0, ph) + (ph < 6 ? 1 : 2);      // Hd(k, ph)
      o.oH6 = XO<N>(hp_ ? k - 1 : 0, ph < 6 ? ph + 6 : 11) + 1;   // H6(k, ph)
      o.oF = fo;
      const int ta = c < 3 ? c : 3;  // first own friction row
      o.ta0 = (ta >> 1) == 0;
      o.oFa = FO<N>(k, f, ta >> 1) + 5 + (ta & 1);
      o.oFb = FO<N>(k, f, 2) + 5 + ta;
      o.oF4 = FO<N>(k, f, 2) + 9;
      o.oFW = kFWS<N> * k + 6 * ph;
      const int oFWc = kFWS<N> * k + (isv_ ? ph - 6 : 0);
      o.oQL = 36 * k + 6 * (isv_ ? ph - 6 : 0);
      o.oXSp = 12 * k + ph;  // natural order (update_info)
      o.oXSp6 = 12 * k + (ph < 6 ? ph + 6 : ph);
      // the sweep's states in its slots (SIGX): own X_{k+1}, the previous stage's X_k
      auto xsl = [](int kk) __attribute__((always_inline)) -> int { return 12 * SIGX<N>(kk + 1); };
      o.rXS = xsl(k) + ph;
      o.rXSpm = hp_ ? xsl(k - 1) + ph : zXS;
      o.rXSp6m = hp_ ? xsl(k - 1) + (ph < 6 ? ph + 6 : ph) : zXS;
      o.oHdm = hp_ ? o.oHd : zAb;
      o.oH6m = hp_ && !isv_ ? o.oH6 : zAb;
      o.oFWcm = isv_ ? oFWc : zFW;
      o.oQLm = isv_ ? o.oQL : zQL;
      o.oB0 = FO<N>(k, 0, 0) + (ph >= 9 ? ph - 8 : 0);  // B row ph on force (fp, cp): + 24 fp + 7 cp
      o.Wbo = &sh.u.it.bo[SIG<N>(k)][ph];
      o.Wna = &sh.u.it.na[SIG<N>(hp_ ? k - 1 : N - 1)][ph];
      return o;
    };
    LaneOffs O0 = offs();  // (re-derived at the top of every stretch of iterations up to 32 stages, below)
    // (MPCQ_LANE_OFFS, above the kernel, gives a phase their names: from O0, or re-derived)
    // beyond 32 stages the loop phases re-derive them too
    constexpr bool kRecompLoop = BIG;
    auto launder_p = [&]() __attribute__((always_inline)) {
      lds_uniform(Ab); lds_uniform(GHr); lds_uniform(SmR); lds_uniform(FWr); lds_uniform(QLr); lds_uniform(XSr);
    };
    // force column of A' v for own-row values v (dynamics rows 6..11 by row broadcast,
    // swing, friction by quad broadcast)
    auto colF_c = [&](const double (&A)[10], const double (&v)[3]) __attribute__((always_inline)) -> double {
      const double w6 = rbc<LN(6)>(v[0]), w7 = rbc<LN(7)>(v[0]), w8 = rbc<LN(8)>(v[0]);
      const double w9 = rbc<LN(9)>(v[0]), w10 = rbc<LN(10)>(v[0]), w11 = rbc<LN(11)>(v[0]);
      const double wf0 = qbc<0>(v[2]), wf1 = qbc<1>(v[2]), wf2 = qbc<2>(v[2]);
      const double wf3 = qbc<3>(v[0]), wf4 = qbc<3>(v[1]);
      double sA = A[0] * (cc == 0 ? w6 : (cc == 1 ? w7 : w8));
      double sB = A[1] * w9;
      sA += A[2] * w10;
      sB += A[3] * w11;
      sA += A[4] * v[1];
      sB += A[5] * (cc == 1 ? wf2 : wf0);
      sA += A[6] * (cc == 1 ? wf3 : wf1);
      const double sC = (A[7] * wf2 + A[8] * wf3) + A[9] * wf4;  // friction rows 2..4 (cc == 2)
      return (sA + sB) + m2 * sC;
    };
    // Row maxima of several quantities at once, by a transposing butterfly over the
    // 16-lane row: each step pairs lane s with a partner that differs in one bit
    // (row_mirror: s ^ 15, bit 3; row_half_mirror: s ^ 7, bit 2; quad xor 2, bit 1;
    // quad xor 1, bit 0) and the lanes on either side of that bit keep half of the
    // quantities, so a step reduces half as many values as the one before instead of
    // every quantity taking all four steps (12 quantities: 13 maxima and 13 DPP moves
    // instead of 48 each, for 26 two-way selects instead of 12).  Maxima are exact in
    // any order: the results are the ones the per-quantity reduction gave.
    // one step: lanes with the bit clear keep quantity a, the others b
    auto tstep = [](auto ctrl, double a, double b, bool hi) __attribute__((always_inline)) {
      constexpr int C = decltype(ctrl)::value;
      const double mine = hi ? b : a, send = hi ? a : b;
      return fmax_hw(mine, dppd<C>(send));
    };
    auto sstep = [](auto ctrl, double a) __attribute__((always_inline)) {
      constexpr int C = decltype(ctrl)::value;
      return fmax_hw(a, dppd<C>(a));
    };
    using kMirror = std::integral_constant<int, 0x140>;   // row_mirror (s ^ 15)
    using kHalfMir = std::integral_constant<int, 0x141>;  // row_half_mirror (s ^ 7)
    using kXor2 = std::integral_constant<int, 0x4E>;      // quad_perm [2,3,0,1]
    using kXor1 = std::integral_constant<int, 0xB1>;      // quad_perm [1,0,3,2]
    // six quantities over bits 3, 2, 1: lane s keeps quantity 3 b3 + (b2 ? 2 : b1),
    // maximised over the eight lanes s ^ {0, 15, 7, 8, 2, 13, 5, 10}
    auto tred6 = [&](const double (&v)[6], int s_) __attribute__((always_inline)) {
      const bool h3 = s_ & 8, h2 = s_ & 4, h1 = s_ & 2;
      const double a0 = tstep(kMirror{}, v[0], v[3], h3), a1 = tstep(kMirror{}, v[1], v[4], h3),
                   a2 = tstep(kMirror{}, v[2], v[5], h3);
      const double c0 = tstep(kHalfMir{}, a0, a2, h2), c1 = tstep(kHalfMir{}, a1, a2, h2);
      return tstep(kXor2{}, c0, c1, h1);
    };
    // three quantities over the whole row: lane s keeps x0 on lanes 0..3, x1 on 4..7,
    // x2 on 8..15
    auto tred3 = [&](double x0, double x1, double x2, int s_) __attribute__((always_inline)) {
      const bool h3 = s_ & 8, h2 = s_ & 4;
      const double a0 = tstep(kMirror{}, x0, x2, h3), a1 = tstep(kMirror{}, x1, x2, h3);
      return sstep(kXor1{}, sstep(kXor2{}, tstep(kHalfMir{}, a0, a1, h2)));
    };
    // A v on the own rows for own-column values (vf, vX), the previous stage's states in P
    auto rowA = [&](double vf, double vX, lds_cd* P, double (&ax)[3]) __attribute__((always_inline)) {
      MPCQ_LANE_OFFS(true);
      const int zP = (int)((lds_cd*)sh.zero - P);  // stage 0 has no X_0 term: read zeros, not slot -1
      // every operand of the rows in one batch of loads (up to 32 stages, hold_all): the
      // twelve B coefficients, then the state terms' and the friction / swing rows'
      double L[21];
#pragma unroll
      for (int psi = 0; psi < 12; ++psi) L[psi] = Ab[oB0 + 24 * (psi / 3) + 7 * (psi % 3)];
      L[12] = Ab[oXd]; L[13] = Ab[oHd]; L[14] = P[hp ? oXSp - 12 : zP];
      L[15] = Ab[oH6]; L[16] = P[hp ? oXSp6 - 12 : zP];
      L[17] = Ab[oFb]; L[18] = Ab[oFa]; L[19] = Ab[oF4]; L[20] = Ab[oF + 4];
      if constexpr (!BIG) hold_all(L);
      double bco[12];
#pragma unroll
      for (int psi = 0; psi < 12; ++psi) {
        const int cp = psi % 3;
        bco[psi] = (ph >= 9 || (isv && cp == ph - 6)) ? L[psi] : 0.0;
      }
      const double bfx = bdot_ln12(bco, vf, 0.0);
      double dyn = L[12] * vX;
      const double d1 = dyn + L[13] * L[14];
      const double d2 = d1 + L[15] * L[16];
      dyn = hp ? (isv ? d1 : d2) : dyn;
      dyn = isv ? dyn + bfx : dyn;
      const double q0 = qbc<0>(vf), q1 = qbc<1>(vf), q2 = qbc<2>(vf);
      const double frA = L[17] * q2 + L[18] * (ta0 ? q0 : q1);
      const double frB = L[19] * q2;
      const double swg = L[20] * vf;
      ax[0] = cl ? dyn : frA;
      ax[1] = cl ? swg : frB;
      ax[2] = cl ? frA : 0.0;
    };
    // A' w on the own columns for own-row values w, the next stage's dynamics-row w in W
    auto colAt = [&](const double (&w)[3], const double* W, double& atf, double& atX)
        __attribute__((always_inline)) {
      MPCQ_LANE_OFFS(true);
      const double* wn = W + 12 * (k < N - 1 ? k + 1 : k);
      // the force column's ten coefficients, then the state column's and the next stage's
      // duals: one batch of loads (up to 32 stages, hold_all)
      double L[15];
#pragma unroll
      for (int i = 0; i < 10; ++i) L[i] = Ab[fo + i];
      L[10] = Ab[oXd]; L[11] = Ab[oXd + 1]; L[12] = Ab[oXd + 2];
      L[13] = wn[isv ? ph - 6 : ph]; L[14] = wn[ph];
      if constexpr (!BIG) hold_all(L);
      const double A[10] = {L[0], L[1], L[2], L[3], L[4], L[5], L[6], L[7], L[8], L[9]};
      atf = colF_c(A, w);
      const double sXv = L[10] * w[0];
      const double x1 = sXv + L[11] * L[13];
      const double x2 = x1 + L[12] * L[14];
      atX = k < N - 1 ? (isv ? x2 : x1) : sXv;
    };

    // ---- 6. factorisation -----------------------------------------------------------------------
    // dynamics-row rho of stage kk (published in GH[kk][108..120) at factor time)
    // (stage-keyed scratch: unshifted slots; every read of it precedes the serial
    // steps that overwrite the slots with G / H at SLOT offsets)
    auto rdy = [&](int kk, int i) __attribute__((always_inline)) { return GHr[GS * kk + 108 + i]; };
    auto Qv = [&](int kk, int j1, int j2) __attribute__((always_inline)) { return GHr[GS * kk + 6 * j1 + j2]; };
    // The factorisation's row builders are branch-free: every load is unconditional
    // (indices clamped in range) and the structure is applied by selects.
    // The couplings are sparse: row i of L_kk (and column i) has its nonzeros on
    // column a(i) = i mod 6 and the velocity columns 6..11, so a row is kept as
    // (ca, c6[0..5]).
    // Row i of L_kk (kk >= 1): the dynamics rows of stage kk on (X_{kk+1}[i], X_kk[ci]).
    auto Ctop = [&](int kk, int i, double& ca, double (&c6)[6]) __attribute__((always_inline)) {
      const int iq = i >= 6 ? i - 6 : 0;
      const double ri = rdy(kk, i), xi = Xd(kk, i), hi = Hd(kk, i), h6 = H6(kk, i < 6 ? i : 0);
      const double dv = ri * xi * hi, tv = ri * xi * h6;
      ca = i < 6 ? dv : 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double sc = xi * Qv(kk, iq, j) * Hd(kk, 6 + j);
        const double vv = (6 + j == i ? dv : 0.0) - sc;
        c6[j] = i < 6 ? (j == i ? tv : 0.0) : vv;
      }
    };
    // Column i of L_kk (kk >= 1), i.e. row i of L_kk'.
    auto Cbot = [&](int kk, int i, double& ca, double (&c6)[6]) __attribute__((always_inline)) {
      const int ip = i >= 6 ? i - 6 : 0;
      const double hi = Hd(kk, i);
      const double dv = rdy(kk, i) * Xd(kk, i) * hi;
      const double tv = rdy(kk, ip) * Xd(kk, ip) * H6(kk, ip);
      ca = i < 6 ? dv : tv;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double sc = Xd(kk, 6 + j) * Qv(kk, j, ip) * hi;
        const double vv = (6 + j == i ? dv : 0.0) - sc;
        c6[j] = i >= 6 ? vv : 0.0;
      }
    };
    // Row i of D_kk (the state block of X_{kk+1}).
    auto Drow = [&](int kk, int i, double diag0, double (&Dr)[12]) __attribute__((always_inline)) {
      const bool nx = kk < N - 1;  // stage kk+1 exists
      const int k1 = nx ? kk + 1 : kk;
      const int i6 = i < 6 ? i : i - 6, iq = i >= 6 ? i - 6 : 0;
      const double xi = Xd(kk, i), ri0 = rdy(kk, i);
      const double hi1 = Hd(k1, i), ri1 = rdy(k1, i);
      const double h6p = H6(k1, i6), rp1 = rdy(k1, i6), hp1 = Hd(k1, i6);
      double dg = diag0 + ri0 * xi * xi;
      const double dn = ri1 * hi1 * hi1 + (i >= 6 ? rp1 * h6p * h6p : 0.0);
      dg = nx ? dg + dn : dg;
      const double cross = nx ? (i < 6 ? ri1 * hi1 * h6p : rp1 * hp1 * h6p) : 0.0;
      const int partner = i < 6 ? i + 6 : i - 6;
#pragma unroll
      for (int ci = 0; ci < 12; ++ci) {
        double v = (ci == i) ? dg : 0.0;
        v = (ci == partner) ? cross : v;
        if (ci >= 6) {
          const double s0 = xi * Qv(kk, iq, ci - 6) * Xd(kk, ci);
          const double s1 = hi1 * Qv(k1, iq, ci - 6) * Hd(k1, ci);
          v = i >= 6 ? v - (nx ? s0 + s1 : s0) : v;
        }
        Dr[ci] = v;
      }
    };

    // pr: per-own-row rho override (polish: 1/delta on active rows, 0 elsewhere);
    // nullptr in the ADMM loop, where the class rho applies
    auto factor = [&](double sigma, const double* pr) __attribute__((always_inline)) -> bool {
      bool ok = true;
      launder();
      auto rho_of = [&](int j) __attribute__((always_inline)) -> double {
        return pr ? pr[j] : rho_of_cls(j);
      };
      double* gk = gh0 + GS * k;
      if (cl) gk[108 + ph] = rho_of(0);
      sync_all();
      {  // ---- phase P: F_k = K_ff^{-1} (row ph per column lane), F_k W_k, Q_k
        double rd6[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) rd6[j] = gk[114 + j];
        double rfr[5];
        {
          const double r0 = rho_of(0), r1 = rho_of(1), r2 = rho_of(2);
          rfr[0] = qbc<0>(r2); rfr[1] = qbc<1>(r2); rfr[2] = qbc<2>(r2);
          rfr[3] = qbc<3>(r0); rfr[4] = qbc<3>(r1);
        }
        const double Bo0 = Ab[fo], Bo1 = Ab[fo + 1], Bo2 = Ab[fo + 2], Bo3 = Ab[fo + 3];
        const double sw = Ab[fo + 4];
        const double rsw = rho_of(1);  // swing-row rho (own slot 1)
        double own_fr[5];
#pragma unroll
        for (int t_ = 0; t_ < 5; ++t_) own_fr[t_] = rfr[t_] * Frc(k, f, t_, cc);
        const double dgf = Pbf() + sigma + rsw * sw * sw;
#pragma unroll
        for (int psi = 0; psi < 12; ++psi) {
          const int fp = psi / 3, cp = psi % 3;
          double v = (cp == cc) ? rd6[cp] * Bo0 * Ab[FO<N>(k, fp, cp)] : 0.0;
          v += rd6[3] * Bo1 * Ab[FO<N>(k, fp, cp) + 1];
          v += rd6[4] * Bo2 * Ab[FO<N>(k, fp, cp) + 2];
          v += rd6[5] * Bo3 * Ab[FO<N>(k, fp, cp) + 3];
          if (psi == ph) v += dgf;
          if (fp == f) {
            double fr = 0.0;
#pragma unroll
            for (int t_ = 0; t_ < 5; ++t_) fr += own_fr[t_] * Frc(k, f, t_, cp);
            v += fr;
          }
          Fr[psi] = v;
        }
        gj12<!kBig<N>>(Fr, ph, ok);
        if constexpr (kFrWork<N>) {
#pragma unroll
          for (int i = 0; i < 12; ++i) FRg[16 * NR * i] = Fr[i];
        }
        // F W (row ph): W[psi][j] = rho_{6+j} B[6+j][psi]
        double fw[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          double acc = 0.0;
#pragma unroll
          for (int psi = 0; psi < 12; ++psi) {
            const double bv = Bc(k, 6 + j, psi / 3, psi % 3);
            if (j >= 3 || psi % 3 == j) acc += Fr[psi] * (rd6[j] * bv);
          }
          fw[j] = acc;
        }
        if (cl) {
#pragma unroll
          for (int j = 0; j < 6; ++j) { gk[36 + 6 * ph + j] = fw[j]; FWW[kFWS<N> * k + 6 * ph + j] = fw[j]; }
        }
        wave_sync();
        // Q = W' (F W): 36 entries over the row's 16 lanes
        for (int e = s; e < 36; e += 16) {
          const int j1 = e / 6, j2 = e % 6;
          const double r1 = gk[114 + j1];
          double acc = 0.0;
#pragma unroll
          for (int psi = 0; psi < 12; ++psi)
            acc += (r1 * Bc(k, 6 + j1, psi / 3, psi % 3)) * gk[36 + 6 * psi + j2];
          gk[e] = acc;
          QLW[36 * k + e] = acc / r1;
        }
      }
      const double dgX = PbX() + sigma;
      sync_all();
      STAMP(13);
      // ---- phase S: two-ended block factorisation of the state system.  Per
      // step the active row keeps one 12-vector live (its row of S / U / M):
      // L goes to LDS entry by entry, G / H straight to their GH slot.
      double* const St = sh.u.fa.St;
      double* const Sb = sh.u.fa.Sb;
      // Step j < MID: top row k = j (C = L_k against S_{k-1}^{-1}) and bottom row
      // k = N-1-j > MID (C = L_{k+1}' against U_{k+1}^{-1}) in parallel; step MID:
      // the meeting row (both couplings).  G_k -> GH[k], H_k -> GH[k+1], M^{-1} -> GH[0].
      // One coupling of the active row: upper C = L_k (row ph) against S_{k-1}^{-1}
      // (St), giving G_k -> GH[k]; lower C = L_{k+1}' (row ph) against U_{k+1}^{-1}
      // (Sb), giving H_k -> GH[k+1].  Ro -= (C S^{-1}) C'.  Products run block by
      // block (a compiler fence per block keeps the loads from piling up).
      // Every row's D / L coefficients depend only on its own stage and the next
      // one, all final here: each lane builds its rows before the serial steps
      // (in parallel, one LDS round trip) instead of inside them.
      double Dr0[12], cta, ct6[6], cba, cb6[6];
      Drow(k, ph, dgX, Dr0);
      Ctop(k, ph, cta, ct6);                      // used from k >= 1 only
      Cbot(k < N - 1 ? k + 1 : k, ph, cba, cb6);  // used from k < N-1 only
      auto couple = [&](bool upper, double (&Ro)[12]) __attribute__((always_inline)) {
        const double ca = upper ? cta : cba;
        double c6[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) c6[j] = upper ? ct6[j] : cb6[j];
        const double* const Sp = upper ? St : Sb;
        wave_sync();  // this row's reads of GH[k], GH[k+1] are done
        const int ar = ph < 6 ? ph : ph - 6;
        // two columns at a time: their fourteen operands as seven 16-B reads, loaded
        // together and waited for once, and two independent FMA chains (each column's
        // sum in the same order as one at a time; row blocks waited load by load under
        // the register pressure here)
        double G[12];
        if constexpr (kBig<N>) {  // (beyond 32 stages one column at a time, as gj_step)
#pragma unroll
          for (int ci = 0; ci < 12; ++ci) {
            double sv[7];
            sv[0] = Sp[12 * ar + ci];
#pragma unroll
            for (int j = 0; j < 6; ++j) sv[1 + j] = Sp[12 * (6 + j) + ci];
            double gv = ca * sv[0];
#pragma unroll
            for (int j = 0; j < 6; ++j) gv = fma(c6[j], sv[1 + j], gv);
            G[ci] = gv;
            asm volatile("" ::: "memory");
          }
        } else {
#pragma unroll
        for (int ci = 0; ci < 12; ci += 2) {
          const dbl2 s0 = *(lds_cd2*)(Sp + 12 * ar + ci);
          dbl2 su[6];
#pragma unroll
          for (int j = 0; j < 6; ++j) su[j] = *(lds_cd2*)(Sp + 12 * (6 + j) + ci);
          double g0 = ca * s0.x, g1 = ca * s0.y;
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            g0 = fma(c6[j], su[j].x, g0);
            g1 = fma(c6[j], su[j].y, g1);
          }
          G[ci] = g0;
          G[ci + 1] = g1;
          asm volatile("" ::: "memory");
        }
        }
        if (cl) {
          double* const Gd = gh0 + SLOT<N>(upper ? SIG<N>(k) : SIG<N>(k + 1)) + RS * ph;
#pragma unroll
          for (int ci = 0; ci < 12; ++ci) Gd[ci] = -G[ci];  // stored negated
        }
        schur_cols<!kBig<N>>(Ro, G, ca, c6, std::make_integer_sequence<int, 12>{});
      };
      // Step j < MID: top row k = j and bottom row k = N-1-j > MID in parallel; step
      // MID: the meeting row (both couplings).  M^{-1} -> GH[0].
#pragma nounroll
      for (int j = 0; j <= MID; ++j) {
        launder();
        const bool mid = j == MID;
        const bool top = !mid && k == j, bot = !mid && k == N - 1 - j && k > MID, mrow = mid && k == MID;
        if (top || bot || mrow) {
          const bool useT = (top && k > 0) || mrow, useB = (bot && k < N - 1) || mrow;
          double Ro[12];
#pragma unroll
          for (int ci = 0; ci < 12; ++ci) Ro[ci] = Dr0[ci];
          if (useT) couple(true, Ro);
          if (useB) couple(false, Ro);
          gj12<!kBig<N>>(Ro, ph, ok);
          if (cl) {
#pragma unroll
            for (int ci = 0; ci < 12; ++ci) SmW[SLOT<N>(SIG<N>(k)) + RS * ph + ci] = Ro[ci];
          }
          wave_sync();  // the previous inverse has been consumed by this row
          if (cl) {
            double* dst = mrow ? &sh.GH[0][RS * ph] : (bot ? Sb : St) + 12 * ph;
#pragma unroll
            for (int ci = 0; ci < 12; ++ci) dst[ci] = Ro[ci];
          }
        }
        sync_all();
      }
      STAMP(14);
      // a non-positive pivot anywhere fails the whole instance (uniform result)
      if (!ok) atomicOr(&sh.flag[2], 1);
      sync_all();
      const bool good = sh.flag[2] == 0;
      sync_all();
      return good;
    };

    // ---- 7. scaling: the check's constants, then (status == 0) the Ruiz passes and the start ----
    // The termination check's scaling constants (fixed once the Ruiz scaling is done):
    // D, D^-1 of the own columns, E^-1 of the own rows, the scaled P diagonal, c and
    // 1/c.  Held across the ADMM loop, which does not use them, they were spilled and
    // each use in the check waited on its own scratch reload; they are stored once in
    // private memory instead and read back in a batch at the top of each check phase
    // (through a laundered pointer: never forwarded from the store, so nothing derived
    // from them is hoisted out of the loop either; cached scratch loads, not volatile
    // ones, which would bypass the caches).  Values and rounding are the ones the check
    // computed before (1.0 / Df etc.).
    // (the reciprocals 1 / D, 1 / E and 1 / c are divided again where the check uses them:
    // the same correctly rounded quotients, and 48 B less private memory per lane)
    enum { CK_DF, CK_DX, CK_PBF, CK_PBX, CK_C, CK_E0, CK_E1, CK_E2, CK_BND, CK_COUNT };
    double ck_mem_[CK_COUNT];
    auto ck_ptr = [&]() __attribute__((always_inline)) -> pdbl* {
      pdbl* q = (pdbl*)&ck_mem_[0];
      asm volatile("" : "+v"(q));
      return q;
    };
    // (beyond 32 stages the loop itself is short of registers: there the values are
    // derived where used, as before -- held in memory they cost the loop a spill,
    // N = 48 9.7 -> 10.4 us per iteration, profiles/r03k_iterbench.txt)
    auto ck = [&](int i) __attribute__((always_inline)) -> double {
      if constexpr (BIG) {
        switch (i) {
          case CK_DF: return Df;
          case CK_DX: return DX;
          case CK_PBF: return Pbf();
          case CK_PBX: return PbX();
          case CK_C: return cscale;
          case CK_E0: return E[0];
          case CK_E1: return E[1];
          case CK_E2: return E[2];
          default: return bnd;
        }
      } else {
        return ck_ptr()[i];
      }
    };
    // every constant of the block through one laundered pointer (one batch of loads; the
    // unused ones are dropped by the compiler)
    auto ck_all = [&](double (&cv)[CK_COUNT]) __attribute__((always_inline)) {
      if constexpr (BIG) {
#pragma unroll
        for (int i = 0; i < CK_COUNT; ++i) cv[i] = ck(i);
      } else {
        const pdbl* const q = ck_ptr();
#pragma unroll
        for (int i = 0; i < CK_COUNT; ++i) cv[i] = q[i];
      }
    };

    if (status == 0) {
      STAMP(0);
      // Ruiz scaling
      {
        double Pf = P0f, PX = P0X;
        double* Ex = gh0;  // row factors of this pass: Ex[48 k + 3 s + slot]
        // friction row t of foot fp: owner lane / slot
        auto fr_E = [&](int kk, int fp, int t_) __attribute__((always_inline)) {
          return t_ < 3 ? Ex[48 * kk + 3 * (4 * fp + t_) + 2] : Ex[48 * kk + 3 * (4 * fp + 3) + (t_ - 3)];
        };
        auto dyn_E = [&](int kk, int i) __attribute__((always_inline)) { return Ex[48 * kk + 3 * LN(i)]; };
        auto fr_norm = [&](int t_) __attribute__((always_inline)) {
          double v = fabs(Ab[FO<N>(k, f, 2) + 5 + t_]);
          if (t_ < 4) v = fmax(v, fabs(Ab[FO<N>(k, f, t_ >> 1) + 5 + (t_ & 1)]));
          return v;
        };
        for (int it = 0; it < p.scaling; ++it) {
          double dtf = fabs(Pf);
          {
            const int cnt = cc < 2 ? 7 : 10;
            for (int e = 0; e < cnt; ++e) dtf = fmax(dtf, fabs(Ab[fo + e]));
          }
          double dtx = fabs(PX);
          {
            const int cnt = (k < N - 1) ? (ph < 6 ? 2 : 3) : 1;
            for (int h = 0; h < cnt; ++h) dtx = fmax(dtx, fabs(Ab[xo + h]));
          }
          double et[3];
          {
            double v = fabs(Xd(k, ph));
            if (k >= 1) {
              v = fmax(v, fabs(Hd(k, ph)));
              if (ph < 6) v = fmax(v, fabs(H6(k, ph)));
            }
            if (ph >= 6) {
#pragma unroll
              for (int psi = 0; psi < 12; ++psi) v = fmax(v, fabs(Bc(k, ph, psi / 3, psi % 3)));
            }
            et[0] = cl ? v : fr_norm(3);
            et[1] = cl ? fabs(Ab[fo + 4]) : fr_norm(4);
            et[2] = cl ? fr_norm(c) : 0.0;
          }
          dtf = dtf < kMinScaling ? 1.0 : (dtf > kMaxScaling ? kMaxScaling : dtf);
          dtx = dtx < kMinScaling ? 1.0 : (dtx > kMaxScaling ? kMaxScaling : dtx);
          dtf = 1.0 / sqrt(dtf);
          dtx = 1.0 / sqrt(dtx);
          Df *= dtf;
          DX *= dtx;
          Pf = dtf * Pf * dtf;
          PX = dtx * PX * dtx;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            double v = et[j];
            v = v < kMinScaling ? 1.0 : (v > kMaxScaling ? kMaxScaling : v);
            et[j] = 1.0 / sqrt(v);
            E[j] *= et[j];
          }
#pragma unroll
          for (int j = 0; j < 3; ++j) Ex[48 * k + 3 * s + j] = et[j];
          sync_all();
          if (cl && !phantom) {  // own columns: E_row A D_col (in place: phantom rows keep out)
            const double dA = dyn_E(k, 6 + cc);
            AbW[fo] = dA * AbW[fo] * dtf;
#pragma unroll
            for (int j = 0; j < 3; ++j) AbW[fo + 1 + j] = dyn_E(k, 9 + j) * AbW[fo + 1 + j] * dtf;
            AbW[fo + 4] = et[1] * AbW[fo + 4] * dtf;
            if (cc < 2) {
              AbW[fo + 5] = fr_E(k, f, 2 * cc) * AbW[fo + 5] * dtf;
              AbW[fo + 6] = fr_E(k, f, 2 * cc + 1) * AbW[fo + 6] * dtf;
            } else {
#pragma unroll
              for (int t_ = 0; t_ < 5; ++t_) AbW[fo + 5 + t_] = fr_E(k, f, t_) * AbW[fo + 5 + t_] * dtf;
            }
            AbW[xo] = et[0] * AbW[xo] * dtx;
            if (k < N - 1) {
              if (ph >= 6) {
                AbW[xo + 1] = dyn_E(k + 1, ph - 6) * AbW[xo + 1] * dtx;
                AbW[xo + 2] = dyn_E(k + 1, ph) * AbW[xo + 2] * dtx;
              } else {
                AbW[xo + 1] = dyn_E(k + 1, ph) * AbW[xo + 1] * dtx;
              }
            }
          }
          // cost scaling: c = 1 / max(mean |P|, 1)  (q = 0)
          double ps = cl && !phantom ? fabs(Pf) + fabs(PX) : 0.0;
          ps = wave_sum(ps);
          if ((t & 63) == 0) sh.red[wv] = ps;
          sync_all();
          ps = 0.0;
#pragma unroll
          for (int w = 0; w < NW; ++w) ps += sh.red[w];
          const double mean = ps / n;
          double ctmp = mean > 1.0 ? mean : 1.0;
          ctmp = ctmp < kMinScaling ? 1.0 : (ctmp > kMaxScaling ? kMaxScaling : ctmp);
          ctmp = 1.0 / ctmp;
          Pf *= ctmp;
          PX *= ctmp;
          cscale = uni(cscale * ctmp);
          sync_all();
        }
      }
      // scaled bounds, constraint classes (osqp set_rho_vec)
      if constexpr (FUSED) {
        bnd *= E[0];
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) { lo_g[j] *= E[j]; hi_g[j] *= E[j]; }
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double lj = lo_of(j), hj = hi_of(j);
        unsigned cj;
        if (lj < -kInf * kMinScaling && hj > kInf * kMinScaling) cj = RC_LOOSE;
        else if (hj - lj < kRhoTol) cj = RC_EQ;
        else cj = RC_INEQ;
        cls |= cj << (2 * j);
      }
      set_rho();
      zc_store();
      if constexpr (!BIG) {
        pdbl* const q = ck_ptr();
        q[CK_DF] = Df; q[CK_DX] = DX; q[CK_PBF] = Pbf(); q[CK_PBX] = PbX(); q[CK_C] = cscale;
        q[CK_E0] = E[0]; q[CK_E1] = E[1]; q[CK_E2] = E[2]; q[CK_BND] = bnd;
      }
      // warm start (osqp_warm_start: x = D^-1 x0, z = A x; y = c E^-1 y0)
      if (a.warm_x && !first) {
        xf = a.warm_x[b * n + colF] / Df;
        xX = a.warm_x[b * n + colX] / DX;
        if (cl) sh.u.it.xs[k + 1][ph] = xX;
        sync_all();
        row_A(xf, xX, z);
        if (!cl) z[2] = 0.0;
        sync_all();
      }
      if (a.warm_y && !first) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int r = nat_row(j);
          // dual_warm = 1: osqp's workspace y from the previous solve, kept as is across the
          // re-scaled update(Ax=) (MPC.py:419-420); 0: osqp_warm_start_y's scaling
          const double wy = r >= 0 ? a.warm_y[b * m + r] : 0.0;
          y[j] = r >= 0 ? (p.dual_warm ? wy : cscale * wy / E[j]) : 0.0;
        }
      }
      // a resumed slice (mpcq_set_slice): the iterate every lane held when it was suspended
      if constexpr (kSlice<N>) {
        if (a.resume) {
          constexpr int64_t RL = res_lanes(N);
          const double* const q = a.res + b * 8 * RL + t;
          xf = q[0];
          xX = q[RL];
#pragma unroll
          for (int j = 0; j < 3; ++j) { z[j] = q[(2 + j) * RL]; y[j] = q[(5 + j) * RL]; }
        }
      }
      sync_all();
      STAMP(1);

      // ---- 8. the loop phases: ph_rhs, ph_sweep (lag / split), ph_recover -----------------------
      // The phases of one KKT solve (K w = b, K = P + sigma I + A'RA as factored):
      // ph_rhs publishes the sweep right-hand sides of b = xc + A' w (P1-P4), ph_sweep
      // runs the state sweeps (P5-P7), ph_recover the forces and A w on the own rows
      // (P8, P9's first half).  The ADMM loop calls them with admm = true (w = rho z - y,
      // xc = sigma x); polish with its own w and x terms.
      // the iteration-invariant LDS operands of ph_rhs (A_f column, F W column, the
      // state column's dynamics coefficients)
      // (kColfFold, round 5) A_f's first coefficient masked by the force component: cf0m[j] =
      // cf[0] on the lanes of component j (2: every other), else 0, so the component-dependent
      // row broadcast of colF folds into v_fmac_f64_dpp.  With the right-hand-side phase's
      // pointer laundering dropped (below) the phase lost ~40 instructions per wave and
      // iteration: same box (profiles/r05p_*, r05q_*), N = 16 1.851-1.872 -> 1.788-1.791 us
      // per iteration alone, 2.18-2.21 -> 2.134-2.142 at two per CU, N = 32 3.105-3.124 ->
      // 2.966-2.982; C2 125.3 k -> 130.7 k QP/s.  The same terms in the same order (the
      // compiler's own contraction of colF had rounded A_2 w_10 first, so the last bits of
      // b_f differ from round 4's); statuses and iterations equal to the oracle's.  Up to 32
      // stages: beyond, that last-bit change moved the N = 48 session loop's fifth tick
      // 1.01e-7 from the oracle (its test allows 1e-7; r05r), and the loop reads its operands
      // per iteration there anyway.  Dropping the checks' laundering as well was slower at
      // N = 32 (3.06 us, r05q).
      constexpr bool kColfFold = !BIG;
      struct RhsOps {
        double cf[10], fwc[12], cXd, cHd, cH6;
        double cf0m[kColfFold ? 3 : 1];
      };
      auto load_rhs_ops = [&](RhsOps& o) __attribute__((always_inline)) {
        MPCQ_LANE_OFFS(true);  // (once per stretch of iterations)
#pragma unroll
        for (int i = 0; i < 10; ++i) o.cf[i] = Ab[oF + i];
        if constexpr (kColfFold) {
          const int cs = cc == 0 ? 0 : (cc == 1 ? 1 : 2);
#pragma unroll
          for (int j = 0; j < 3; ++j) o.cf0m[j] = cs == j ? o.cf[0] : 0.0;
        }
#pragma unroll
        for (int psi = 0; psi < 12; ++psi) o.fwc[psi] = FWr[oFWcm + 6 * psi];
        o.cXd = Ab[oXd];
        o.cHd = Ab[oHdm];
        o.cH6 = Ab[oH6m];
      };
      // o: the operands held in registers (the ADMM loop), or null: read them here (polish,
      // whose loop would otherwise spill them)
      auto ph_rhs = [&](bool admm, const RhsOps* op, const double (&pw)[3], double xcf, double xcX, double& uf,
                        double& beta) __attribute__((always_inline)) {
          // (up to 48 stages no launder_p here since round 5: the laundered base pointers
          // cost ~40 instructions per iteration and the loop has no spill without them; beyond
          // 48 stages, at 128 VGPRs, the iteration was 15.0 -> 16.9 us without, r05r)
          if constexpr (kFrWork<N>) launder_p();
          RhsOps own_;
          if (!op) load_rhs_ops(own_);
          const RhsOps& o = op ? *op : own_;
          MPCQ_LANE_OFFS(kRecompLoop);
          // beyond 48 stages (kFrWork) the F_k row is read from the workspace here (issued first,
          // its latency behind the phase's other loads) instead of being held through
          // the ADMM loop in 24 of the 128 VGPRs
          double frg[12];
          if constexpr (kFrWork<N>) {
            g_cd* q = FRg;
            asm volatile("" : "+v"(q));
#pragma unroll
            for (int i = 0; i < 12; ++i) frg[i] = q[16 * NR * i];
          }
          // P1-P4: w = rho z - y; b_f = sigma x_f + A_f' w and u = F b_f, beta = R B u
          // (stage-local, DPP only); then the sweep right-hand side of the own state
          // column (bo) and this stage's dynamics-row terms of stage k-1's state
          // columns (na, nb): the only LDS hand-off before the sweeps.
          // every LDS operand of this phase is iteration-invariant: issue all the loads
          // first (one LDS round trip instead of one per use)
          const double cXd = o.cXd, cHd = o.cHd, cH6 = o.cH6;
          double w[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) w[j] = admm ? rr[j] * z[j] - y[j] : pw[j];
          if constexpr (kZcMem<N>) {
            if (admm) {
              pdbl* const q = zc_ptr();
              const double r0 = q[ZC_RR], r1 = q[ZC_RR + 1], r2 = q[ZC_RR + 2];
              w[0] = r0 * z[0] - y[0];
              w[1] = r1 * z[1] - y[1];
              w[2] = r2 * z[2] - y[2];
            }
          }
          // the phase's arithmetic starts after this point, the loads before it
          asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]) : : "memory");
          double colf;
          if constexpr (kColfFold) {
            // colF_c's six row-broadcast terms folded into v_fmac_f64_dpp (the masked terms
            // add exact zeros); the quad-broadcast terms as there
            double sA = -0.0, sB = -0.0;
            asm("s_nop 1\n\t"
                "v_fmac_f64_dpp %0, %2, %3 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                "v_fmac_f64_dpp %1, %2, %4 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                "v_fmac_f64_dpp %0, %2, %5 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                "v_fmac_f64_dpp %1, %2, %6 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                "v_fmac_f64_dpp %0, %2, %7 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                "v_fmac_f64_dpp %0, %2, %8 row_newbcast:13 row_mask:0xf bank_mask:0xf"
                : "+v"(sA), "+v"(sB)
                : "v"(w[0]), "v"(o.cf0m[0]), "v"(o.cf[1]), "v"(o.cf0m[1]), "v"(o.cf[3]), "v"(o.cf0m[2]),
                  "v"(o.cf[2]));
            static_assert(LN(6) == 8 && LN(7) == 9 && LN(8) == 10 && LN(9) == 12 && LN(10) == 13 && LN(11) == 14,
                          "the broadcast lanes above");
            const double wf1 = qbc<1>(w[2]), wf2 = qbc<2>(w[2]);
            const double wf3 = qbc<3>(w[0]), wf4 = qbc<3>(w[1]);
            // cc == 1 ? wf2 : wf0 as one quad permute (cc is the lane's place in its quad,
            // lane 3 shadowing lane 2): two DPP moves instead of four and two selects
            const double wf02 = qperm<0, 2, 0, 0>(w[2]);
            const double* const A = o.cf;
            sA += A[4] * w[1];
            sB += A[5] * wf02;
            sA += A[6] * (cc == 1 ? wf3 : wf1);
            const double sC = (A[7] * wf2 + A[8] * wf3) + A[9] * wf4;
            colf = (sA + sB) + m2 * sC;
          } else {
            colf = colF_c(o.cf, w);
          }
          const double bf = colf + (admm ? p.sigma * xf : xcf);  // b_f = sigma x_f + A_f' w (- q, q = 0)
          // u = F b_f (kept for the forces) and beta = R B u = (F W)' b_f (rows 6..11)
          if constexpr (kFrWork<N>) {
            uf = bdot_ln12(frg, bf, 0.0);
          } else {
            uf = bdot_ln12(Fr, bf, 0.0);
          }
          beta = bdot_ln12(o.fwc, bf, 0.0);
          {
            const double wd = w[0] - beta;  // dynamics-row w less the force Schur term (beta = 0 on rows 0..5)
            const double bo = (admm ? p.sigma * xX : xcX) + cXd * wd;
            const double na = cHd * wd;                  // Hd(k, ph): on X_k[ph], stage k-1's column ph
            const double nb = cH6 * w[0];                // H6(k, ph): on X_k[ph+6] (ph < 6)
            // stage 0 zeroes the last stage's na / nb (that stage has no next stage:
            // its coefficients read zero)
            *(cl ? Wbo : Wdump) = bo;
            // stage k-1's component r takes na of lane r and nb of the lane 8 away in the
            // row (component r -+ 6, LN): summed here, one value and one add less per
            // sweep step
            const double nbx = dppd<0x128>(nb);  // row_ror:8
            *(cl ? Wna : Wdump) = na + nbx;
          }
          // (the barrier that publishes bo / na / nb opens ph_sweep)
      };
      auto ph_sweep_lag = [&]() __attribute__((always_inline)) {
          // P5-P7: the state solve on wave 0 alone (no block barrier inside), up to 32
          // stages (beyond: ph_sweep_split).
          // Inward step j = 1..MID: top kk(j) = j, bottom kk(j) = N-1-j.  Half 0 (rows
          // 0 top / 1 bottom) runs the recurrence y_kk = b_kk - G_kk y_kk(j-1) (G_kk of
          // the top in GH[kk], H_kk of the bottom in GH[kk+1], stored negated), one
          // full 12-term row per lane.  Half 1 (rows 2 / 3) runs the same instruction
          // stream on S^{-1} rows two stages behind: w_kk(j-2) = S^{-1} y_kk(j-2), its y
          // handed over by permlane32_swap.  Step MID+1 is the meeting stage: half 0
          // solves x_m = M^{-1} (y_m + v_m - b_m) (top and bottom rows joined by
          // permlane16_swap), half 1 the last top w.  Then the outward sweeps.
          const int half = (t >> 5) & 1;
#pragma nounroll
          for (int rep_ = 0; rep_ < MPCQ_REP_SWEEP; ++rep_) {  // > 1: timing experiments only
          double xp = 0.0;
          // Step-ordered bases (SIG): step j's rows / right-hand sides / w / X are at
          // base + j * stride for every lane, an immediate offset.  Half 0: G_j (top,
          // slot j) / H_{N-1-j} (bottom, slot MID+j); half 1: S^{-1} of stage kk(j-2),
          // top slot j-2 / bottom slot MID-1+j.  Step 1's rows are iteration-invariant:
          // wave 0 reads them before the barrier that publishes the right-hand sides.
          // (N > 32: S^{-1} is global, so the row pointer is a generic one)
          using swp = lds_cd;
          using swp2 = lds_cd2;
          swp* const GHs = GHr;
          // (the bottom chain's slots are past N/2: +2, SLOT)
          swp* const Mb = half == 0 ? GHs + (GS * (cr == 0 ? 0 : MID) + (cr == 0 ? 0 : kSlotPad<N>) + RS * rr_)
                                    : (swp*)&sh.Sm[0][0] + (GS * (cr == 0 ? -2 : MID - 1) + (cr == 0 ? 0 : kSlotPad<N>) + RS * rr_);
          double g[12];
          auto row12 = [&](swp* q) __attribute__((always_inline)) {  // 16-B aligned row: 6 ds_read_b128
#pragma unroll
            for (int i = 0; i < 6; ++i) {
              const dbl2 v = ((swp2*)q)[i];
              g[2 * i] = v.x;
              g[2 * i + 1] = v.y;
            }
          };
          // the rows of step j (j a constant after unrolling): every lane reads a slot the
          // factorisation wrote -- the steps a chain does not take (half 1's first step,
          // the bottom chain's steps past its BOT stages at even N) re-read a row of the
          // chain's own, and their products are discarded by the hand-off select / the sink
          auto rowp = [&](int j) __attribute__((always_inline)) -> swp* {
            if (j >= 2 && j <= BOT) return Mb + GS * j;
            const int jj = half == 0 ? (cr == 0 ? j : (j < BOT ? j : BOT))
                                     : (cr == 0 ? (j > 2 ? j : 2) : (j < BOT + 1 ? j : BOT + 1));
            return Mb + GS * jj;
          };
          STAMP(15);  // (diagnostic builds: as in ph_sweep_split)
          if (t < 64) row12(rowp(1));
          sync_all();
          STAMP(3);
          // outward step j reads G_{MID-j+1}' (top, slot MID+1-j) / H_{MID+j-1}'
          // (bottom, slot N-j) columns: Ob + (MID - j) GS (LDS offsets are unsigned,
          // so the bases sit at the lowest slot a chain reaches)
          lds_cd* const Ob = GHr + (GS * (cr == 0 ? 1 : N - MID) + (cr == 0 ? 0 : kSlotPad<N>) + rr_);
          if (t < 64) {
            // the sweeps are every wave's critical path (the other waves of the
            // instance wait at the barrier): issue them ahead of a co-resident
            // instance's stage-parallel phases
            __builtin_amdgcn_s_setprio(3);
            // right-hand side of step j: top stage j (slot j), bottom stage N-1-j (slot
            // MID+1+j, except the meeting stage MID at the bottom's last step BOT, slot
            // MID, which the bottom re-reads in the steps it does not take); na at +12N
            lds_cd* const Bb = (lds_cd*)&sh.u.it.bo[0][0] + (12 * (cr == 0 ? 0 : MID + 1) + rr_);
            lds_cd* const Bm = (lds_cd*)&sh.u.it.bo[0][0] + (12 * MID + rr_);
            auto rhs = [&](int j) __attribute__((always_inline)) -> lds_cd* {  // j: a constant
              return (j >= BOT && cr != 0) ? Bm : Bb + 12 * j;
            };
            // w of stage kk(j-2) (half 1): top slot j-2, bottom slot MID-1+j; the other
            // lanes store into the sink with the same stride
            lds_d* const sink = (lds_d*)&sh.red[0] + (t & 31);
            lds_d* const Yb = (half == 1 && s < 12) ? (lds_d*)&sh.u.it.yv[0][0] + (12 * (cr == 0 ? -2 : MID - 1) + rr_)
                                                    : sink;
            // step MID+1's store: every lane has one target, so it is one store and no branch
            lds_d* const Ym = ((N & 1) || cr == 0) ? Yb + 12 * (MID + 1) : sink;
            lds_d* const Pm = (half == 0 && cr == 0 && s < 12)
                                  ? (lds_d*)&sh.u.it.xs[0][0] + (12 * SIGX<N>(MID + 1) + rr_) : Ym;
            // right-hand sides run two steps ahead: step j sums the one of step j+1
            // (loaded during step j-1) and loads the one of step j+2; half 1 (the w
            // products) starts its chain from 0.  The first two (y_kk(0) and step 1's)
            // are loaded together and waited for once: they were published by the
            // barrier just passed, so this round trip is on the critical path.
            const double m0 = half == 0 ? 1.0 : 0.0;
            double s0 = rhs(0)[0], s1 = rhs(0)[12 * N];
            double c0 = rhs(1)[0], c1 = rhs(1)[12 * N];
            double src = half == 0 ? s0 + s1 : 0.0;  // y_kk(0) (half 0)
            double bcn = add_mul_here(c0, c1, m0);
            double b0 = rhs(2)[0], b1 = rhs(2)[12 * N];
#pragma unroll
            for (int j = 1; j <= MID + 1; ++j) {
              asm volatile("" : : : "memory");
              double gc[12];
#pragma unroll
              for (int i = 0; i < 12; ++i) gc[i] = g[i];
              const double bc = j <= MID ? bcn : 0.0;
              if (j < MID) {  // prefetch the next step's rows
                row12(rowp(j + 1));
              } else if (j == MID) {  // the meeting step: M^{-1} rows (half 0), the S walk (half 1)
                row12(half == 0 ? GHs + RS * rr_ : rowp(MID + 1));
                lds_cd* qb = (lds_cd*)&sh.u.it.bo[0][0] + (12 * MID + rr_);
                b0 = qb[0]; b1 = qb[12 * N];
              } else {  // the last step: the first outward step's columns
#pragma unroll
                for (int i = 0; i < 12; ++i) g[i] = Ob[RS * i + GS * (MID - 1)];
              }
              asm volatile("" : : : "memory");  // the prefetch is issued here, not sunk to its use
              double s_in = src;
              if (j == MID + 1) s_in = half == 0 ? row_pair_sum(src) - (b0 + b1) : src;
              const double acc = bdot12(gc, s_in, bc);
              // the next right-hand side is summed after the chain: its loads were
              // issued at the end of the previous step, and summing them ahead of the
              // chain would put their LDS latency on the critical path
              // (the sum and its mask as a volatile asm, which keeps its place behind the chain's
              // block: an empty-asm launder of b0 / b1 did too, but it redefines them, and the
              // compiler then copied the first pair and put a wait state in front of every sum)
              if (j < MID) bcn = add_mul_here(b0, b1, m0);
              if (j + 2 <= MID) {
                b0 = rhs(j + 2)[0]; b1 = rhs(j + 2)[12 * N];
              }
              if (j >= 2 && j <= MID) {  // half 1: w of stage kk(j-2)
                Yb[12 * j] = acc;
              } else if (j == MID + 1) {
                // the last step's one store: x_m from row 0's state lanes, half 1's last w
                // (even N: the bottom's kk(MID-1) is the meeting stage, no w), else the sink
                *Pm = acc;
              }
              if (j <= MID) {
                // half 0 continues with y_kk(j) (the bottom chain stops after step BOT), half 1
                // receives y_kk(j-1) from half 0
                const bool adv = j <= BOT || cr == 0;
                src = keep_lo_take_lo(adv ? acc : src, src);
                // (the hand-off stays ahead of the next step's row reads: with the reads
                // between it and the chain, the chain's opening s_nop is dropped, nop_elide.py)
                asm volatile("" : "+v"(src));
              } else {
                xp = acc;
              }
            }
            STAMP(6);
          }
          if (t < 64) {
            // Outward step j: top kk = MID-j: X_kk = w_kk - G_{kk+1}' X_{kk+1}; bottom
            // kk = MID+j: X_kk = w_kk - H_{kk-1}' X_{kk-1} (columns from Ob - j GS).  Lane
            // rr reads column rr (a full 12-term product per lane; half 1 repeats half 0).
            // w of stage kk: top slot MID-j, bottom slot N-j (Wb - 12 j); X_kk = xs[kk+1]:
            // top slot MID+1-j, bottom slot N-j (SIGX; Xb - 12 j).  The bottom row's last
            // step (kk = N) is idle: its store goes to the sink.
            // (bases at step MID's slot: step j at base + 12 (MID - j))
            lds_cd* const Wb = (lds_cd*)&sh.u.it.yv[0][0] + (12 * (cr == 0 ? 0 : N - MID) + rr_);
            lds_d* const sinkO = (lds_d*)&sh.red[0] + (t & 31);
            lds_d* const Xb = (half == 0 && s < 12) ? (lds_d*)&sh.u.it.xs[0][0] + (12 * (cr == 0 ? 1 : N - MID) + rr_)
                                                    : sinkO;
            wave_sync();  // the w written by half 1
            double bq = Wb[12 * (MID - 1)];
#pragma unroll
            for (int j = 1; j <= MID; ++j) {
              asm volatile("" : : : "memory");
              double gc[12];
#pragma unroll
              for (int i = 0; i < 12; ++i) gc[i] = g[i];
              const double bc = bq;
              if (j < MID) {
#pragma unroll
                for (int i = 0; i < 12; ++i) g[i] = Ob[RS * i + GS * (MID - j - 1)];
                // (even N: the bottom chain has no step MID; it re-reads its last w)
                if (j + 1 <= BOT) bq = Wb[12 * (MID - j - 1)];
                else bq = Wb[12 * (MID - (cr == 0 ? j + 1 : BOT))];
              }
              asm volatile("" : : : "memory");
              const double acc = bdot12(gc, xp, bc);  // x = w - G' x_next with -G stored
              if (j < MID) {
                xp = acc;
                Xb[12 * (MID - j)] = acc;
              } else if constexpr (N & 1) {
                *Xb = acc;
              } else {  // even N: the bottom chain has no step MID
                *(cr == 0 ? Xb : sinkO) = acc;
              }
            }
            __builtin_amdgcn_s_setprio(0);
          }
          wave_sync();
          }  // MPCQ_REP_SWEEP
      };
      auto ph_sweep_split = [&]() __attribute__((always_inline)) {
          // P5-P7: the state solve.  The two chains run on wave 0, each on a pair of rows
          // that splits every 12-term row product in two: rows 0 / 1 (top / bottom chain)
          // take the first six terms and the right-hand side, rows 2 / 3 the last six, and
          // one permlane32 swap-add joins the halves (rows 0 + 2, 1 + 3).  Rows 2 / 3 hold
          // the chain vector rotated by six lanes (row_ror:10), so both halves broadcast
          // from lanes 0..5 with the same instruction.  Inward step j = 1..MID: y_kk =
          // b_kk - G_kk y_kk(j-1) (top kk = j, G_kk in GH slot j; bottom kk = N-1-j, H_kk
          // in slot MID+j, stopping after BOT steps), each y stored to its stage's yv slot;
          // step MID+1: the meeting stage x_m = M^{-1} (y_m + v_m - b_m) (the two pairs
          // joined by permlane16).  Then, on every wave, w_k = S_k^{-1} y_k stage-parallel
          // (one barrier pair); then the outward steps x_kk = w_kk - G' x_next on wave 0.
          // Used beyond 32 stages, where S^{-1} lives in L2 (N = 48: 13.9 -> 12.9 us per
          // iteration); up to 32 stages ph_sweep_lag is faster (N = 16: 1.90 vs 2.31 us,
          // N = 32: 3.31 vs 3.92, profiles/r03h_iterbench.txt): the split saves six FMAs and
          // three row reads per step but adds the swap-add, the rotation and the selects,
          // and the stage-parallel S^{-1} phase with its two barriers.
          int tl_ = t;  // (laundered: the lane ids derived here are not hoisted out of the loop and spilled)
          asm volatile("" : "+v"(tl_));
          const int hi = (tl_ >> 5) & 1;  // rows 2 / 3: the second six terms
          const int h6 = 6 * hi;
#pragma nounroll
          for (int rep_ = 0; rep_ < MPCQ_REP_SWEEP; ++rep_) {  // > 1: timing experiments only
          double xp = 0.0;
          double g[6];
          // lane rr of a row reads entries h6..h6+5 of row rr of the step's matrix
          // (16-B aligned: 3 ds_read_b128); the bottom chain's slots sit past N/2 (+2, SLOT)
          lds_cd* const Mb = GHr + (GS * (cr == 0 ? 0 : MID) + (cr == 0 ? 0 : kSlotPad<N>) + RS * rr_ + h6);
          auto row6 = [&](lds_cd* q) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              const dbl2 v = ((lds_cd2*)q)[i];
              g[2 * i] = v.x;
              g[2 * i + 1] = v.y;
            }
          };
          // step j's rows (j a constant after unrolling); the bottom chain's steps past BOT
          // (even N) re-read its last matrix, their products discarded by the hand-off select
          auto rowp = [&](int j) __attribute__((always_inline)) -> lds_cd* {
            if (j <= BOT) return Mb + GS * j;
            return Mb + GS * (cr == 0 ? j : BOT);
          };
          STAMP(15);  // (diagnostic builds: the own right-hand side, then the wait for the others)
          if (t < 64) row6(rowp(1));
          sync_all();
          STAMP(3);
          // outward step j reads G_{MID-j+1}' (top, slot MID+1-j) / H_{MID+j-1}' (bottom,
          // slot N-j): column rr, entries h6..h6+5 (LDS offsets are unsigned, so the bases
          // sit at the lowest slot a chain reaches)
          lds_cd* const Ob = GHr + (GS * (cr == 0 ? 1 : N - MID) + (cr == 0 ? 0 : kSlotPad<N>) + rr_ + RS * h6);
          // (kLagOut) the same columns read whole: lane rr takes all 12 entries of column rr
          [[maybe_unused]] lds_cd* const ObL = GHr + (GS * (cr == 0 ? 1 : N - MID) + (cr == 0 ? 0 : kSlotPad<N>) + rr_);
          [[maybe_unused]] double go[kLagOut<N> ? 12 : 1];
          if (t < 64) {
            // the sweeps are every wave's critical path (the other waves of the instance
            // wait at the barrier): issue them ahead of a co-resident instance's phases
            __builtin_amdgcn_s_setprio(3);
            // right-hand side of step j (rows 0 / 1 add it): top stage j (slot j), bottom
            // stage N-1-j (slot MID+1+j; the meeting stage MID at the bottom's step BOT,
            // slot MID, which the bottom re-reads in the steps it does not take); na at +12N
            lds_cd* const Bb = (lds_cd*)&sh.u.it.bo[0][0] + (12 * (cr == 0 ? 0 : MID + 1) + rr_);
            lds_cd* const Bm = (lds_cd*)&sh.u.it.bo[MID][rr_];
            auto rhs = [&](int j) __attribute__((always_inline)) -> lds_cd* {  // j: a constant
              return (j >= BOT && cr != 0) ? Bm : Bb + 12 * j;
            };
            // the index a lane holds in the broadcast layout (rows 2 / 3: rotated by six)
            const int ri = hi ? (rr_ < 6 ? rr_ + 6 : rr_ - 6) : rr_;
            lds_d* const sink = (lds_d*)&sh.red[0] + (t & 31);
            // y of step j's stage from rows 0 / 1 (top slot j, bottom slot MID+1+j: SIG)
            lds_d* const Yh = (hi == 0 && s < 12) ? (lds_d*)&sh.u.it.yv[0][0] + (12 * (cr == 0 ? 0 : MID + 1) + rr_)
                                                  : sink;
            // y_kk(0) = b of the chain's first stage, in the broadcast layout; the next two
            // right-hand sides in the output layout (published by the barrier just passed:
            // loaded together, waited for once)
            lds_cd* const B0 = (lds_cd*)&sh.u.it.bo[0][0] + (12 * (cr == 0 ? 0 : MID + 1) + ri);
            double s0 = B0[0], s1 = B0[12 * N];
            double c0 = rhs(1)[0], c1 = rhs(1)[12 * N];
            asm volatile("" : "+v"(s0), "+v"(s1), "+v"(c0), "+v"(c1));
            double src = s0 + s1;
            *Yh = src;  // (rows 0 / 1: the broadcast layout is the output layout)
            double bcn = hi ? 0.0 : c0 + c1;
            double b0 = rhs(2)[0], b1 = rhs(2)[12 * N];
#pragma unroll
            for (int j = 1; j <= MID + 1; ++j) {
              asm volatile("" : : : "memory");
              double gc[6];
#pragma unroll
              for (int i = 0; i < 6; ++i) gc[i] = g[i];
              const double bc = j <= MID ? bcn : 0.0;
              if (j < MID) {  // prefetch the next step's rows
                row6(rowp(j + 1));
              } else if (j == MID) {  // the meeting step: M^{-1} (slot 0) and b_m in the broadcast layout
                row6(GHr + RS * rr_ + h6);
                lds_cd* qb = (lds_cd*)&sh.u.it.bo[MID][ri];
                b0 = qb[0]; b1 = qb[12 * N];
              } else if constexpr (kLagOut<N>) {  // the last step: the first outward step's columns (12 terms)
#pragma unroll
                for (int i = 0; i < 12; ++i) go[i] = ObL[RS * i + GS * (MID - 1)];
              } else {  // the last step: the first outward step's columns
#pragma unroll
                for (int i = 0; i < 6; ++i) g[i] = Ob[RS * i + GS * (MID - 1)];
              }
              asm volatile("" : : : "memory");  // the prefetch is issued here, not sunk to its use
              double s_in = src;
              if (j == MID + 1) s_in = row_pair_sum(src) - (b0 + b1);
              const double y = pair_sum32(bdot6(gc, s_in, bc));
              // the next right-hand side is summed after the chain: its loads were issued at
              // the end of the previous step, and summing them ahead of the chain would put
              // their LDS latency on the critical path
              asm volatile("" : "+v"(b0), "+v"(b1));
              if (j < MID) bcn = hi ? 0.0 : b0 + b1;
              if (j + 2 <= MID) {
                b0 = rhs(j + 2)[0]; b1 = rhs(j + 2)[12 * N];
              }
              // row_ror:10 (lane q <- lane q + 6) on every lane, then a select: as a select on
              // the rotated value the compiler kept an exec-masked branch, and the register
              // copies in front of it waited for the right-hand-side loads just issued (an LDS
              // round trip per step)
              double yr = dppd<0x12A>(y);
              asm volatile("" : "+v"(yr));
              const double yb = hi ? yr : y;
              if (j <= MID) {
                // y of stage kk(j) (the meeting stage's y_m / v_m stay in registers); the
                // bottom chain keeps its v_m through the steps past BOT
                if (j < MID) *((cr == 0 || j < BOT) ? Yh + 12 * j : sink) = y;
                const bool adv = j <= BOT || cr == 0;
                src = adv ? yb : src;
              } else {
                // (kLagOut: the outward products are full rows on every row pair, so every
                // row takes x_m in its own layout; pair_sum32 left it bit-identical in rows
                // 0 / 2 and 1 / 3)
                xp = kLagOut<N> ? y : yb;
                if (cr == 0 && hi == 0 && s < 12) sh.u.it.xs[SIGX<N>(MID + 1)][rr_] = y;
              }
            }
            STAMP(6);
          }
          {
            // w_k = S_k^{-1} y_k for every stage but the meeting one, stage-parallel: lane
            // LN(ph) of stage k's row takes row ph of S_k^{-1} and y_k by row broadcast
            sync_all();
            using scd2 = std::conditional_t<BIG, const dbl2, lds_cd2>;
            const scd2* const q = (scd2*)(SmR + SLOT<N>(SIG<N>(k)) + RS * ph);
            double srow[12];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
              const dbl2 v = q[i];
              srow[2 * i] = v.x;
              srow[2 * i + 1] = v.y;
            }
            // (the meeting stage has no y / w: its lanes read stage 0's y, their product unused)
            double* const yk = &sh.u.it.yv[SIG<N>(k == MID ? 0 : k)][ph];
            const double wk = bdot_ln12(srow, *yk, 0.0);
            // in place: the row's reads of y_k precede (DPP operands); phantom rows keep out
            // (stage N-1's row may sit in another wave and read y after their store)
            if (cl && k != MID && !phantom) *yk = wk;
            sync_all();
          }
          if (t < 64) {
            // Outward step j: top kk = MID-j: X_kk = w_kk - G_{kk+1}' X_{kk+1}; bottom
            // kk = MID+j: X_kk = w_kk - H_{kk-1}' X_{kk-1}.  w of stage kk: top slot MID-j,
            // bottom slot N-j (Wb - 12 j); X_kk = xs[kk+1]: top slot MID+1-j, bottom slot
            // N-j (SIGX; Xb - 12 j).  Even N: the bottom chain has no step MID (its store
            // goes to the sink).  (bases at step MID's slot: step j at base + 12 (MID - j))
            lds_cd* const Wb = (lds_cd*)&sh.u.it.yv[0][0] + (12 * (cr == 0 ? 0 : N - MID) + rr_);
            lds_d* const sinkO = (lds_d*)&sh.red[0] + (t & 31);
            lds_d* const Xb = (hi == 0 && s < 12) ? (lds_d*)&sh.u.it.xs[0][0] + (12 * (cr == 0 ? 1 : N - MID) + rr_)
                                                  : sinkO;
            double bq = Wb[12 * (MID - 1)];
            if constexpr (kLagOut<N>) {
              // full 12-term column products on every row (rows 2 / 3 repeat rows 0 / 1): one
              // v_fmac chain per step, no swap-add, rotation or select (as ph_sweep_lag)
#pragma unroll
              for (int j = 1; j <= MID; ++j) {
                asm volatile("" : : : "memory");
                double gc[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) gc[i] = go[i];
                const double bc = bq;
                if (j < MID) {
#pragma unroll
                  for (int i = 0; i < 12; ++i) go[i] = ObL[RS * i + GS * (MID - j - 1)];
                  if (j + 1 <= BOT) bq = Wb[12 * (MID - j - 1)];
                  else bq = Wb[12 * (MID - (cr == 0 ? j + 1 : BOT))];
                }
                asm volatile("" : : : "memory");
                const double acc = bdot12(gc, xp, bc);  // x = w - G' x_next with -G stored
                if (j < MID) {
                  xp = acc;
                  Xb[12 * (MID - j)] = acc;
                } else if constexpr (N & 1) {
                  *Xb = acc;
                } else {
                  *(cr == 0 ? Xb : sinkO) = acc;
                }
              }
            } else {
#pragma unroll
            for (int j = 1; j <= MID; ++j) {
              asm volatile("" : : : "memory");
              double gc[6];
#pragma unroll
              for (int i = 0; i < 6; ++i) gc[i] = g[i];
              const double bc = hi ? 0.0 : bq;
              if (j < MID) {
#pragma unroll
                for (int i = 0; i < 6; ++i) g[i] = Ob[RS * i + GS * (MID - j - 1)];
                // (even N: the bottom chain has no step MID; it re-reads its last w)
                if (j + 1 <= BOT) bq = Wb[12 * (MID - j - 1)];
                else bq = Wb[12 * (MID - (cr == 0 ? j + 1 : BOT))];
              }
              asm volatile("" : : : "memory");
              const double x = pair_sum32(bdot6(gc, xp, bc));  // x = w - G' x_next with -G stored
              if (j < MID) {
                double xr = dppd<0x12A>(x);
                asm volatile("" : "+v"(xr));
                xp = hi ? xr : x;
                Xb[12 * (MID - j)] = x;
              } else if constexpr (N & 1) {
                *Xb = x;
              } else {  // even N: the bottom chain has no step MID
                *(cr == 0 ? Xb : sinkO) = x;
              }
            }
            }
            __builtin_amdgcn_s_setprio(0);
          }
          wave_sync();
          }  // MPCQ_REP_SWEEP
      };
      // the state sweep: the lagging form up to 32 stages, the split form beyond
      auto ph_sweep = [&]() __attribute__((always_inline)) {
        if constexpr (BIG) ph_sweep_split();
        else ph_sweep_lag();
      };
      // ri0: 1/rho of the own slot-0 row (the ADMM loop's, or polish's)
      auto ph_recover = [&](const RhsOps* op, double ri0, double uf, double beta, double& sf, double& sX,
                            double (&ax)[3]) __attribute__((always_inline)) {
          // P8: forces f_k = F_k (b_f - R B' g) = u - (F W) g, with g = Xd X_{k+1} + Hd X_k
          // on the velocity rows (the states' part of those rows)
          double gv;
          MPCQ_LANE_OFFS(kRecompLoop);
          // the iteration-invariant LDS operands of P8 / P9 are read before the
          // barrier that ends the sweeps (their latency hides behind it), the
          // sweep's states after it
          double fwl[6], qll[6];
#pragma unroll
          for (int i = 0; i < 3; ++i) {  // 16-B aligned pairs: ds_read_b128 (twice ds_read2_b64's LDS rate)
            using wcd2 = std::conditional_t<BIG, const dbl2, lds_cd2>;
            const dbl2 fa = ((lds_cd2*)(FWr + oFW))[i], qa = ((wcd2*)(QLr + oQLm))[i];
            fwl[2 * i] = fa.x; fwl[2 * i + 1] = fa.y;
            qll[2 * i] = qa.x; qll[2 * i + 1] = qa.y;
          }
          // (the same coefficients as ph_rhs's, from the held set when there is one)
          const double eXd = op ? op->cXd : Ab[oXd], eHd = op ? op->cHd : Ab[oHdm], eH6 = op ? op->cH6 : Ab[oH6m];
          const double cFb = Ab[oFb], cFa = Ab[oFa], cF4 = Ab[oF4];
          const double cSw = op ? op->cf[4] : Ab[oF + 4];
          sync_all();
          STAMP(7);
          const double xa = XSr[rXSpm];  // (stage 0: X_0 = 0, a zero slot)
          const double xb = XSr[rXSp6m];
          sX = XSr[rXS];
          asm volatile("" : : : "memory");
          {
            gv = eXd * sX + eHd * xa;  // used from the lanes of rows 6..11 only
            sf = uf - bdot_ln6v(fwl, gv, 0.0);
          }
          STAMP(9);
          // P9: z, y update (osqp update_z / update_y), x update.  A x~ on the own rows:
          // dynamics rows use B f = B u - B F W g = beta / rho - (R^{-1} Q) g (no force gather)
          {
            {
              // B f on the velocity rows (zero coefficients elsewhere)
              const double bfv = beta * ri0 - bdot_ln6v(qll, gv, 0.0);
              const double dyn = (gv + eH6 * xb) + bfv;
              // friction rows: lane c < 3 owns row c, lane 3 rows 3 and 4 (all loads unconditional)
              const double q2 = qbc<2>(sf);
              double q01;
              if constexpr (kColfFold) {  // ta0 ? q0 : q1 (ta0: quad lanes 0, 1) as one quad permute
                q01 = qperm<0, 0, 1, 1>(sf);
              } else {
                const double q0 = qbc<0>(sf), q1 = qbc<1>(sf);
                q01 = ta0 ? q0 : q1;
              }
              const double frA = cFb * q2 + cFa * q01;
              const double frB = cF4 * q2;
              const double swg = cSw * sf;
              ax[0] = cl ? dyn : frA;
              ax[1] = cl ? swg : frB;
              ax[2] = cl ? frA : 0.0;
            }
          }
      };
      const double kNoW[3] = {0.0, 0.0, 0.0};

      // ---- 9. residuals (OSQP update_info, uniform results), termination, infeasibility ---------
      double pri_res = 0.0, dua_res = 0.0, eps_pri = 0.0, eps_dua = 0.0, s_pri = 0.0, s_dua = 0.0;
      // OSQP 0.6's infeasibility tests (auxil.c is_primal_infeasible / is_dual_infeasible)
      // on the last iteration's delta_y (dy, own rows) and delta_x (dxf, dxX, own
      // columns), evaluated the way osqp evaluates them: the cheap conditions first
      // (||E dy||, u'dy+ + l'dy-, ||D dx||, ||D^-1 P dx||), the products A' dy / A dx
      // only where those hold.  infeas_cheap runs right after the update, while the
      // deltas are live: it publishes them (na / nb, free between the sweeps) with
      // update_info's states / duals under one barrier and leaves the per-wave partials
      // of the cheap quantities in red[32 wv + 16 ..]; update_info(INF) combines them
      // into uniform flags (each test only where its residual test fails, as osqp's
      // check_termination); infeas_products, only when a flag holds, adds the products
      // (two more barriers).  On MPC.py's QPs the dual side never reaches its product
      // and the primal side does at ~40 % of the checks (oracle counts, C2 batch), so
      // the product pass is skipped at most checks -- with identical outcomes.
      // outcome bits (one uniform int: the loop carries it): 1 primal, 2 dual infeasible
      // at the check's tolerances, 4 / 8 at the approximate (x10) ones
      int inf_bits = 0;
      int inf_need = 0;  // cheap-condition bits (same layout) awaiting the products
      // The bounds as the check sees them: lo_of / hi_of from the row scaling E and the
      // dynamics bound in the check's constant block (ck, read with the others in one
      // batch).  Formed from the loop's own E / bnd, the products (-inf E, -fz_max E) were
      // hoisted out of the ADMM loop and spilled, and each came back in the check as a
      // scratch reload waited for on its own.  Same expressions, same values.
      auto chk_bounds = [&](const double (&cv)[CK_COUNT], double (&lo)[3], double (&hi)[3])
          __attribute__((always_inline)) {
        if constexpr (FUSED) {
          const double e0 = cv[CK_E0], e1 = cv[CK_E1], e2 = cv[CK_E2], bd = cv[CK_BND];
          double fz = fz_max();
          asm volatile("" : "+v"(fz));
          lo[0] = cl ? bd : -kInf * e0;
          lo[1] = cl ? 0.0 : -fz * e1;
          lo[2] = cl ? -kInf * e2 : -kInf;
          hi[0] = cl ? bd : 0.0;
          hi[1] = 0.0;
          hi[2] = cl ? 0.0 : kInf;
        } else {
#pragma unroll
          for (int j = 0; j < 3; ++j) { lo[j] = lo_of(j); hi[j] = hi_of(j); }
        }
      };
      // the infeasibility tolerances, laundered for the same reason (10 eps, hoisted, was
      // spilled)
      auto chk_eps = [&](double& epi0, double& edi0) __attribute__((always_inline)) {
        epi0 = p.eps_prim_inf;
        edi0 = p.eps_dual_inf;
        asm volatile("" : "+v"(epi0), "+v"(edi0));
      };
      double dyp[3];     // delta_y projected onto the polar of the recession cone of [l, u]
      // The cheap part of OSQP's infeasibility tests on the last iteration's deltas, own
      // data only: dyp, and this wave's maxima ||E dy|| / ||D dx|| / ||D^-1 P dx|| and sum
      // u'dy+ + l'dy- into P[PS wv + 16 + {0, 2, 3, 6}] (red for the blocking check, dcp
      // for the deferred one).  cv: the constant block, read ahead of the check (ck_all).
      auto cheap_partials = [&](const double (&dy)[3], double dxf, double dxX, const double (&cv)[CK_COUNT],
                                double* const P, int PS) __attribute__((always_inline)) {
        MPCQ_CHECK_IDS();
        double lob[3], hib[3];
        chk_bounds(cv, lob, hib);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const bool uinf = hib[j] > kInf * kMinScaling, linf = lob[j] < -kInf * kMinScaling;
          dyp[j] = uinf ? (linf ? 0.0 : fmin(dy[j], 0.0)) : (linf ? fmax(dy[j], 0.0) : dy[j]);
        }
        double ndy = 0.0, ineq = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double lj = lob[j], hj = hib[j];
          ndy = fmax(ndy, fabs(cv[CK_E0 + j] * dyp[j]));
          ineq += hj * fmax(dyp[j], 0.0) + lj * fmin(dyp[j], 0.0);
        }
        if (phantom) ineq = 0.0;  // a sum: stage N-1 counts once
        double q3[2] = {0.0, 0.0};
        {
          const double df = cv[CK_DF], dx = cv[CK_DX], dif = 1.0 / df, diX = 1.0 / dx;
          const double pbf = cv[CK_PBF], pbx = cv[CK_PBX];
          if (cl) {
            q3[0] = fmax(fabs(df * dxf), fabs(dx * dxX));                // ||D dx||
            q3[1] = fmax(fabs(pbf * dxf * dif), fabs(pbx * dxX * diX));  // ||D^-1 P dx||
          }
        }
        // maxima over the wave (lanes 0 / 4 / 8 keep ||E dy|| / ||D dx|| / ||D^-1 P dx||,
        // published in slots 0 / 2 / 3), the sum by xor butterflies
        const double mine = pair_max(row_pair_max(tred3(ndy, q3[0], q3[1], s)));
        ineq += dppd<0xB1>(ineq);
        ineq += dppd<0x4E>(ineq);
        ineq += dppd<0x124>(ineq);
        ineq += dppd<0x128>(ineq);
        ineq = row_pair_sum(ineq);
        {
          const long long bb = __double_as_longlong(ineq);
          const auto lo_ = __builtin_amdgcn_permlane32_swap((unsigned)bb, (unsigned)bb, false, false);
          const auto hi_ = __builtin_amdgcn_permlane32_swap((unsigned)(bb >> 32), (unsigned)(bb >> 32), false, false);
          ineq = __longlong_as_double(((long long)hi_[0] << 32) | lo_[0]) +
                 __longlong_as_double(((long long)hi_[1] << 32) | lo_[1]);
        }
        if (lane == 0 || lane == 4 || lane == 8) P[PS * wv + 16 + (lane == 0 ? 0 : 2 + (lane >> 3))] = mine;
        if (lane == 6) P[PS * wv + 16 + 6] = ineq;
      };
      auto infeas_cheap = [&](const double (&dy)[3], double dxf, double dxX, const double (&cv)[CK_COUNT])
          __attribute__((always_inline)) {
        cheap_partials(dy, dxf, dxX, cv, sh.red, 32);
        // published together with update_info's states / duals, one barrier for both
        if (cl) {
          sh.u.it.na[k][ph] = dxX;
          sh.u.it.nb[k][ph] = dyp[0];
          sh.u.it.yv[k][ph] = xX;
          sh.u.it.bo[k][ph] = y[0];
        }
        sync_all();  // (update_info(INF) relies on this barrier for its own publication)
      };
      // the products, where a cheap condition holds (inf_need != 0, uniform): A' dy for
      // the primal test, A dx for the dual one, on the deltas infeas_cheap published
      auto infeas_products = [&](double dxf, double dxX, const double (&cv)[CK_COUNT])
          __attribute__((always_inline)) {
        MPCQ_CHECK_IDS();
        launder_p();
        double vu = -INFINITY, vl = -INFINITY;
        {
          double adx[3], lob[3], hib[3];
          rowA(dxf, dxX, (lds_cd*)&sh.u.it.na[0][0], adx);
          chk_bounds(cv, lob, hib);
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const double lj = lob[j], hj = hib[j], v = adx[j] / cv[CK_E0 + j];
            if (hj < kInf * kMinScaling) vu = fmax(vu, v);
            if (lj > -kInf * kMinScaling) vl = fmax(vl, -v);
          }
        }
        double naty = 0.0;
        {
          double dtf, dtX;
          colAt(dyp, &sh.u.it.nb[0][0], dtf, dtX);
          const double dif = 1.0 / cv[CK_DF], diX = 1.0 / cv[CK_DX];
          if (cl) naty = fmax(fabs(dtf * dif), fabs(dtX * diX));  // ||D^-1 A' dy||
        }
        // lanes 0 / 4 / 8 keep ||D^-1 A' dy|| / vu / vl, published in slots 1 / 4 / 5
        const double mine = pair_max(row_pair_max(tred3(naty, vu, vl, s)));
        if (lane == 0 || lane == 4 || lane == 8) sh.red[32 * wv + 16 + (lane == 0 ? 1 : 4 + (lane >> 3))] = mine;
        sync_all();
        const int e = s < 6 ? s : 0;  // slots 16..21 are all maxima (0 / 2 / 3 from infeas_cheap)
        double v = sh.red[16 + e];
#pragma unroll
        for (int w = 1; w < NW; ++w) v = fmax_hw(v, sh.red[32 * w + 16 + e]);
        const double ndy = rbc<0>(v), ndx = rbc<2>(v);  // (the cheap maxima, kept in slots 0 / 2)
        const double naty_ = rbc<1>(v), vu_ = rbc<4>(v), vl_ = rbc<5>(v);
        double epi0, edi0;
        chk_eps(epi0, edi0);
        int bits = 0;
#pragma unroll
        for (int fi = 0; fi < 2; ++fi) {
          const double f = fi == 0 ? 1.0 : 10.0, epi = f * epi0, edi = f * edi0;
          const bool pi = ((inf_need >> (2 * fi)) & 1) && naty_ < epi * ndy;
          const bool di = ((inf_need >> (2 * fi)) & 2) && !(vu_ > edi * ndx) && !(vl_ > edi * ndx);
          bits |= (pi ? 1 : 0) << (2 * fi);
          bits |= (di ? 2 : 0) << (2 * fi);
        }
        inf_bits = __builtin_amdgcn_readfirstlane(bits);
        sync_all();
      };
      // The states and dynamics-row duals are published in yv / bo, which the sweeps
      // no longer need (xs still feeds the force recovery of slower waves); lane s
      // of each row then owns residual quantity s, reduced over the wave's rows by
      // permlane swaps and over the waves through red[].  INF: also combine the
      // cheap partials of infeas_cheap into inf_need.
      // info_terms: this wave's 16 residual maxima into D[DS wv + 0..15], from the own
      // rows / columns and the published states XP (X_{k'} of stage k' at 12 (k' - 1))
      // and duals WD (y of stage k' at 12 k')
      auto info_terms = [&](const double (&cv)[CK_COUNT], lds_cd* const XP, const double* WD, double* const D,
                            int DS) __attribute__((always_inline)) {
        MPCQ_CHECK_IDS();
        const double ei3[3] = {1.0 / cv[CK_E0], 1.0 / cv[CK_E1], 1.0 / cv[CK_E2]};
        const double dif = 1.0 / cv[CK_DF], diX = 1.0 / cv[CK_DX], pbf = cv[CK_PBF], pbx = cv[CK_PBX];
        double mine, pmine;  // this lane's row maxima (tred6: primal quantity 3 b3 + (b2 ? 2 : b1))
        {  // primal side: A x - z on the own rows
          double ax[3], q6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
          rowA(xf, xX, XP, ax);
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const double ei = ei3[j], d = ax[j] - z[j];
            q6[0] = fmax(q6[0], fabs(ei * d));
            q6[1] = fmax(q6[1], fabs(ei * ax[j]));
            q6[2] = fmax(q6[2], fabs(ei * z[j]));
            q6[3] = fmax(q6[3], fabs(d));
            q6[4] = fmax(q6[4], fabs(ax[j]));
            q6[5] = fmax(q6[5], fabs(z[j]));
          }
          pmine = tred6(q6, s);
        }
        STAMP(5);
        {  // dual side: P x + A' y on the own columns
          double q6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
          double atf, atX;
          colAt(y, WD, atf, atX);
          const double pxf = pbf * xf, pxX = pbx * xX;
          const double df_ = pxf + atf, dX_ = pxX + atX;
          if (cl) {
            q6[0] = fmax(fabs(dif * df_), fabs(diX * dX_));
            q6[1] = fmax(fabs(dif * pxf), fabs(diX * pxX));
            q6[2] = fmax(fabs(dif * atf), fabs(diX * atX));
            q6[3] = fmax(fabs(df_), fabs(dX_));
            q6[4] = fmax(fabs(pxf), fabs(pxX));
            q6[5] = fmax(fabs(atf), fabs(atX));
          }
          // the last step of the butterfly joins the sides: primal quantity e on lane
          // 2 e (e < 3) / 2 e + 2 (e >= 3), the dual's on the lane after it
          mine = tstep(kXor1{}, pmine, tred6(q6, s), s & 1);
        }
        mine = pair_max(row_pair_max(mine));  // the wave's four rows
        if (lane < 16) D[DS * wv + lane] = mine;
      };
      // info_combine: the residuals and tolerances (uniform) from every wave's partials in
      // D (stride DS); INF: the cheap infeasibility partials (slots 16..) into inf_need
      auto info_combine = [&](auto inf_tag, const double (&cv)[CK_COUNT], const double* const D, int DS)
          __attribute__((always_inline)) {
        constexpr bool INF = decltype(inf_tag)::value;
        MPCQ_CHECK_IDS();
        const double csc = cv[CK_C], cinv = 1.0 / csc;
        double qv[12];
        {
          double v = D[s];
#pragma unroll
          for (int w = 1; w < NW; ++w) v = fmax_hw(v, D[DS * w + s]);
          qv[0] = rbc<0>(v); qv[1] = rbc<2>(v); qv[2] = rbc<4>(v);
          qv[3] = rbc<8>(v); qv[4] = rbc<10>(v); qv[5] = rbc<12>(v);
          qv[6] = rbc<1>(v); qv[7] = rbc<3>(v); qv[8] = rbc<5>(v);
          qv[9] = rbc<9>(v); qv[10] = rbc<11>(v); qv[11] = rbc<13>(v);
        }
        pri_res = qv[0];
        dua_res = cinv * qv[6];
        eps_pri = p.eps_abs + p.eps_rel * fmax(qv[1], qv[2]);
        eps_dua = p.eps_abs + p.eps_rel * cinv * fmax(qv[7], qv[8]);
        s_pri = qv[3] / (fmax(qv[4], qv[5]) + kDivTol);
        s_dua = qv[9] / (fmax(qv[10], qv[11]) + kDivTol);
        // uniform by construction; readfirstlane lets the compiler see it
        pri_res = uni(pri_res); dua_res = uni(dua_res); eps_pri = uni(eps_pri);
        eps_dua = uni(eps_dua); s_pri = uni(s_pri); s_dua = uni(s_dua);

        if constexpr (INF) {
          // the cheap conditions of infeas_cheap: slots 0 ||E dy||, 2 ||D dx||, 3 ||D^-1 P dx||, 6 u'dy+ + l'dy-
          const int e = s == 2 || s == 3 || s == 6 ? s : 0;
          // (every wave's partial read first, up to 32 stages in one batch: the select between the
          // sum and the maximum is a branch, and each read sat inside it behind its own wait)
          double tv[NW];
#pragma unroll
          for (int w = 0; w < NW; ++w) tv[w] = D[DS * w + 16 + e];
          if constexpr (!BIG) hold_all(tv);
          double v = tv[0];
#pragma unroll
          for (int w = 1; w < NW; ++w) v = s == 6 ? v + tv[w] : fmax_hw(v, tv[w]);
          // kept in VGPRs (every lane holds the same values) and folded into one uniform
          // int at the end: SGPRs here would push loop-carried scalars into VGPR lanes
          // (v_readlane on the hot path, measured)
          const double ndy = rbc<0>(v), ndx = rbc<2>(v), npdx = rbc<3>(v), ineq = rbc<6>(v);
          double epi0, edi0;
          chk_eps(epi0, edi0);
          int need = 0;
#pragma unroll
          for (int fi = 0; fi < 2; ++fi) {
            const double f = fi == 0 ? 1.0 : 10.0, epi = f * epi0, edi = f * edi0;
            const bool pi = !(pri_res < f * eps_pri) && ndy > kDivTol && ineq < epi * ndy;
            const bool di = !(dua_res < f * eps_dua) && ndx > kDivTol && 0.0 < csc * edi * ndx &&
                            npdx < csc * edi * ndx;
            need |= (pi ? 1 : 0) << (2 * fi);
            need |= (di ? 2 : 0) << (2 * fi);
          }
          inf_need = __builtin_amdgcn_readfirstlane(need);
          inf_bits = 0;
        }
      };
      // INF: after infeas_cheap, which has published the states / duals with its deltas
      auto update_info = [&](auto inf_tag, const double (&cv)[CK_COUNT]) __attribute__((always_inline)) {
        constexpr bool INF = decltype(inf_tag)::value;
        if constexpr (!INF) {
          if (cl) { sh.u.it.yv[k][ph] = xX; sh.u.it.bo[k][ph] = y[0]; }
          sync_all();
        }
        STAMP(4);
        launder_p();
        info_terms(cv, (lds_cd*)&sh.u.it.yv[0][0], &sh.u.it.bo[0][0], sh.red, 32);
        sync_all();
        STAMP(8);
        info_combine(inf_tag, cv, sh.red, 32);
        sync_all();
      };
      auto converged = [&](double fac) __attribute__((always_inline)) {
        return pri_res < fac * eps_pri && dua_res < fac * eps_dua;
      };

      // ---- 10. the ADMM loop --------------------------------------------------------------------
      // The factorisation sits outside the hot loop: the outer loop factors,
      // the inner loop iterates until convergence, max_iter or a rho update.
      bool last_checked = false;
      int iter = 1;
      if constexpr (kXstLds<N>) MPCQ_SET_XST(0);
      int to_check = p.check_termination, to_adapt = p.adaptive_rho_interval;
      // a resumed slice continues the saved loop counters; slice_iters > 0 suspends at the
      // first segment end slice_iters iterations on (mpcq_set_slice)
      if (kSlice<N> && a.resume) {
        iter = __builtin_amdgcn_readfirstlane(a.res_i[8 * b]);
        to_check = __builtin_amdgcn_readfirstlane(a.res_i[8 * b + 1]);
        to_adapt = __builtin_amdgcn_readfirstlane(a.res_i[8 * b + 2]);
      }
      const int slice_end =
          kSlice<N> && a.slice_iters > 0 && a.slice_iters < p.max_iter ? iter + a.slice_iters : 0x7fffffff;
      bool suspended = false;
      // the bounds are re-derived where used (lo_of / hi_of: a select on the lane's
      // class and its row scaling in the fused path) rather than held in 6 registers
      for (;;) {
        bool fac_ok = true;
#ifdef MPCQ_FACTIME
        const uint64_t ft0_ = __builtin_amdgcn_s_memtime();
#endif
#pragma nounroll
        for (int rep_ = 0; rep_ < MPCQ_REP_FACTOR; ++rep_) fac_ok = factor(p.sigma, nullptr);  // > 1: timing only
#ifdef MPCQ_FACTIME
        fac_cycles += __builtin_amdgcn_s_memtime() - ft0_;
#endif
        if (!fac_ok) { MPCQ_SET_XST(MPCQ_STATUS_FACTOR_FAILED); break; }
        STAMP(2);
        bool refactor = false;
        // One ADMM iteration (osqp update_xz_tilde / update_x / update_z / update_y).
        // DELTA: also keep delta_y / delta_x (the last iteration before a check, for the
        // infeasibility tests).  The iterations between two checks run in a loop of
        // their own without them, so the check / infeasibility code and its live values
        // sit outside the hot loop's register allocation (inside it, they cost 0.31 us
        // per iteration through spills on the sweep path, measured).
        // MODE 0: a plain iteration; 1 (DELTA): the checked one, also keeping delta_y / delta_x
        auto admm_iter = [&](auto mode_tag, const RhsOps& ops, double (&dyv)[3], double& dxf_, double& dxX_,
                             double (&cvp)[CK_COUNT])
            __attribute__((always_inline)) {
          constexpr int MODE = decltype(mode_tag)::value;
          constexpr bool DELTA = MODE == 1;
          double uf, beta, sf, sX, ax[3];
          // (beyond 32 stages the operands are read per iteration: held, they cost the
          // register budget of the 9..16-wave workgroups -- N = 48: scratch 840 -> 712 B
          // per lane, 17.68 -> 16.75 us per iteration, profiles/r03c_iterbench.txt)
          ph_rhs(true, kBig<N> ? nullptr : &ops, kNoW, 0.0, 0.0, uf, beta);
          ph_sweep();
          // DELTA (the last iteration before a check): the check's constant block is read
          // here, its memory latency behind the force recovery and the z / y / x update
          if constexpr (DELTA) ck_all(cvp);
          double zl[3], zh[3], zrr[3], zri[3];  // the update's per-row constants
          if constexpr (kZcMem<N>) {
            ph_recover(nullptr, zc_ptr()[ZC_RI], uf, beta, sf, sX, ax);
            pdbl* const q = zc_ptr();
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              zl[j] = q[ZC_LO + j]; zh[j] = q[ZC_HI + j]; zrr[j] = q[ZC_RR + j]; zri[j] = q[ZC_RI + j];
            }
          } else {
            ph_recover(kBig<N> ? nullptr : &ops, ri[0], uf, beta, sf, sX, ax);
#pragma unroll
            for (int j = 0; j < 3; ++j) { zl[j] = lo_of(j); zh[j] = hi_of(j); zrr[j] = rr[j]; zri[j] = ri[j]; }
          }
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const double zr = p.alpha * ax[j] + (1.0 - p.alpha) * z[j];
            const double tt = zr + zri[j] * y[j];
            const double zn = clamp_hw(tt, zl[j], zh[j]);  // osqp project: c_min(c_max(tt, l), u)
            const double d = zrr[j] * (zr - zn);
            if constexpr (DELTA) dyv[j] = d;
            y[j] = y[j] + d;
            z[j] = zn;
          }
          const double nxf = p.alpha * sf + (1.0 - p.alpha) * xf;
          const double nxX = p.alpha * sX + (1.0 - p.alpha) * xX;
          if constexpr (DELTA) { dxf_ = nxf - xf; dxX_ = nxX - xX; }
          xf = nxf;
          xX = nxX;
          STAMP(10);
        };
        const bool chk_on = p.check_termination > 0;
        const bool adp_on = p.adaptive_rho && p.adaptive_rho_interval > 0;
        while (iter <= p.max_iter) {
          // the next event: a termination check, an adaptive-rho step or the last iteration
          int until = p.max_iter - iter + 1;
          if (chk_on && to_check < until) until = to_check;
          if (adp_on && to_adapt < until) until = to_adapt;
          double dyv[3], dxf_, dxX_;
          // held in registers through the iterations up to the next check: no LDS traffic
          // for them in the loop
          RhsOps ops;
          // The offsets the loop's phases take from O0 are derived again here from laundered
          // coordinates: held across the check, five of them were spilled, and each came back
          // here as a scratch reload waited for on its own, one round trip after another in
          // front of the first iteration.
          if constexpr (!kBig<N>) {
            launder();
            O0 = offs();
            load_rhs_ops(ops);
          }
          double cvp[CK_COUNT];
#pragma nounroll
          for (int r_ = 1; r_ < until; ++r_, ++iter)
            admm_iter(std::integral_constant<int, 0>{}, ops, dyv, dxf_, dxX_, cvp);
          admm_iter(std::integral_constant<int, 1>{}, ops, dyv, dxf_, dxX_, cvp);
          // iter % check_termination == 0 / iter % adaptive_rho_interval == 0, by countdown
          const bool can_check = chk_on && (to_check -= until) == 0;
          if (can_check) to_check = p.check_termination;
          const bool adapt = adp_on && (to_adapt -= until) == 0;
          if (adapt) to_adapt = p.adaptive_rho_interval;
          last_checked = can_check;
          // the last iteration's information is always formed here, while its deltas are
          // live (osqp's update_info after the loop when the last iteration was unchecked)
          infeas_cheap(dyv, dxf_, dxX_, cvp);
          update_info(std::true_type{}, cvp);
          if (inf_need) infeas_products(dxf_, dxX_, cvp);
          if (!(isfinite(pri_res) && isfinite(dua_res))) { MPCQ_SET_XST(MPCQ_STATUS_NONFINITE); break; }
          if (can_check) {  // osqp check_termination
            if (converged(1.0)) { MPCQ_SET_XST(MPCQ_STATUS_SOLVED); break; }
            if (inf_bits & 1) { MPCQ_SET_XST(MPCQ_STATUS_PRIMAL_INFEASIBLE); break; }
            if (inf_bits & 2) { MPCQ_SET_XST(MPCQ_STATUS_DUAL_INFEASIBLE); break; }
          }
          if (adapt) {
            double rn = rho_s * sqrt(s_pri / (s_dua + kDivTol));
            rn = fmin(fmax(rn, kRhoMin), kRhoMax);
            if (rn > rho_s * p.adaptive_rho_tolerance || rn < rho_s / p.adaptive_rho_tolerance) {
              rho_s = rn;
              set_rho();
              zc_store();
              refactor = true;
              ++n_upd;
              ++iter;
              sync_all();
              break;
            }
          }
          STAMP(11);
          ++iter;
          // (a sliced launch) the residuals over their tolerances at the last segment end up to
          // half way through the slice, for the suspended instance's key (below)
          if (kSlice<N> && a.slice_iters > 0 && iter <= slice_end - (a.slice_iters >> 1) && t == 0) {
            a.res_key[2 * b] = pri_res / eps_pri;
            a.res_key[2 * b + 1] = dua_res / eps_dua;
            a.res_i[8 * b + 4] = iter;
          }
          if (kSlice<N> && iter >= slice_end && iter <= p.max_iter) {  // (uniform) suspend this slice here
            suspended = true;
            break;
          }
        }
        if (!refactor) break;
      }
      if (kSlice<N> && suspended) {  // the iterate and the loop's counters for the next slice; no other output
        constexpr int64_t RL = res_lanes(N);
        double* const q = a.res + b * 8 * RL + t;
        q[0] = xf;
        q[RL] = xX;
#pragma unroll
        for (int j = 0; j < 3; ++j) { q[(2 + j) * RL] = z[j]; q[(5 + j) * RL] = y[j]; }
        if (t == 0) {
          a.res_rho[b] = rho_s;
          // the key: the iterations left, extrapolated from the residuals' geometric decay between
          // the half-way sample and now, primal and dual, the larger (a residual not decaying, or
          // no half-way sample: as long as can be); 0 for one already within its tolerance
          const int i1 = a.res_i[8 * b + 4];
          const double rp = pri_res / eps_pri, rd = dua_res / eps_dua;
          auto left = [&](double r1, double r2) __attribute__((always_inline)) -> double {
            if (!(r2 > 1.0)) return 0.0;
            if (i1 <= 0 || !(r1 > r2)) return 1e30;
            return log(r2) / log(r1 / r2) * (double)(iter - i1);
          };
          a.res_key[2 * b] = fmax(left(a.res_key[2 * b], rp), left(a.res_key[2 * b + 1], rd));
          a.res_i[8 * b] = iter;
          a.res_i[8 * b + 1] = to_check;
          a.res_i[8 * b + 2] = to_adapt;
          a.res_i[8 * b + 3] = n_upd;
          if (a.status) a.status[b] = kStatusSuspended;
        }
        return;
      }
      if constexpr (kXstLds<N>) {
        sync_all();  // thread 0's exit status
        status = sh.flag[4];
      }
      if constexpr (kXstRe<N>) {  // the exit's reason, as the loop tested it (kXstRe)
        if (sh.flag[2] != 0) status = MPCQ_STATUS_FACTOR_FAILED;
        else if (iter <= p.max_iter) {
          if (!(isfinite(pri_res) && isfinite(dua_res))) status = MPCQ_STATUS_NONFINITE;
          else if (converged(1.0)) status = MPCQ_STATUS_SOLVED;
          else if (inf_bits & 1) status = MPCQ_STATUS_PRIMAL_INFEASIBLE;
          else if (inf_bits & 2) status = MPCQ_STATUS_DUAL_INFEASIBLE;
        }
      }
      it_done = iter > p.max_iter ? p.max_iter : iter;
      if (status == 0) {
        if (!last_checked) {  // the information of the last (unchecked) iteration
          if (converged(1.0)) status = MPCQ_STATUS_SOLVED;
          else if (inf_bits & 1) status = MPCQ_STATUS_PRIMAL_INFEASIBLE;
          else if (inf_bits & 2) status = MPCQ_STATUS_DUAL_INFEASIBLE;
        }
        if (status == 0)  // the approximate check (tolerances x10)
          status = converged(10.0) ? MPCQ_STATUS_SOLVED_INACCURATE
                   : (inf_bits & 4) ? MPCQ_STATUS_PRIMAL_INFEASIBLE_INACCURATE
                   : (inf_bits & 8) ? MPCQ_STATUS_DUAL_INFEASIBLE_INACCURATE
                                   : MPCQ_STATUS_MAX_ITER_REACHED;
      }

      admm_st = status;
      // ---- 11. polish ---------------------------------------------------------------------------
      // OSQP 0.6 polish (polish.c): guess the active set from (z, y), solve the
      // equality-constrained QP  min 1/2 x'Px  s.t. A_act x = b_act,  project
      // (A x, y) onto the normal cone and keep the point if it lowers the
      // residuals; polish_rounds > 1 repeats the guess from the polished point
      // until the set repeats (primal-dual active set).  The equality QP is solved
      // by the method of multipliers on the engine's own factorisation
      // (K = P + sigma I + rho_p A_act' A_act, rho_p = kPolishRho):
      //   x+ = K^{-1} (sigma x + A_act' (rho_p b - y)),  y+ = y + rho_p (A_act x+ - b),
      // 1 + max(polish_refine_iter, kPolishMinIter) solves.  OSQP's own reduced KKT
      // (rho = 1/delta = 1e6) is not used: the engine's stage elimination forms
      // F = K_ff^{-1} explicitly, and at 1e6 its Schur complements lose positive
      // definiteness (measured: negative pivots on every instance).  Equality rows
      // stay in the set even when y is exactly 0.
      if constexpr (POLISH) {
        if (p.polish != 0 && (status == MPCQ_STATUS_SOLVED ||
                              (p.polish >= 2 && (status == MPCQ_STATUS_SOLVED_INACCURATE ||
                                                 status == MPCQ_STATUS_MAX_ITER_REACHED)))) {
          constexpr double kPolishRho = 1e3;
          // the refinement contracts by the error of the explicit stage inverses, which
          // grows with the chain length: 10 steps land within 2e-10 of x* up to N = 32,
          // N = 48 needs 20 (measured: 10 -> 2-4e-7, 20 -> 1e-10, tools/attic/polish48b.py),
          // N = 64 more than 20 (20 -> 3.2e-8 on the fixtures, r03b)
          constexpr int kPolishMinIter = N > 48 ? 30 : (N > 32 ? 20 : 10);
          const double a_pri = pri_res, a_dua = dua_res;
          const double axf = xf, axX = xX;
          double az[3], ay[3], zs[3], ys[3], bred[3], prho[3];
          int act[3], prv[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) { az[j] = z[j]; ay[j] = y[j]; zs[j] = z[j]; ys[j] = y[j]; prv[j] = 0; }
          bool have = false;
          double b_pri = 0.0, b_dua = 0.0, b_epri = 0.0, b_edua = 0.0, bxf = 0.0, bxX = 0.0, bz[3], by[3];
          const int rounds = p.polish_rounds > 0 ? p.polish_rounds : 1;
          const int mom = p.polish_refine_iter > kPolishMinIter ? p.polish_refine_iter : kPolishMinIter;
          for (int rd = 0; rd < rounds; ++rd) {
            int changed = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              const int r = nat_row(j);
              const bool eq = ((cls >> (2 * j)) & 3u) == RC_EQ;
              int a_ = 0;
              if (r >= 0) {
                if (rd == 0) {  // OSQP's guess (polish.c form_Ared)
                  if (zs[j] - lo_of(j) < -ys[j]) a_ = -1;
                  else if (hi_of(j) - zs[j] < ys[j]) a_ = 1;
                  if (eq && a_ == 0) a_ = 1;
                } else {  // keep correctly signed active rows, add violated rows
                  const double tol = 1e-12;
                  if (prv[j] == -1 && (ys[j] <= tol || eq)) a_ = -1;
                  else if (prv[j] == 1 && (ys[j] >= -tol || eq)) a_ = 1;
                  else if (zs[j] < lo_of(j) - tol) a_ = -1;
                  else if (zs[j] > hi_of(j) + tol) a_ = 1;
                }
              }
              changed |= a_ != prv[j];
              act[j] = a_;
              prv[j] = a_;
              bred[j] = a_ < 0 ? lo_of(j) : (a_ > 0 ? hi_of(j) : 0.0);
              prho[j] = a_ ? kPolishRho : 0.0;
            }
            if (rd > 0) {  // stop when the set repeats (uniform over the block)
              if (t == 0) sh.flag[3] = 0;
              sync_all();
              if (changed) atomicOr(&sh.flag[3], 1);
              sync_all();
              const bool same = sh.flag[3] == 0;
              sync_all();
              if (same) break;
            }
            ++pol_rounds;
            if (!factor(p.sigma, prho)) break;
#pragma unroll
            for (int j = 0; j < 3; ++j) { rr[j] = prho[j]; ri[j] = act[j] ? 1.0 / kPolishRho : 0.0; }
            // one proximal multiplier step from the ADMM point (x, y on the active rows),
            // then refinement against the true residuals of the equality QP
            //   r_x = -(P x + A_act' y),  r_y = b - A_act x,
            //   dx = K^{-1} (r_x + rho_p A_act' r_y),  dy = rho_p (A_act dx - r_y),
            // so that the error of the explicit stage inverses does not reach the fixed point
            double xpf, xpX, axp[3], yp[3];
            {
              double pw[3], uf, beta, ax[3];
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                yp[j] = act[j] ? y[j] : 0.0;
                pw[j] = act[j] ? kPolishRho * bred[j] - yp[j] : 0.0;
              }
              ph_rhs(false, nullptr, pw, p.sigma * xf, p.sigma * xX, uf, beta);
              ph_sweep();
              ph_recover(nullptr, ri[0], uf, beta, xpf, xpX, ax);
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                axp[j] = ax[j];
                if (act[j]) yp[j] += kPolishRho * (ax[j] - bred[j]);
              }
            }
            for (int it_ = 0; it_ < mom; ++it_) {
              double pw[3], ry[3], uf, beta, dxf, dxX, ax[3];
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                ry[j] = act[j] ? bred[j] - axp[j] : 0.0;
                pw[j] = act[j] ? kPolishRho * ry[j] - yp[j] : 0.0;
              }
              ph_rhs(false, nullptr, pw, -Pbf() * xpf, -PbX() * xpX, uf, beta);
              ph_sweep();
              ph_recover(nullptr, ri[0], uf, beta, dxf, dxX, ax);
              xpf += dxf;
              xpX += dxX;
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                axp[j] += ax[j];
                if (act[j]) yp[j] += kPolishRho * (ax[j] - ry[j]);
              }
#ifdef MPCQ_DEBUG_POLISH
              {
                double rmax = 0.0, dxm = fmax(fabs(dxf), fabs(dxX));
                for (int j = 0; j < 3; ++j) if (act[j]) rmax = fmax(rmax, fabs(axp[j] - bred[j]));
                for (int o = 32; o > 0; o >>= 1) { rmax = fmax(rmax, __shfl_xor(rmax, o)); dxm = fmax(dxm, __shfl_xor(dxm, o)); }
                if (b == 0 && lane == 0) printf("blk0 wave %d rd %d it %d max|Ax-b| %.3e max|dx| %.3e\n", wv, rd, it_, rmax, dxm);
              }
#endif
            }
            // the next round guesses from the unprojected point
#pragma unroll
            for (int j = 0; j < 3; ++j) { zs[j] = axp[j]; ys[j] = yp[j]; }
            // project onto the normal cone (polish.c project_normalcone), residuals
            xf = xpf;
            xX = xpX;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              const double tt = axp[j] + yp[j];
              const double zz = fmin(fmax(tt, lo_of(j)), hi_of(j));
              z[j] = zz;
              y[j] = tt - zz;
            }
#ifdef MPCQ_DEBUG_POLISH
            if (b == 0)
              for (int j = 0; j < 3; ++j)
                if (fabs(y[j] - yp[j]) > 1e-9 || (act[j] == 0 && fabs(axp[j] - z[j]) > 1e-12))
                  printf("blk0 k %d s %d j %d row %d act %d bred %.3e ax %.6e yp %.3e -> z %.6e y %.3e lo %.3e hi %.3e\n",
                         k, s, j, nat_row(j), act[j], bred[j], axp[j], yp[j], z[j], y[j], lo_of(j), hi_of(j));
#endif
            {
              double cvq[CK_COUNT];
              ck_all(cvq);
              update_info(std::false_type{}, cvq);
            }
#ifdef MPCQ_DEBUG_POLISH
            if (b < 2 && t == 0) printf("blk %d rd %d admm pri %.3e dua %.3e | polished pri %.3e dua %.3e eps %.3e %.3e\n", (int)b, rd, a_pri, a_dua, pri_res, dua_res, eps_pri, eps_dua);
#endif
            if (!have || fmax(pri_res, dua_res) < fmax(b_pri, b_dua)) {
              have = true;
              b_pri = pri_res; b_dua = dua_res; b_epri = eps_pri; b_edua = eps_dua;
              bxf = xf; bxX = xX;
#pragma unroll
              for (int j = 0; j < 3; ++j) { bz[j] = z[j]; by[j] = y[j]; }
            }
          }
          const bool good = have && ((b_pri < a_pri && b_dua < a_dua) || (b_pri < a_pri && a_dua < 1e-10) ||
                                     (b_dua < a_dua && a_pri < 1e-10));
          if (good) {
            xf = bxf;
            xX = bxX;
#pragma unroll
            for (int j = 0; j < 3; ++j) { z[j] = bz[j]; y[j] = by[j]; }
            pol_st = 1;
            if (status != MPCQ_STATUS_SOLVED && b_pri < b_epri && b_dua < b_edua) status = MPCQ_STATUS_SOLVED;
          } else {
            xf = axf;
            xX = axX;
#pragma unroll
            for (int j = 0; j < 3; ++j) { z[j] = az[j]; y[j] = ay[j]; }
            pol_st = have ? -1 : 0;
          }
        }
      }
    }
    // ---- 12. outputs ----------------------------------------------------------------------------
    // osqp store_solution: no solution (x = y = NaN) for the infeasibility statuses
    const bool nan_out = status == MPCQ_STATUS_NONFINITE || status == MPCQ_STATUS_FACTOR_FAILED ||
                         status == MPCQ_STATUS_BAD_GAIT || status == MPCQ_STATUS_BAD_BOUNDS ||
                         status == MPCQ_STATUS_PRIMAL_INFEASIBLE ||
                         status == MPCQ_STATUS_DUAL_INFEASIBLE || status == MPCQ_STATUS_PRIMAL_INFEASIBLE_INACCURATE ||
                         status == MPCQ_STATUS_DUAL_INFEASIBLE_INACCURATE;
    if (cl) {
      const double vf = nan_out ? NAN : Df * xf, vX = nan_out ? NAN : DX * xX;
      if (a.x) { a.x[b * n + colF] = vf; a.x[b * n + colX] = vX; }
      if (a.f0 && k == 0) a.f0[b * 12 + ph] = vf;
    }
    if (a.y) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int r = nat_row(j);
        // dual_warm = 1: the scaled workspace y, what the next tick's warm start reads
        if (r >= 0) a.y[b * m + r] = nan_out ? NAN : (p.dual_warm ? y[j] : E[j] * y[j] / cscale);
      }
    }
#ifdef MPCQ_STAMPS
    STAMP(12);
    if (t == kStampT && a.stamps) {
      for (int i = 0; i < 16; ++i) a.stamps[b * 16 + i] = st_acc[i];
    }
#endif
    if (t == 0) {
      if (a.status) a.status[b] = status;
      if (a.iters) a.iters[b] = it_done;
      if (a.rho_out) a.rho_out[b] = rho_s;
      if (a.info) {
        a.info[4 * b + 0] = n_upd;
        a.info[4 * b + 1] = pol_st;
#ifdef MPCQ_FACTIME
        a.info[4 * b + 2] = (int)(fac_cycles >> 8);  // factorisation cycles / 256 (timing build)
#else
        a.info[4 * b + 2] = pol_rounds;
#endif
        a.info[4 * b + 3] = admm_st != 0 ? admm_st : status;  // the ADMM's exit status before polish
      }
    }
  }
}

#undef MPCQ_LANE_OFFS
#undef MPCQ_CHECK_IDS
#undef MPCQ_SET_XST

template <int N>
hipError_t launch_t(bool fused, bool solve, const mpcq_params& p, const LaunchArgs& a,
                    hipStream_t s) {
  const dim3 grid((unsigned)a.batch), block(16 * kRows<N>);
  if (kBig<N> && solve && !a.work) return hipErrorInvalidValue;  // the caller sizes it with work_doubles(N)
  // polish lives in its own instantiation: the production kernel's code (and its
  // register allocation in the ADMM loop) does not carry it
  const bool pol = p.polish != 0;
  const bool rob = a.robots != nullptr && (fused || !solve);
  // the solving ROB kernels read both tables (mpcq_api.cpp launch_tables passes both or neither)
  if (rob && solve && !a.weights) return hipErrorInvalidValue;
  if (rob && !a.disturb) return hipErrorInvalidValue;
  if (!rob && (a.weights || a.disturb)) return hipErrorInvalidValue;
  if (rob && !solve) hipLaunchKernelGGL((engine_kernel<N, true, false, false, true>), grid, block, 0, s, p, a);
  else if (rob && pol) hipLaunchKernelGGL((engine_kernel<N, true, true, true, true>), grid, block, 0, s, p, a);
  else if (rob) hipLaunchKernelGGL((engine_kernel<N, true, true, false, true>), grid, block, 0, s, p, a);
  else if (!solve) hipLaunchKernelGGL((engine_kernel<N, true, false, false>), grid, block, 0, s, p, a);
  else if (fused && pol) hipLaunchKernelGGL((engine_kernel<N, true, true, true>), grid, block, 0, s, p, a);
  else if (fused) hipLaunchKernelGGL((engine_kernel<N, true, true, false>), grid, block, 0, s, p, a);
  else if (pol) hipLaunchKernelGGL((engine_kernel<N, false, true, true>), grid, block, 0, s, p, a);
  else hipLaunchKernelGGL((engine_kernel<N, false, true, false>), grid, block, 0, s, p, a);
  return hipGetLastError();
}

}  // namespace

// One translation unit per horizon (the Makefile compiles this file once per
// N with -DMPCQ_ENGINE_N=N, in parallel); mpcq_dispatch.cpp picks the unit.
#ifndef MPCQ_ENGINE_N
#error "compile mpcq_engine.hip with -DMPCQ_ENGINE_N=<horizon> (see the Makefile)"
#endif
// (here, where both headers are seen; the unit's other layout checks end mpcq_engine_layout.h, and
// tests/host/engine_layout_check.cpp runs them all for every horizon at once)
static_assert(!kBig<MPCQ_ENGINE_N> || Work<MPCQ_ENGINE_N>::SIZE == work_doubles(MPCQ_ENGINE_N),
              "work_doubles(N) (mpcq_internal.h) and Work<N> disagree");

#define MPCQ_CAT_(a, b) a##b
#define MPCQ_CAT(a, b) MPCQ_CAT_(a, b)
hipError_t MPCQ_CAT(engine_launch_n, MPCQ_ENGINE_N)(bool fused, bool solve, const mpcq_params& p,
                                                   const LaunchArgs& a, hipStream_t s) {
  return launch_t<MPCQ_ENGINE_N>(fused, solve, p, a, s);
}

}  // namespace mpcq
