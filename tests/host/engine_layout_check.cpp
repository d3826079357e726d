// engine_layout_check.cpp — the engine's layout (csrc/mpcq_engine_layout.h) instantiated for
// every compiled horizon on the CPU; no GPU.  tests/test_engine_layout_host.py compiles it with
// the address and undefined-behaviour sanitizers and reads its output:
//
//   "C N <24 N column starts>"   XO / FO of every state and force column, in column order
//   "OK N"                       every invariant below holds at N
//   "FAIL N: <what>"             one line per broken invariant (exit status 1)
//
// An engine unit checks its own horizon alone (the static_asserts of its build); here the same
// conditions, and the ones no build checks (slots, permutations, prologue aliases, workspace
// regions), run for all 61.
#include <stddef.h>
#include <stdio.h>

#include <vector>

#include "mpcq_internal.h"
#include "mpcq_engine_layout.h"

using namespace mpcq;

static int failures = 0;

#define CHECK(N, cond, ...)                \
  do {                                     \
    if (!(cond)) {                         \
      printf("FAIL %d: ", N);              \
      printf(__VA_ARGS__);                 \
      printf(" (%s)\n", #cond);            \
      ++bad;                               \
    }                                      \
  } while (0)

// f maps 0..count-1 one-to-one onto itself
template <typename F>
static bool permutes(F f, int count) {
  std::vector<int> seen(count, 0);
  for (int i = 0; i < count; ++i) {
    const int v = f(i);
    if (v < 0 || v >= count || seen[v]++) return false;
  }
  return true;
}

template <int N>
static void check() {
  int bad = 0;
  using W = Work<N>;
  using S = Smem<N>;
  constexpr long KB = 1024;
  constexpr int fr_rows = N > 48 ? 12 * 16 * kRows<N> : 0;  // 12 entries of every lane's F_k row

  // the workspace: its size is the host's, and each region ends before the next begins
  if (N > 32) CHECK(N, W::SIZE == work_doubles(N), "Work::SIZE %d, work_doubles %lld", W::SIZE, (long long)work_doubles(N));
  else CHECK(N, work_doubles(N) == 0, "a workspace up to 32 stages");
  CHECK(N, 0 < W::SM, "SM %d", W::SM);
  CHECK(N, W::SM + SLOT<N>(N - 1) + GS <= W::FW, "S^-1 slots end at %d, FW at %d", W::SM + SLOT<N>(N - 1) + GS, W::FW);
  CHECK(N, W::FW + 72 * N <= W::QL, "FW ends at %d, QL at %d", W::FW + 72 * N, W::QL);
  CHECK(N, W::QL + 36 * N <= W::ZERO, "QL ends at %d, ZERO at %d", W::QL + 36 * N, W::ZERO);
  CHECK(N, W::ZERO + 72 <= W::AB, "ZERO ends at %d, AB at %d", W::ZERO + 72, W::AB);
  CHECK(N, W::AB + (kAbG<N> ? 126 * N - 18 : 0) <= W::FR, "AB ends before FR %d", W::FR);
  CHECK(N, W::FR + fr_rows <= W::SIZE, "FR ends at %d, SIZE %d", W::FR + fr_rows, W::SIZE);
  CHECK(N, W::SM < W::FW && W::FW < W::QL && W::QL < W::ZERO && W::ZERO < W::AB && W::AB <= W::FR && W::FR <= W::SIZE,
        "region order");
  // (the masked reads take ZERO as an offset from QL; the b128 reads need both 16-byte aligned)
  CHECK(N, W::SM % 2 == 0 && W::QL % 2 == 0 && W::ZERO % 2 == 0 && W::AB % 2 == 0 && W::FR % 2 == 0 && W::SIZE % 2 == 0,
        "16-byte alignment of the workspace regions");

  // LDS: one instance per CU, two up to 16 rows; what is read as b128 sits at 16 bytes
  CHECK(N, (long)sizeof(S) <= 160 * KB, "sizeof(Smem) %zu", sizeof(S));
  CHECK(N, kRows<N> > 16 || (long)sizeof(S) <= 80 * KB, "sizeof(Smem) %zu, two per CU", sizeof(S));
  CHECK(N, kRows<N> >= N && kRows<N> < N + 4 && kRows<N> % 4 == 0 && kRows<N> <= 64, "kRows %d", kRows<N>);
  CHECK(N, alignof(S) >= 16, "alignof(Smem) %zu", alignof(S));
  CHECK(N, offsetof(S, GH) % 16 == 0, "GH at %zu", offsetof(S, GH));
  CHECK(N, offsetof(S, Sm) % 16 == 0, "Sm at %zu", offsetof(S, Sm));
  CHECK(N, offsetof(S, FWb) % 16 == 0, "FWb at %zu", offsetof(S, FWb));
  CHECK(N, offsetof(S, FWs) % 16 == 0, "FWs at %zu", offsetof(S, FWs));
  CHECK(N, offsetof(S, zero) % 16 == 0, "zero at %zu", offsetof(S, zero));
  CHECK(N, offsetof(S, u.fa.St) % 16 == 0, "u.fa.St at %zu", offsetof(S, u.fa.St));
  CHECK(N, offsetof(S, u.fa.Sb) % 16 == 0, "u.fa.Sb at %zu", offsetof(S, u.fa.Sb));

  // the step order of the sweeps: every stage (SIG) and every state vector (SIGX) has its own slot
  CHECK(N, permutes([](int k) { return SIG<N>(k); }, N), "SIG is not a permutation of 0..N-1");
  CHECK(N, permutes([](int q) { return SIGX<N>(q); }, N + 1), "SIGX is not a permutation of 0..N");

  // the slots of GH (and of Sm, up to 32 stages): GS doubles each, disjoint, inside the array and its pad
  static_assert(offsetof(S, GHpad) == offsetof(S, GH) + sizeof(S::GH), "GHpad follows GH");
  static_assert(offsetof(S, Smpad) == offsetof(S, Sm) + sizeof(S::Sm), "Smpad follows Sm");
  const int gh_end = (int)((sizeof(S::GH) + sizeof(S::GHpad)) / sizeof(double));
  const int sm_end = (int)((sizeof(S::Sm) + sizeof(S::Smpad)) / sizeof(double));
  for (int q = 0; q < N; ++q) {
    const int at = SLOT<N>(q);
    CHECK(N, at >= 0 && at % 2 == 0, "slot %d at %d", q, at);
    CHECK(N, at + GS <= gh_end, "slot %d ends at %d, GH and its pad at %d", q, at + GS, gh_end);
    if (!kBig<N>) CHECK(N, at + GS <= sm_end, "slot %d ends at %d, Sm and its pad at %d", q, at + GS, sm_end);
    for (int r = 0; r < q; ++r)
      CHECK(N, SLOT<N>(r) + GS <= at || at + GS <= SLOT<N>(r), "slots %d and %d overlap", r, q);
  }

  // the prologue's aliases inside GH: xref, fsteps, then N + 80 ints (phase of stage, contact[20][4])
  using P = Prologue<N>;
  CHECK(N, P::XR == 0 && P::XR + 12 * (N + 1) <= P::FS, "xref ends at %d, fsteps at %d", P::XR + 12 * (N + 1), P::FS);
  CHECK(N, P::FS + 260 <= P::INTS, "fsteps ends at %d, the ints at %d", P::FS + 260, P::INTS);
  CHECK(N, sizeof(double) * P::INTS + sizeof(int) * (N + 80) <= sizeof(S::GH), "the ints end at byte %zu, GH at %zu",
        sizeof(double) * P::INTS + sizeof(int) * (N + 80), sizeof(S::GH));

  // the column starts, for the test to hold against the CSC pattern
  printf("C %d", N);
  for (int k = 0; k < N; ++k)
    for (int i = 0; i < 12; ++i) printf(" %d", XO<N>(k, i));
  for (int k = 0; k < N; ++k)
    for (int f = 0; f < 4; ++f)
      for (int c = 0; c < 3; ++c) printf(" %d", FO<N>(k, f, c));
  printf("\n");
  if (!bad) printf("OK %d\n", N);
  failures += bad;
}

#define MPCQ_CHECK_N(n) check<n>();

int main() {
  MPCQ_HORIZONS(MPCQ_CHECK_N)
  return failures ? 1 : 0;
}
