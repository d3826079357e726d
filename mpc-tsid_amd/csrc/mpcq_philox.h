// mpcq_philox.h — the counter-based generator the scenario and channel kernels share
// (mpcq_scenario.hip, mpcq_channel.hip): Philox4x32-10 and the draws derived from its words.
// Integer arithmetic for the generator, every derived double exact or a single rounding, so the
// host restatements (mpcq/scenario.py, mpcq/channel.py) agree bit for bit; include/mpcq.h has
// the rules.  Include it under `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpcq {

struct W4 {
  uint32_t w0, w1, w2, w3;
};

__device__ inline W4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return W4{c0, c1, c2, c3};
}

// 53 bits of two words as a double in [0, 1): both products and the sum are exact
__device__ inline double u01(uint32_t wa, uint32_t wb) {
  return ((double)(wa >> 5) * 67108864.0 + (double)(wb >> 6)) * 0x1p-53;
}

__device__ inline double range(double lo, double hi, double u) { return lo + (hi - lo) * u; }

}  // namespace mpcq
