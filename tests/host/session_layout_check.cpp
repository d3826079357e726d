// session_layout_check.cpp — the session layout unit (csrc/mpcq_session_layout.cpp) driven from
// standard input, one command per line, one answer per line; no HIP, no GPU.
// tests/test_session_layout_host.py compiles both with the address and undefined-behaviour
// sanitizers and compares the answers with tests/snapshot_model.py.
//
//   L N B k_mpc parts delay latency n_gaits have_order resets
//       -> "H <header, hex> A <part>:<array>:<bytes> ..."      (parts: bit gi = part gi exists)
//   P N bytes <header, hex>
//       -> "OK B k_mpc parts delay latency n_gaits have_order resets" or "NO <the refusal's text>"
//   D <shape a: B k_mpc parts delay latency n_gaits> <shape b: the same> batch_too
//       -> "SAME" or "DIFF <text>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mpcq_session_layout.h"

using namespace mpcq;

static void set_parts(SnapShape* sh, unsigned parts) {
  for (int gi = 0; gi < G_COUNT; ++gi) sh->has[gi] = parts >> gi & 1u;
}

static unsigned parts_of(const SnapShape& sh) {
  unsigned parts = 0;
  for (int gi = 0; gi < G_COUNT; ++gi) parts |= sh.has[gi] ? 1u << gi : 0u;
  return parts;
}

int main() {
  char* line = nullptr;
  size_t cap = 0;
  while (getline(&line, &cap, stdin) > 0) {
    if (line[0] == 'L') {
      SnapShape sh;
      long long B;
      int N, have_order, resets;
      unsigned parts;
      if (sscanf(line + 1, "%d %lld %d %u %d %d %d %d %d", &N, &B, &sh.k_mpc, &parts, &sh.delay, &sh.latency,
                 &sh.n_gaits, &have_order, &resets) != 9)
        return 2;
      sh.B = B;
      set_parts(&sh, parts);
      BlobHeader h;
      blob_header(sh, N, have_order, resets, &h);
      printf("H ");
      for (size_t i = 0; i < header_bytes(h.version); ++i) printf("%02x", ((const unsigned char*)&h)[i]);
      printf(" A");
      size_t nb[G_COUNT][kPartArrays];
      snap_sizes(sh, N, nb);
      for (int gi = 0; gi < G_COUNT; ++gi)
        for (int w = 0; w < kPartArrays; ++w)
          if (nb[gi][w]) printf(" %d:%d:%zu", gi, w, nb[gi][w]);
      printf("\n");
    } else if (line[0] == 'P') {
      int N, at = 0;
      long long bytes;
      if (sscanf(line + 1, "%d %lld %n", &N, &bytes, &at) != 2) return 2;
      const char* hex = line + 1 + at;
      std::vector<unsigned char> buf;  // exactly the header's bytes: a read behind them is the sanitizer's
      for (; hex[0] && hex[1] && hex[0] != '\n'; hex += 2) {
        unsigned v;
        if (sscanf(hex, "%2x", &v) != 1) return 2;
        buf.push_back((unsigned char)v);
      }
      SnapShape sh;
      bool have_order = false, resets = false;
      char msg[256];
      if (parse_blob_header(buf.data(), bytes, N, &sh, &have_order, &resets, msg, sizeof(msg)))
        printf("OK %lld %d %u %d %d %d %d %d\n", (long long)sh.B, sh.k_mpc, parts_of(sh), sh.delay, sh.latency,
               sh.n_gaits, (int)have_order, (int)resets);
      else
        printf("NO %s\n", msg);
    } else if (line[0] == 'D') {
      SnapShape s[2];
      long long B[2];
      unsigned parts[2];
      int batch_too;
      if (sscanf(line + 1, "%lld %d %u %d %d %d %lld %d %u %d %d %d %d", &B[0], &s[0].k_mpc, &parts[0], &s[0].delay,
                 &s[0].latency, &s[0].n_gaits, &B[1], &s[1].k_mpc, &parts[1], &s[1].delay, &s[1].latency,
                 &s[1].n_gaits, &batch_too) != 13)
        return 2;
      for (int i = 0; i < 2; ++i) {
        s[i].B = B[i];
        set_parts(&s[i], parts[i]);
      }
      const char* diff = shape_difference(s[0], s[1], batch_too != 0);
      if (diff) printf("DIFF %s\n", diff);
      else printf("SAME\n");
    } else {
      return 2;
    }
  }
  free(line);
  return 0;
}
