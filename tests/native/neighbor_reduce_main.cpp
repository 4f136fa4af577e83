// neighbor_reduce_main.cpp -- csrc/neighbor_reduce.h on the host, compiled alone (no HIP header, no kernel, no GPU): for
// every C in 1 .. 2048 and a range of K, nr_plan deals every channel to exactly one lane (V, G, rows, chunks), the staged
// tile stays within its budget and is a single one where a chunked row would re-read it, and nr_lds_bytes matches.
// Prints "no violation" when everything holds; a line with VIOLATION and exit status 1 otherwise.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../pytorch3d_pointops_amd/csrc/neighbor_reduce.h"

using namespace pointops;

static int violations = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      printf("VIOLATION: ");        \
      printf(__VA_ARGS__);          \
      printf("\n");                 \
      ++violations;                 \
    }                               \
  } while (0)

int main() {
  const int64_t Ks[] = {0, 1, 3, 16, 20, 64, 255, 256, 1024, 1025, 100000};
  long plans = 0;
  for (int64_t C = 1; C <= 2048; ++C) {
    for (int64_t K : Ks) {
      const NrPlan p = nr_plan(C, K);
      ++plans;
      CHECK(p.V == (C % 4 == 0 ? 4 : 1), "C = %lld: V = %d", (long long)C, p.V);
      const int64_t units = (C + p.V - 1) / p.V;
      CHECK(p.G >= 1 && p.G <= kNrMaxGroup && (p.G & (p.G - 1)) == 0, "C = %lld: G = %d", (long long)C, p.G);
      CHECK(p.G >= units || p.G == kNrMaxGroup, "C = %lld: G = %d does not cover %lld units", (long long)C, p.G,
            (long long)units);
      CHECK(p.G == 1 || p.G / 2 < units, "C = %lld: G = %d is not the smallest width", (long long)C, p.G);
      CHECK(p.rows * p.G == kNrBlock, "C = %lld: rows = %d, G = %d", (long long)C, p.rows, p.G);
      CHECK(p.chunks >= 1 && (p.chunks == 1 || p.G == kNrMaxGroup), "C = %lld: %d chunks at G = %d", (long long)C,
            p.chunks, p.G);
      std::vector<int> seen((size_t)C, 0);
      for (int c = 0; c < p.chunks; ++c) {
        int filled = 0;
        for (int j = 0; j < p.G; ++j) {
          const int64_t ch = ((int64_t)c * p.G + j) * p.V;
          if (ch >= C) continue;
          ++filled;
          CHECK(ch + p.V <= C, "C = %lld: a lane of V = %d starts at %lld", (long long)C, p.V, (long long)ch);
          for (int q = 0; q < p.V && ch + q < C; ++q) ++seen[(size_t)(ch + q)];
        }
        CHECK(filled > 0, "C = %lld: chunk %d of %d is empty", (long long)C, c, p.chunks);
      }
      for (int64_t ch = 0; ch < C; ++ch) CHECK(seen[(size_t)ch] == 1, "C = %lld: channel %lld is held %d times", (long long)C, (long long)ch, seen[(size_t)ch]);
      CHECK(p.tile >= 1 && (K < 1 || p.tile <= K), "C = %lld, K = %lld: tile = %d", (long long)C, (long long)K, p.tile);
      CHECK((int64_t)p.rows * p.tile <= kNrTileEntries, "C = %lld, K = %lld: %d rows of %d slots", (long long)C,
            (long long)K, p.rows, p.tile);
      CHECK(p.chunks == 1 || K > 1024 || p.tile >= K, "C = %lld, K = %lld: %d chunks re-read a table of %d-slot tiles",
            (long long)C, (long long)K, p.chunks, p.tile);
      CHECK(nr_lds_bytes(p, false) == (size_t)p.rows * p.tile * 4 && nr_lds_bytes(p, true) == 2 * nr_lds_bytes(p, false) &&
                nr_lds_bytes(p, true) <= 32768,
            "C = %lld, K = %lld: %zu bytes of LDS", (long long)C, (long long)K, nr_lds_bytes(p, true));
    }
  }
  const NrPlan a = nr_plan(64, 16), b = nr_plan(260, 20), c = nr_plan(7, 3), d = nr_plan(3, 3);
  CHECK(a.V == 4 && a.G == 16 && a.rows == 16 && a.chunks == 1 && a.tile == 16, "the plan of C = 64, K = 16");
  CHECK(b.V == 4 && b.G == 64 && b.rows == 4 && b.chunks == 2 && b.tile == 20, "the plan of C = 260, K = 20");
  CHECK(c.V == 1 && c.G == 8 && c.chunks == 1 && d.V == 1 && d.G == 4, "the plans of C = 7 and C = 3");
  printf("%ld plans checked\n", plans);
  if (violations) return 1;
  printf("no violation\n");
  return 0;
}
