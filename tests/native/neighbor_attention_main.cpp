// neighbor_attention_main.cpp -- csrc/neighbor_attention.h on the host, compiled alone (no HIP header, no GPU): for every D
// with 1 .. 70 heads (the shapes of tests/test_neighbor_attention_gpu.py among them) and the cap on C, na_plan holds every
// channel of every head on exactly one lane of one chunk, no head straddles a group or a wave, and the staged tile stays
// within the LDS budget.  Prints "no violation" when everything holds; VIOLATION and exit status 1 otherwise.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../pytorch3d_pointops_amd/csrc/neighbor_attention.h"

using namespace pointops;

static int violations = 0;
#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) printf("VIOLATION: "), printf(__VA_ARGS__), printf("\n"), ++violations; \
  } while (0)

static void check(int64_t heads, int64_t D, int64_t K) {
  const NaPlan p = na_plan(heads, D, K);
  const long long H = heads, d = D, k = K;
  CHECK(na_head_ok(D) && p.Gh * kNaVec == D, "D = %lld: Gh = %d", d, p.Gh);
  CHECK(p.G <= kNaMaxGroup && (p.G & (p.G - 1)) == 0 && p.Hg * p.Gh == p.G && p.rows * p.G == kNaBlock &&
            (p.G >= heads * p.Gh || p.G == kNaMaxGroup) && (int64_t)(p.chunks - 1) * p.Hg < heads,
        "(%lld, %lld): G = %d, Hg = %d, rows = %d, chunks = %d", H, d, p.G, p.Hg, p.rows, p.chunks);
  std::vector<int> seen((size_t)(heads * D), 0);
  for (int c = 0; c < p.chunks; ++c) {
    for (int lane = 0; lane < kNaBlock; ++lane) {  // lane of the workgroup: its group is lane / G, its wave lane / 64
      const int j = lane % p.G, jl = j % p.Gh, first = lane - jl, last = first + p.Gh - 1;  // first .. last: the head's lanes
      const int64_t h = (int64_t)c * p.Hg + j / p.Gh;
      CHECK(first / p.G == last / p.G && first / 64 == last / 64, "(%lld, %lld): the head of lane %d straddles", H, d, lane);
      if (h >= heads || lane >= p.G) continue;  // (count the first group only)
      for (int x = 0; x < kNaVec; ++x) ++seen[(size_t)(h * D + jl * kNaVec + x)];
    }
  }
  for (int64_t ch = 0; ch < heads * D; ++ch)
    CHECK(seen[(size_t)ch] == 1, "(%lld, %lld): channel %lld is held %d times", H, d, (long long)ch, seen[(size_t)ch]);
  CHECK(p.tile >= 1 && (K < 1 || p.tile <= K) && (K > 16 || K < 1 || p.tile == K) &&
            na_lds_bytes(p) == (size_t)p.rows * p.tile * (1 + p.Hg) * 4 && na_lds_bytes(p) <= 32768,
        "(%lld, %lld), K = %lld: tile = %d, %zu bytes of LDS", H, d, k, p.tile, na_lds_bytes(p));
}

int main() {
  long plans = 0;
  for (int64_t K : {0, 1, 3, 16, 20, 255, 1024, 100000}) {
    for (int64_t D = kNaVec; D <= kNaMaxD; D *= 2) {
      for (int64_t heads = 1; heads <= 70; ++heads) check(heads, D, K), ++plans;
      check(kNaMaxC / D, D, K), ++plans;  // the cap on C
    }
  }
  CHECK(!na_head_ok(0) && !na_head_ok(2) && !na_head_ok(12) && !na_head_ok(512), "na_head_ok takes a bad head size");
  const NaPlan a = na_plan(1, 4, 20), b = na_plan(3, 4, 20), c = na_plan(8, 32, 16), d = na_plan(3, 128, 20);
  CHECK(a.G == 1 && a.rows == 256 && a.tile == 16, "the plan of (1, 4), K = 20: two tiles");
  CHECK(b.G == 4 && b.Hg == 4 && b.chunks == 1 && b.tile == 20, "the plan of (3, 4), K = 20");
  CHECK(c.G == 64 && c.Gh == 8 && c.Hg == 8 && c.chunks == 1 && c.rows == 4, "the plan of (8, 32)");
  CHECK(d.G == 64 && d.Gh == 32 && d.Hg == 2 && d.chunks == 2, "the plan of (3, 128): a tail head");
  printf("%ld plans checked\n", plans);
  if (violations) return 1;
  printf("no violation\n");
  return 0;
}
