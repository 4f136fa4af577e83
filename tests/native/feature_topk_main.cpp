// feature_topk_main.cpp -- csrc/feature_topk.h on the host, compiled alone with feature_screen.h (no HIP header, no
// kernel, no GPU).  For S in {1, 4} and K in {1, 16, 17, 32}, on a few thousand rows of random, tied and spread
// distances whose screen values obey |s - r| <= E:
//   lists      every target goes to list topk_list_of(j, S); a list keeps the M smallest (s, j)
//   merge      topk_merge over the 2 S sorted key lists equals the K smallest (r, j) of the collected targets
//   r_K        is the K-th of them, +inf when fewer were collected
//   certified  every certified row's merged keys equal the brute-force K smallest (r, j) over ALL targets
// Prints "no violation" when everything holds; a line with VIOLATION and exit status 1 otherwise.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <utility>
#include <vector>

#include "../../pytorch3d_pointops_amd/csrc/feature_topk.h"

using namespace pointops;

static int violations = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      if (violations < 20) {        \
        printf("VIOLATION: ");      \
        printf(__VA_ARGS__);        \
        printf("\n");               \
      }                             \
      ++violations;                 \
    }                               \
  } while (0)

static const char* kModes[] = {"random", "tied", "spread"};

template <int S>
static void check_row(std::mt19937& rng, int mode, int K, long* rows, long* certified) {
  constexpr int LISTS = 2 * S;
  const int D = 33;
  const int len2 = std::uniform_int_distribution<int>(1, 400)(rng);
  const float E = mode == 0 ? 1e-3f : ldexpf(1.0f, -20);
  std::uniform_real_distribution<float> u(0.0f, 4.0f), noise(-E, E);
  std::uniform_int_distribution<int> tied(0, 7), spread(0, 100000);
  std::vector<float> r((size_t)len2), s((size_t)len2);
  for (int j = 0; j < len2; ++j) {
    r[j] = mode == 0 ? u(rng) : (float)(mode == 1 ? tied(rng) : spread(rng));
    s[j] = mode == 0 ? r[j] + noise(rng) : r[j];
    if (fabs((double)s[j] - (double)r[j]) > (double)E) s[j] = r[j];
  }
  // the lists: the M smallest (s, j) of every list, then the exact keys of the kept targets, sorted
  uint64_t keys[LISTS][kTopkM];
  float s_cut = INFINITY;
  std::vector<uint64_t> collected;
  for (int t = 0; t < LISTS; ++t) {
    std::vector<std::pair<float, int>> mine;
    for (int j = 0; j < len2; ++j)
      if (topk_list_of(j, S) == t) mine.push_back({s[j], j});
    std::sort(mine.begin(), mine.end());
    if ((int)mine.size() >= kTopkM) s_cut = fminf(s_cut, mine[kTopkM - 1].first);
    for (int k = 0; k < kTopkM; ++k)
      keys[t][k] = k < (int)mine.size() ? topk_key(r[mine[k].second], mine[k].second) : kTopkEmpty;
    std::sort(keys[t], keys[t] + kTopkM);
    for (int k = 0; k < kTopkM && k < (int)mine.size(); ++k) collected.push_back(keys[t][k]);
  }
  std::sort(collected.begin(), collected.end());
  std::vector<uint64_t> merged((size_t)K, 0);
  const float rK = topk_merge<LISTS>(
      K, [&](int t, int k) { return keys[t][k]; }, [&](int k, uint64_t v) { merged[(size_t)k] = v; });
  for (int k = 0; k < K; ++k) {
    const uint64_t want = k < (int)collected.size() ? collected[(size_t)k] : kTopkEmpty;
    CHECK(merged[k] == want, "S %d K %d %s: merged key %d is %016llx, want %016llx", S, K, kModes[mode], k,
          (unsigned long long)merged[k], (unsigned long long)want);
  }
  const float want_rK = K <= (int)collected.size() ? topk_key_dist(collected[(size_t)K - 1]) : INFINITY;
  CHECK(rK == want_rK, "S %d K %d %s: r_K %a, want %a", S, K, kModes[mode], rK, want_rK);
  ++*rows;
  if (!topk_certified(D, 1.0f, 1.0f, len2, rK, E, s_cut)) return;
  ++*certified;
  std::vector<uint64_t> all;
  for (int j = 0; j < len2; ++j) all.push_back(topk_key(r[j], j));
  std::sort(all.begin(), all.end());
  for (int k = 0; k < K && k < len2; ++k)
    CHECK(merged[k] == all[(size_t)k], "S %d K %d %s, %d targets: certified, but key %d is %016llx, brute force %016llx", S,
          K, kModes[mode], len2, k, (unsigned long long)merged[k], (unsigned long long)all[(size_t)k]);
}

static void check_predicate() {
  const int D = 33;
  CHECK(topk_list_of(0, 1) == 0 && topk_list_of(4, 1) == 1 && topk_list_of(36, 1) == 1 && topk_list_of(40, 1) == 0,
        "t(j), S = 1");
  CHECK(topk_list_of(3, 4) == 0 && topk_list_of(37, 4) == 3 && topk_list_of(64, 4) == 4 && topk_list_of(127, 4) == 7 &&
            topk_list_of(128, 4) == 0,
        "t(j), S = 4");
  CHECK(topk_key(INFINITY, INT32_MAX) == kTopkEmpty && topk_key_dist(kTopkEmpty) == INFINITY, "the empty key");
  CHECK(topk_key(1.0f, 7) < topk_key(1.0f, 8) && topk_key(1.0f, 8) < topk_key(2.0f, 0), "(r, j) order of the keys");
  CHECK(topk_certified(D, 1.0f, 1.0f, kTopkM, INFINITY, 1.0f, 0.0f), "M targets are collected whole");
  CHECK(!topk_certified(D, 1.0f, 1.0f, kTopkM + 1, 5.0f, 1.0f, 0.0f), "M + 1 targets need the comparison");
  CHECK(!topk_certified(D, 1.0f, 1.0f, 100, 1.0f, 0.0f, 1.0f), "r_K + E == s_cut is not certified");
  CHECK(topk_certified(D, 1.0f, 1.0f, 100, 1.0f, 0.0f, nextafterf(1.0f, 2.0f)), "one ulp of room is");
  CHECK(!topk_certified(D, 1.0f, 1.0f, 100, INFINITY, 0.5f, INFINITY), "fewer than K collected");
  CHECK(!topk_certified(D, NAN, 1.0f, 3, 0.0f, 0.0f, INFINITY), "NaN n1, even with three targets");
  CHECK(!topk_certified(D, 1.0f, INFINITY, 3, 0.0f, 0.0f, INFINITY), "infinite n2max");
  CHECK(!topk_certified(D, kScreenMaxNorm, kScreenMaxNorm, 100, 0.0f, 0.0f, INFINITY), "n1 + n2max above 2^126");
}

int main() {
  check_predicate();
  std::mt19937 rng(20250712);
  long rows = 0, certified = 0;
  const int ks[] = {1, 16, 17, 32};
  for (int K : ks)
    for (int mode = 0; mode < 3; ++mode)
      for (int i = 0; i < 250; ++i) {
        check_row<1>(rng, mode, K, &rows, &certified);
        check_row<4>(rng, mode, K, &rows, &certified);
      }
  printf("%ld rows, %ld certified\n", rows, certified);
  CHECK(rows >= 6000 && certified >= rows / 4 && certified < rows, "the rows do not exercise both outcomes: %ld of %ld",
        certified, rows);
  if (violations) {
    printf("%d VIOLATION(s)\n", violations);
    return 1;
  }
  printf("no violation\n");
  return 0;
}
