// knn_in_radius_list_main.cpp -- csrc/knn_radius_list.h on the host, compiled alone (no HIP header, no kernel, no GPU).
//
//   keys     radius_list_key packs (d2, j) so that the order of the keys is the (d2, j) order, for +0, subnormals, the
//            largest finite value and +inf, with j at 0 and at 2^32 - 1; the round trip gives d2 and j back bit for bit;
//            every key is below kRadiusListEmpty
//   lists    RadiusList<KC>::insert over streams of candidates against std::sort over (d2, j): KC at every bucket of
//            the kernel (1, 4, 8, 16, 32, 64) and one past the edges that a template can have (2, 5, 9, 17, 33), streams
//            shorter than, equal to and longer than KC (the empty stream too), with duplicated candidates' distances
//            (many exact ties, resolved by j), all-equal distances, +0, subnormals and +inf among them, in random,
//            ascending and descending order of arrival; worst() is the KC-th key or kRadiusListEmpty
// Prints "no violation" when everything holds; a line with VIOLATION and exit status 1 otherwise.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <utility>
#include <vector>

#include "../../pytorch3d_pointops_amd/csrc/knn_radius_list.h"

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

static uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, sizeof(b));
  return b;
}
static float float_of(uint32_t b) {
  float f;
  memcpy(&f, &b, sizeof(f));
  return f;
}

static void check_keys() {
  const float ds[] = {0.0f, float_of(1u), float_of(2u), float_of(0x007fffffu), float_of(0x00800000u), 1.0f,
                      float_of(0x3f800001u), 3.4028234663852886e38f, INFINITY};
  const uint32_t js[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  std::vector<std::pair<std::pair<float, uint32_t>, uint64_t>> all;
  for (float d : ds)
    for (uint32_t j : js) {
      const uint64_t key = radius_list_key(d, j);
      CHECK(bits_of(radius_list_d2(key)) == bits_of(d) && radius_list_index(key) == j, "round trip of (%a, %u)", d, j);
      CHECK(key < kRadiusListEmpty, "the key of (%a, %u) is not below the empty key", d, j);
      all.push_back({{d, j}, key});
    }
  for (const auto& a : all)
    for (const auto& b : all)
      CHECK((a.first < b.first) == (a.second < b.second), "order of (%a, %u) and (%a, %u)", a.first.first,
            a.first.second, b.first.first, b.first.second);
}

static float draw_distance(std::mt19937& rng, int mode) {
  std::uniform_real_distribution<float> u(0.0f, 4.0f);
  std::uniform_int_distribution<int> pick(0, 9), few(0, 3);
  switch (mode) {
    case 0: return u(rng);                         // distinct with probability ~1
    case 1: return (float)few(rng) * 0.25f;        // four values: many exact ties
    case 2: return 0.5f;                           // all equal
    default: {                                     // the special values among ordinary ones
      const int p = pick(rng);
      if (p == 0) return 0.0f;
      if (p == 1) return float_of(1u + (uint32_t)few(rng));   // subnormals
      if (p == 2) return INFINITY;
      if (p == 3) return 3.4028234663852886e38f;
      return u(rng);
    }
  }
}

template <int KC>
static long check_lists(std::mt19937& rng) {
  long checked = 0;
  const int lens[] = {0, 1, KC - 1, KC, KC + 1, 2 * KC + 3, 300};
  for (int mode = 0; mode < 4; ++mode)
    for (int len : lens)
      for (int order = 0; order < 3; ++order)
        for (int round = 0; round < 8; ++round, ++checked) {
          if (len < 0) continue;
          std::vector<std::pair<float, uint32_t>> cand((size_t)len);
          std::vector<uint32_t> idx((size_t)len);
          for (int i = 0; i < len; ++i) idx[(size_t)i] = (uint32_t)i * 7u + (round == 7 ? 0xfffff000u : 0u);
          std::shuffle(idx.begin(), idx.end(), rng);
          for (int i = 0; i < len; ++i) cand[(size_t)i] = {draw_distance(rng, mode), idx[(size_t)i]};
          std::vector<std::pair<float, uint32_t>> want = cand;
          std::sort(want.begin(), want.end());  // (d2, j): no NaN among the distances, so < on floats is a strict order
          if (order == 1) cand = want;
          if (order == 2) cand.assign(want.rbegin(), want.rend());
          RadiusList<KC> list;
          list.clear();
          CHECK(list.worst() == kRadiusListEmpty, "KC %d: an empty list's worst key", KC);
          for (const auto& c : cand) list.insert(radius_list_key(c.first, c.second));
          for (int t = 0; t < KC; ++t) {
            if (t < len) {
              const bool same = bits_of(radius_list_d2(list.top[t])) == bits_of(want[(size_t)t].first) &&
                                radius_list_index(list.top[t]) == want[(size_t)t].second;
              CHECK(same, "KC %d mode %d len %d order %d: slot %d holds (%a, %u), want (%a, %u)", KC, mode, len, order, t,
                    radius_list_d2(list.top[t]), radius_list_index(list.top[t]), want[(size_t)t].first,
                    want[(size_t)t].second);
            } else {
              CHECK(list.top[t] == kRadiusListEmpty, "KC %d mode %d len %d: slot %d is not empty", KC, mode, len, t);
            }
          }
          CHECK(list.worst() == list.top[KC - 1], "KC %d: worst() is the last slot", KC);
          if (len >= KC) {  // a key at or above the worst leaves the list as it is
            RadiusList<KC> before = list;
            list.insert(list.worst());
            list.insert(kRadiusListEmpty);
            CHECK(memcmp(before.top, list.top, sizeof(before.top)) == 0, "KC %d: a key at the worst changed the list", KC);
          }
        }
  return checked;
}

int main() {
  check_keys();
  std::mt19937 rng(20240611);
  long n = 0;
  n += check_lists<1>(rng);
  n += check_lists<2>(rng);
  n += check_lists<4>(rng);
  n += check_lists<5>(rng);
  n += check_lists<8>(rng);
  n += check_lists<9>(rng);
  n += check_lists<16>(rng);
  n += check_lists<17>(rng);
  n += check_lists<32>(rng);
  n += check_lists<33>(rng);
  n += check_lists<64>(rng);
  printf("%ld streams checked\n", n);
  if (violations) {
    printf("%d VIOLATION(s)\n", violations);
    return 1;
  }
  printf("no violation\n");
  return 0;
}
