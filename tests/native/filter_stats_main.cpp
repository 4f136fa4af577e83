// filter_stats_main.cpp -- csrc/filter_stats.h on the host, and nothing else of the library: the statistical outlier
// filter of a table of squared distances, evaluated by the header's own functions with one thread (filter_tree_sum is
// the summation tree written out).  tests/test_filters_cpu.py compiles this with the flags of the build (once plain,
// once with the host sanitizers), feeds it seeded tables and compares every output bit for bit with tests/filters_ref.py.
//
//   filter_stats_main IN OUT
//   IN : int64 N, P, K1; float32 std_ratio; int64 lengths[N]; float32 dists[N * P * K1]      (native byte order)
//   OUT: float32 mean_distance[N * P]; float64 stats[N * 3]; float32 threshold[N]; uint8 mask[N * P]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../pytorch3d_pointops_amd/csrc/filter_stats.h"

using namespace pointops;

template <typename T>
static bool read_n(FILE* f, T* p, size_t n) {
  return n == 0 || fread(p, sizeof(T), n, f) == n;
}
template <typename T>
static bool write_n(FILE* f, const T* p, size_t n) {
  return n == 0 || fwrite(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (in == nullptr) return 2;
  int64_t dims[3];
  float std_ratio;
  if (!read_n(in, dims, 3) || !read_n(in, &std_ratio, 1)) return 2;
  const int64_t N = dims[0], P = dims[1], K1 = dims[2];
  if (N < 0 || P < 0 || P > kFilterMaxPoints || K1 < 2 || K1 > kFilterMaxK1) return 2;
  std::vector<int64_t> lengths((size_t)N);
  std::vector<float> dists((size_t)(N * P * K1));
  if (!read_n(in, lengths.data(), lengths.size()) || !read_n(in, dists.data(), dists.size())) return 2;
  fclose(in);

  std::vector<float> m((size_t)(N * P)), threshold((size_t)N);
  std::vector<double> stats((size_t)(N * 3));
  std::vector<uint8_t> mask((size_t)(N * P));
  for (int64_t n = 0; n < N; ++n) {
    const int64_t len = lengths[n] < 0 ? 0 : (lengths[n] > P ? P : lengths[n]);
    const int cnt = (int)(K1 < len ? K1 : len);
    float* const mn = m.data() + n * P;
    for (int64_t i = 0; i < P; ++i)
      mn[i] = i < len ? filter_row_mean(dists.data() + (n * P + i) * K1, cnt) : 0.0f;
    int64_t nf = 0;
    for (int64_t i = 0; i < len; ++i) nf += filter_finite(mn[i]) ? 1 : 0;
    const double S1 =
        filter_tree_sum(P, [&](int64_t i) { return i < len && filter_finite(mn[i]) ? (double)mn[i] : 0.0; });
    const double mean = filter_mean(S1, nf);
    const double S2 = filter_tree_sum(
        P, [&](int64_t i) { return i < len && filter_finite(mn[i]) ? filter_deviation2(mn[i], mean) : 0.0; });
    const double std = filter_std(S2, nf);
    stats[n * 3 + 0] = mean, stats[n * 3 + 1] = std, stats[n * 3 + 2] = (double)nf;
    threshold[n] = filter_threshold(mean, std, std_ratio);
    for (int64_t i = 0; i < P; ++i) mask[n * P + i] = i < len && filter_keep(mn[i], threshold[n]) ? 1 : 0;
  }

  FILE* out = fopen(argv[2], "wb");
  if (out == nullptr) return 2;
  const bool ok = write_n(out, m.data(), m.size()) && write_n(out, stats.data(), stats.size()) &&
                  write_n(out, threshold.data(), threshold.size()) && write_n(out, mask.data(), mask.size());
  return fclose(out) == 0 && ok ? 0 : 2;
}
