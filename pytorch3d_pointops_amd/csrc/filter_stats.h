// filter_stats.h -- the arithmetic of the statistical outlier filter (filters.hip): the mean distance of a row, which
// rows count, the summation tree of the cloud statistics, the standard deviation and the threshold.
// __host__ __device__ and free of HIP types: tests/native/filter_stats_main.cpp compiles this header alone, with any C++
// compiler.  The definition these functions implement step by step is the STATISTICAL FILTER block of
// include/pointops_amd.h; all arithmetic is unfused and in the order written (the build passes -ffp-contract=off).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define POINTOPS_FILTER_HD __host__ __device__ inline
#else
#define POINTOPS_FILTER_HD inline
#endif

namespace pointops {

constexpr int kFilterLanes = 256;                            // lanes of a chunk of the summation tree
constexpr int kFilterRowsPerLane = 16;                       // rows every lane adds one after the other
constexpr int kFilterChunk = kFilterLanes * kFilterRowsPerLane;  // 4096 rows
constexpr int kFilterMaxK1 = 128;                            // knn_points' longest list
constexpr int64_t kFilterMaxPoints = 1 << 24;

// step 1: m_i of a row from its cnt = min(K1, len) ascending squared distances, the row's own 0 among them
POINTOPS_FILTER_HD float filter_row_mean(const float* d2, int cnt) {
  if (cnt < 2) return 0.0f;
  double s = 0.0;
  for (int k = 0; k < cnt; ++k) s = s + sqrt((double)d2[k]);
  return (float)(s / (double)(cnt - 1));
}

// a row takes part in the statistics and can be kept (false for NaN and +-inf)
POINTOPS_FILTER_HD bool filter_finite(float m) { return fabsf(m) <= FLT_MAX; }

// the second pass's addend
POINTOPS_FILTER_HD double filter_deviation2(float m, double mean) {
  const double d = (double)m - mean;
  return d * d;
}

POINTOPS_FILTER_HD double filter_mean(double S1, int64_t nf) { return nf > 0 ? S1 / (double)nf : 0.0; }

POINTOPS_FILTER_HD double filter_std(double S2, int64_t nf) { return nf >= 2 ? sqrt(S2 / (double)(nf - 1)) : 0.0; }

// step 3
POINTOPS_FILTER_HD float filter_threshold(double mean, double std, float std_ratio) {
  return (float)(mean + (double)std_ratio * std);
}

POINTOPS_FILTER_HD bool filter_keep(float m, float threshold) { return filter_finite(m) && m <= threshold; }

// step 2's tree written out for ONE thread: the sum of v[0 .. P), a row i entering as term(i).  This is the
// definition the kernels of filters.hip follow with a thread per lane and a workgroup per chunk (host code: the test
// program holds it to the numpy replay).
template <typename Term>
inline double filter_tree_sum(int64_t P, Term term) {
  double total = 0.0;
  for (int64_t c0 = 0; c0 < P; c0 += kFilterChunk) {
    double s[kFilterLanes];
    for (int t = 0; t < kFilterLanes; ++t) {
      double a = 0.0;
      for (int j = 0; j < kFilterRowsPerLane; ++j) {
        const int64_t i = c0 + t + (int64_t)j * kFilterLanes;
        a = a + (i < P ? term(i) : 0.0);
      }
      s[t] = a;
    }
    for (int h = kFilterLanes / 2; h > 0; h >>= 1)
      for (int t = 0; t < h; ++t) s[t] = s[t] + s[t + h];
    total = total + s[0];
  }
  return total;
}

}  // namespace pointops
