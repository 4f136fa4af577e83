// voxel_key.h -- the per-cloud frame and the per-point key of voxel_downsample (voxel.hip): the origin, the cell function,
// the extent test that refuses a cloud, and the 63-bit key of a cell.  __host__ __device__ and free of HIP types:
// tests/native/voxel_key_main.cpp compiles this header alone, with any C++ compiler.  The definition these functions
// implement step by step is the comment block of pointops_voxel_downsample in include/pointops_amd.h; all arithmetic is
// fp64, unfused and in the order written (the build passes -ffp-contract=off).  Every decision is taken on doubles: a
// value is converted to an integer only after the comparisons have shown that it fits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define POINTOPS_VOXEL_HD __host__ __device__ inline
#else
#define POINTOPS_VOXEL_HD inline
#endif

namespace pointops {

constexpr int kVoxelAxisBits = 21;                    // cells per axis: three axes fill 63 bits of the key
constexpr double kVoxelMaxExtent = 2097152.0;         // 2^21: c_hi - c_lo must stay below it
constexpr double kVoxelMaxCell = 2147483648.0;        // 2^31: |c_lo| and |c_hi| must stay below it
constexpr uint64_t kVoxelDeadKey = ~(uint64_t)0;      // rows of no voxel: sorts behind every cell of the cloud
constexpr uint64_t kVoxelAxisMask = ((uint64_t)1 << kVoxelAxisBits) - 1;

// what the keys of one cloud are relative to
struct VoxelFrame {
  double o[3];      // the origin
  double lo[3];     // c_lo per axis: an integer value with |lo| < 2^31 unless the cloud is refused
  int32_t status;   // 0, or 1 for a refused cloud (which has no voxels)
  int32_t live;     // the cloud has a live row (an empty cloud is not refused and has no voxels either)
};

// Open3D's rule: the grid starts half a voxel below the smallest coordinate
POINTOPS_VOXEL_HD double voxel_default_origin(float min_a, float v) { return (double)min_a - 0.5 * (double)v; }

// c(x) = floor((x - o) / v): a division, monotone in x
POINTOPS_VOXEL_HD double voxel_cell(float x, double o, float v) { return floor(((double)x - o) / (double)v); }

// the extent rule on one axis.  Written with negated "fits" tests so that a NaN (a non-finite explicit origin) refuses.
POINTOPS_VOXEL_HD bool voxel_axis_refused(double c_lo, double c_hi) {
  const bool extent_ok = c_hi - c_lo < kVoxelMaxExtent;
  const bool range_ok = fabs(c_lo) < kVoxelMaxCell && fabs(c_hi) < kVoxelMaxCell;
  return !(extent_ok && range_ok);
}

// The frame of a cloud from the fp32 minimum and maximum over its live rows (ignored when it has none).
// origin: three floats, or null for the default rule.
POINTOPS_VOXEL_HD VoxelFrame voxel_frame(const float (&mn)[3], const float (&mx)[3], bool live, const float* origin,
                                         float v) {
  VoxelFrame f;
  f.status = 0;
  f.live = live ? 1 : 0;
  for (int a = 0; a < 3; ++a) {
    f.o[a] = 0.0;
    f.lo[a] = 0.0;
  }
  if (!live) return f;
  for (int a = 0; a < 3; ++a) {
    f.o[a] = origin != nullptr ? (double)origin[a] : voxel_default_origin(mn[a], v);
    const double c_lo = voxel_cell(mn[a], f.o[a], v), c_hi = voxel_cell(mx[a], f.o[a], v);
    f.lo[a] = c_lo;
    if (voxel_axis_refused(c_lo, c_hi)) f.status = 1;
  }
  if (f.status != 0)
    for (int a = 0; a < 3; ++a) f.lo[a] = 0.0;  // (nothing reads it: a refused cloud has dead keys only)
  return f;
}

POINTOPS_VOXEL_HD uint64_t voxel_pack(uint64_t dx, uint64_t dy, uint64_t dz) {
  return (dz << (2 * kVoxelAxisBits)) | (dy << kVoxelAxisBits) | dx;
}

POINTOPS_VOXEL_HD void voxel_unpack(uint64_t key, uint64_t (&d)[3]) {
  d[0] = key & kVoxelAxisMask;
  d[1] = (key >> kVoxelAxisBits) & kVoxelAxisMask;
  d[2] = (key >> (2 * kVoxelAxisBits)) & kVoxelAxisMask;
}

// The key of a live point of a cloud that is not refused: (c_z - lo_z) << 42 | (c_y - lo_y) << 21 | (c_x - lo_x).  The
// cell function is monotone and the point lies between the cloud's minimum and maximum, so every difference is an
// integer value in [0, 2^21): the conversion is exact.  A point outside that range (a caller's mistake: the frame is of
// another cloud) gets the dead key instead of an out-of-range conversion.
POINTOPS_VOXEL_HD uint64_t voxel_key(const VoxelFrame& f, float x, float y, float z, float v) {
  if (f.status != 0 || f.live == 0) return kVoxelDeadKey;
  const float p[3] = {x, y, z};
  uint64_t d[3];
  for (int a = 0; a < 3; ++a) {
    const double rel = voxel_cell(p[a], f.o[a], v) - f.lo[a];
    if (!(rel >= 0.0 && rel < kVoxelMaxExtent)) return kVoxelDeadKey;
    d[a] = (uint64_t)rel;
  }
  return voxel_pack(d[0], d[1], d[2]);
}

// the cell (relative to the origin) a key stands for, per axis: lo + d, |value| < 2^31 + 2^21
POINTOPS_VOXEL_HD int64_t voxel_coord(const VoxelFrame& f, uint64_t d, int axis) { return (int64_t)f.lo[axis] + (int64_t)d; }

}  // namespace pointops
