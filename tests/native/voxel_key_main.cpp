// voxel_key_main.cpp -- csrc/voxel_key.h on the host, compiled alone (no HIP header, no kernel, no GPU).
//
//   voxel_cell      at the faces k v of the grid (the point goes to the upper cell) and one ulp on either side, for
//                   several voxel sizes and signs; monotone over sorted random inputs with random origins and sizes
//   voxel_pack      round trips at 0 and at 2^21 - 1 on every axis, and the order of the keys: z, then y, then x
//   voxel_frame     the refusal at c_hi - c_lo in {2^21 - 1, 2^21} and at |c| in {2^31 - 1, 2^31}, both signs; the
//                   default origin (the lowest cell is 0); an empty cloud (status 0, dead keys); a NaN origin; and
//                   FLT_MAX over the smallest subnormal voxel size, which must reach the refusal without converting an
//                   out-of-range double to an integer (the sanitized build stops at such a conversion)
//   voxel_key       equals the packed differences of the cells, the dead key for a refused or empty frame and for a
//                   point outside the frame's extent
// Prints "no violation" when everything holds; a line with VIOLATION and exit status 1 otherwise.
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../pytorch3d_pointops_amd/csrc/voxel_key.h"

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

static void check_cell() {
  long n = 0;
  const float sizes[] = {0.25f, 1.0f, 0.5f, 8.0f, 0.0009765625f};  // powers of two: k v is exact in fp32
  for (float v : sizes) {
    for (int k = -300; k <= 300; ++k, ++n) {
      const float x = (float)k * v;
      CHECK(voxel_cell(x, 0.0, v) == (double)k, "cell(%a, v = %a) = %g, want %d", x, v, voxel_cell(x, 0.0, v), k);
      CHECK(voxel_cell(nextafterf(x, -INFINITY), 0.0, v) == (double)(k - 1), "one ulp below the face %d of v = %a", k, v);
      CHECK(voxel_cell(nextafterf(x, INFINITY), 0.0, v) == (double)k, "one ulp above the face %d of v = %a", k, v);
    }
  }
  CHECK(voxel_cell(-0.0f, 0.0, 1.0f) == 0.0, "-0.0 is in cell 0");
  CHECK(voxel_cell(0.3f, 0.1, 0.1f) == floor(((double)0.3f - 0.1) / (double)0.1f), "the expression as written");
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> coord(-1000.0f, 1000.0f), size(1e-3f, 10.0f);
  for (int round = 0; round < 200; ++round) {
    std::vector<float> xs(2000);
    for (float& x : xs) x = coord(rng);
    std::sort(xs.begin(), xs.end());
    const float v = size(rng);
    const double o = (double)coord(rng);
    double prev = voxel_cell(xs[0], o, v);
    for (float x : xs) {
      const double c = voxel_cell(x, o, v);
      CHECK(c >= prev, "cell not monotone at %a (o = %a, v = %a)", x, o, v);
      prev = c;
      ++n;
    }
  }
  printf("voxel_cell: %ld points\n", n);
}

static void check_pack() {
  const uint64_t top = ((uint64_t)1 << 21) - 1;
  const uint64_t ends[2] = {0, top};
  for (uint64_t x : ends)
    for (uint64_t y : ends)
      for (uint64_t z : ends) {
        uint64_t d[3];
        const uint64_t key = voxel_pack(x, y, z);
        voxel_unpack(key, d);
        CHECK(d[0] == x && d[1] == y && d[2] == z, "round trip of (%llu, %llu, %llu)", (unsigned long long)x,
              (unsigned long long)y, (unsigned long long)z);
        CHECK(key != kVoxelDeadKey && key < ((uint64_t)1 << 63), "a cell's key has 63 bits");
      }
  CHECK(voxel_pack(top, top, top) == ((uint64_t)1 << 63) - 1, "the largest key");
  CHECK(voxel_pack(top, top, 0) < voxel_pack(0, 0, 1) && voxel_pack(top, 0, 0) < voxel_pack(0, 1, 0), "z, then y, then x");
  std::mt19937_64 rng(3);
  for (int i = 0; i < 100000; ++i) {
    const uint64_t x = rng() & top, y = rng() & top, z = rng() & top;
    uint64_t d[3];
    voxel_unpack(voxel_pack(x, y, z), d);
    CHECK(d[0] == x && d[1] == y && d[2] == z, "random round trip");
  }
  printf("voxel_pack: ok\n");
}

static VoxelFrame frame_x(float lo, float hi, const float* origin, float v) {
  const float mn[3] = {lo, 0.5f, 0.5f}, mx[3] = {hi, 0.5f, 0.5f};
  return voxel_frame(mn, mx, true, origin, v);
}

static void check_frame() {
  const double two21 = 2097152.0, two31 = 2147483648.0;
  CHECK(!voxel_axis_refused(0.0, two21 - 1.0) && voxel_axis_refused(0.0, two21), "extent 2^21 - 1 / 2^21");
  CHECK(!voxel_axis_refused(-5.0, two21 - 6.0) && voxel_axis_refused(-5.0, two21 - 5.0), "extent from a negative c_lo");
  CHECK(!voxel_axis_refused(two31 - 2.0, two31 - 1.0) && voxel_axis_refused(two31 - 1.0, two31), "|c_hi| = 2^31");
  CHECK(!voxel_axis_refused(-(two31 - 1.0), -(two31 - 2.0)) && voxel_axis_refused(-two31, -(two31 - 1.0)), "|c_lo| = 2^31");
  CHECK(voxel_axis_refused(NAN, 0.0) && voxel_axis_refused(0.0, NAN) && voxel_axis_refused(-INFINITY, INFINITY), "NaN, inf");
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  // cells 0 and 2^21 - 1 / 2^21 through the frame (v = 1, origin 0)
  VoxelFrame f = frame_x(0.5f, 2097151.5f, zero, 1.0f);
  CHECK(f.status == 0 && f.lo[0] == 0.0, "extent 2^21 - 1 passes");
  CHECK(voxel_key(f, 2097151.5f, 0.5f, 0.5f, 1.0f) == voxel_pack(2097151, 0, 0), "the key of the last cell");
  CHECK(voxel_coord(f, 2097151, 0) == 2097151 && voxel_coord(f, 0, 1) == 0, "coords");
  f = frame_x(0.5f, 2097152.5f, zero, 1.0f);
  CHECK(f.status == 1 && voxel_key(f, 0.5f, 0.5f, 0.5f, 1.0f) == kVoxelDeadKey, "extent 2^21 refuses");
  // |c| = 2^31 - 1 / 2^31: x = 2^31 - 256 is an fp32 number, the origin moves x - o to 2^31 - 0.5 / 2^31
  const float x = 2147483392.0f;
  const float o_ok[3] = {-255.5f, 0.0f, 0.0f}, o_bad[3] = {-256.0f, 0.0f, 0.0f};
  f = frame_x(x - 1024.0f, x, o_ok, 1.0f);
  CHECK(f.status == 0 && f.lo[0] == two31 - 1025.0, "|c| = 2^31 - 1 passes");
  CHECK(voxel_coord(f, 1024, 0) == 2147483647LL, "the coordinate 2^31 - 1");
  CHECK(frame_x(x - 1024.0f, x, o_bad, 1.0f).status == 1, "|c| = 2^31 refuses");
  const float n_ok[3] = {255.0f, 0.0f, 0.0f}, n_bad[3] = {255.5f, 0.0f, 0.0f};
  f = frame_x(-x, -x + 1024.0f, n_ok, 1.0f);
  CHECK(f.status == 0 && voxel_coord(f, 0, 0) == -2147483647LL, "c = -(2^31 - 1) passes");
  CHECK(frame_x(-x, -x + 1024.0f, n_bad, 1.0f).status == 1, "c = -2^31 refuses");
  // the default origin: the smallest point sits half a voxel inside cell 0
  f = frame_x(-3.7f, 5.2f, nullptr, 0.3f);
  CHECK(f.status == 0 && f.lo[0] == 0.0 && f.o[0] == (double)-3.7f - 0.5 * (double)0.3f, "default origin");
  CHECK(voxel_key(f, -3.7f, 0.5f, 0.5f, 0.3f) == 0, "the smallest point has key 0");
  CHECK(voxel_key(f, 1e9f, 0.5f, 0.5f, 0.3f) == kVoxelDeadKey && voxel_key(f, -1e9f, 0.5f, 0.5f, 0.3f) == kVoxelDeadKey,
        "a point outside the frame gets the dead key");
  // an empty cloud, a NaN origin
  const float inf3[3] = {INFINITY, INFINITY, INFINITY}, ninf3[3] = {-INFINITY, -INFINITY, -INFINITY};
  f = voxel_frame(inf3, ninf3, false, nullptr, 1.0f);
  CHECK(f.status == 0 && f.live == 0 && voxel_key(f, 0.0f, 0.0f, 0.0f, 1.0f) == kVoxelDeadKey, "an empty cloud");
  const float o_nan[3] = {0.0f, NAN, 0.0f}, o_inf[3] = {INFINITY, 0.0f, 0.0f};
  CHECK(frame_x(0.0f, 1.0f, o_nan, 1.0f).status == 1 && frame_x(0.0f, 1.0f, o_inf, 1.0f).status == 1, "non-finite origin");
  // the widest extent over the smallest voxel size: 2 FLT_MAX / 2^-149 ~ 2^278 cells
  const float tiny = 1.401298464324817e-45f;  // the smallest subnormal
  const float big_mn[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX}, big_mx[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
  f = voxel_frame(big_mn, big_mx, true, nullptr, tiny);
  CHECK(f.status == 1 && voxel_key(f, FLT_MAX, 0.0f, 0.0f, tiny) == kVoxelDeadKey, "FLT_MAX over a subnormal voxel size");
  f = voxel_frame(big_mn, big_mx, true, zero, tiny);
  CHECK(f.status == 1, "the same with an explicit origin");
  f = voxel_frame(big_mx, big_mx, true, zero, tiny);  // one far point: no extent, but |c| ~ 2^277
  CHECK(f.status == 1, "a single point at FLT_MAX");
  f = voxel_frame(big_mx, big_mx, true, nullptr, tiny);  // ... which the default origin brings to cell 0
  CHECK(f.status == 0 && voxel_key(f, FLT_MAX, FLT_MAX, FLT_MAX, tiny) == 0, "a single point under the default origin");
  printf("voxel_frame: ok\n");
}

static void check_key() {
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> coord(-50.0f, 50.0f);
  long n = 0;
  for (int round = 0; round < 100; ++round) {
    const float v = 0.01f + 0.37f * (float)round;
    std::vector<float> p(3 * 500);
    for (float& x : p) x = coord(rng);
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < p.size(); ++i) {
      mn[i % 3] = std::min(mn[i % 3], p[i]);
      mx[i % 3] = std::max(mx[i % 3], p[i]);
    }
    const VoxelFrame f = voxel_frame(mn, mx, true, nullptr, v);
    CHECK(f.status == 0, "a cloud of extent 100 at v = %a is refused", v);
    for (size_t i = 0; i < p.size(); i += 3, ++n) {
      const uint64_t key = voxel_key(f, p[i], p[i + 1], p[i + 2], v);
      uint64_t d[3];
      voxel_unpack(key, d);
      for (int a = 0; a < 3; ++a)
        CHECK((double)voxel_coord(f, d[a], a) == voxel_cell(p[i + a], f.o[a], v), "key and cell disagree on axis %d", a);
    }
  }
  printf("voxel_key: %ld points\n", n);
}

int main() {
  check_cell();
  check_pack();
  check_frame();
  check_key();
  if (violations) {
    printf("%d VIOLATIONS\n", violations);
    return 1;
  }
  printf("no violation\n");
  return 0;
}
