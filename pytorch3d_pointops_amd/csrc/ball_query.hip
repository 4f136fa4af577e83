// ball_query.hip -- first-K-within-radius neighbour search for gfx950.
//
// Replaces BallQuery (reference: csrc/ball_query/ball_query.h:62-93) with the CPU
// path's semantics (csrc/ball_query/ball_query_cpu.cpp:12-54): for each query the
// first K points of p2 in INDEX order with dist2 < radius*radius (strict, fp32
// product), idx padded with -1 and dists with 0 (also for rows >= lengths1[n]).
//
// One lane per query.  A wave stops scanning as soon as all of its 64 queries are full
// (wave-uniform early exit via ballot), which on dense clouds is after ~1 % of p2
// (SURVEY.md section 3.2): the op is then bound by writing the (N,P1,K) outputs.
// There are two scans.  Queries in storage order (small calls without workspace) stream p2
// through the scalar path exactly as in knn.hip (wave-uniform address -> s_load -> SGPR
// operands): the loop inside `ball_query_kernel`.  Queries that come from a list (coarse-cell
// order, or what the grid left) take ONE tile scan, `ball_tile_scan`, which rejects whole tiles
// of p2 against the wave's bounding box; it is written once and knows nothing of where a hit
// goes.  Its two callers pass that as a sink: `ball_query_kernel` stores index and distance
// straight to the output row, `ball_query_list_kernel` (K % 4 == 0) stages the index in LDS
// and writes finished rows with 16-byte stores.
//
// SPARSE balls (few points inside the radius: the scan would walk most of the cloud for every
// query) go through the cell grid of knn_grid.hip instead when the caller provides the
// workspace: `ball_grid_lane_kernel` answers every query whose 3x3x3 cell cube provably contains
// its ball; per cloud the choice between grid and scan is made ON THE DEVICE from the bounding box
// (expected points per ball), and this kernel then scans only what is left: whole clouds whose
// flag is 0, and the listed (uncertified) queries of the others.
#include "common.h"
#include "debug.h"
#include "knn_common.h"
#include "knn_grid.h"
#include "wave.h"

namespace pointops {

constexpr int kBqBlock = 256;
constexpr int kBqTile = 8;  // points per scalar-load group of the storage-order scan

// Hit bit of one candidate into the lane's mask: `mask = 2 mask + (acc < radius2)` is ONE v_addc_co_u32 whose carry-in is
// the lane's bit of the compare result (cmp + select + shift + or: four instructions otherwise).  The first candidate of
// a group therefore ends up in the HIGHEST used bit.
__device__ __forceinline__ void push_hit(unsigned& mask, float radius2, float acc) {
  asm volatile("v_cmp_gt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mask) : "s"(radius2), "v"(acc) : "vcc");
}

// ---------------------------------------------------------------------------
// The TILE SCAN of one wave over its cloud (both kernels below, for their listed clouds): lane `lane` holds the query
// `a` (`active`: it has one) and wants its first `room` hits among q[0 .. len2) in index order; returns the lane's hit
// count.  What a hit does is the caller's: `sink(slot, j, ph)` with the row's slot, the point's index and the point
// itself (DT floats).
//
// Hits are rare per lane (a few %) but SOME lane of the wave hits on ~90 % of the candidates, so a per-candidate
// `if (hit) sink` runs its store block with one or two active lanes almost every iteration (66 cycles per wave-point
// measured vs ~26 of arithmetic).  Instead a tile only accumulates a 64-bit hit mask per lane (branch-free), and one
// expansion loop per tile then hands over the hits in bit (= index) order with every lane that still has a bit active.
//
// The wave's queries come in coarse-cell order (ball_grid.hip) or through the grid's fallback list, so their bounding
// box (exact min / max) is small next to the cloud.  The wave consumes p2 in TILES of 64 points, one per lane:
//  1. every lane tests ITS point against the wave's box: LB = the scan's own distance expression on the
//     per-dimension gaps fl(lo - c) / fl(c - hi) / 0.  fp32 subtraction, squaring and the sums are monotone,
//     so every query's COMPUTED distance to the point is >= LB; LB >= radius2 proves no lane can hit;
//  2. the surviving points (a ballot; ~10-15 % of a uniform cube at r = 0.2) are broadcast one by one
//     (v_readlane) and tested by all lanes: a hit sets bit b of the lane's 64-bit tile mask;
//  3. the lanes hand over their hits in bit (= index) order; the tile still sits in the lanes.
// (Round 1 tested every point in every lane through the scalar path: ~35 cycles per wave-point for what is
// now one vector instruction per 64 points plus ~50 cycles per surviving point.)
// ---------------------------------------------------------------------------
template <int DT, class Sink>
__device__ __forceinline__ int ball_tile_scan(const float (&a)[DT], bool active, const float* __restrict__ q, int len2,
                                              int room, float radius2, int lane, Sink&& sink) {
  float blo[DT], bhi[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    blo[d] = wave_min(active ? a[d] : __builtin_inff());
    bhi[d] = wave_max(active ? a[d] : -__builtin_inff());
  }
  int count = 0;
  int j0 = 0;
  float cn[DT];  // the NEXT tile's point of this lane, loaded one tile ahead
#pragma unroll
  for (int d = 0; d < DT; ++d) cn[d] = lane < len2 ? q[(int64_t)lane * DT + d] : 0.0f;
  while (j0 < len2 && __any(count < room)) {
    const int jc = j0 + lane;
    float c[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) c[d] = cn[d];
    {
      const int jn = jc + kWave;
#pragma unroll
      for (int d = 0; d < DT; ++d) cn[d] = jn < len2 ? q[(int64_t)jn * DT + d] : 0.0f;
    }
    float lb;
    {
      float g0 = fmaxf(fmaxf(blo[0] - c[0], c[0] - bhi[0]), 0.0f);
      lb = g0 * g0;
#pragma unroll
      for (int d = 1; d < DT; ++d) {
        const float gd = fmaxf(fmaxf(blo[d] - c[d], c[d] - bhi[d]), 0.0f);
        lb = lb + gd * gd;
      }
    }
    unsigned long long cand = __ballot(jc < len2 && lb < radius2);
    unsigned mlo = 0u, mhi = 0u;  // the lane's hits among the tile's points
    if (__popcll(cand) >= 48 && j0 + kWave <= len2) {
      // Most of the tile survives (queries in storage order, or a box as large as the cloud): the broadcast
      // loop would cost more than testing all 64 points through the scalar path (wave-uniform addresses ->
      // s_load, SGPR operands).  push_hit leaves the first point in the highest bit, hence the bit reversal.
      unsigned r0 = 0u, r1 = 0u;
      for (int jj = 0; jj < 32; jj += 8) {
        float t[8 * DT];
#pragma unroll
        for (int u = 0; u < 8 * DT; ++u) t[u] = q[(int64_t)(j0 + jj) * DT + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) push_hit(r0, radius2, pair_dist<DT, 2>(a, t + u * DT));
      }
      for (int jj = 32; jj < 64; jj += 8) {
        float t[8 * DT];
#pragma unroll
        for (int u = 0; u < 8 * DT; ++u) t[u] = q[(int64_t)(j0 + jj) * DT + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) push_hit(r1, radius2, pair_dist<DT, 2>(a, t + u * DT));
      }
      mlo = __brev(r0);
      mhi = __brev(r1);
      cand = 0ull;
    }
    while (cand != 0ull) {  // wave-uniform
      const int b = __builtin_ctzll(cand);
      cand &= cand - 1ull;
      float pb[DT];
#pragma unroll
      for (int d = 0; d < DT; ++d) pb[d] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c[d]), b));
      const bool hit = pair_dist<DT, 2>(a, pb) < radius2;
      const unsigned bit = 1u << (b & 31);
      if (b < 32) mlo |= hit ? bit : 0u;
      else mhi |= hit ? bit : 0u;
    }
    if (count >= room) mlo = mhi = 0u;
    while (__any((mlo | mhi) != 0u)) {  // wave-uniform loop: every lane takes part in the shuffles
      const unsigned long long m = ((unsigned long long)mhi << 32) | mlo;
      const bool has = m != 0ull;
      const int b = has ? __builtin_ctzll(m) : 0;
      float ph[DT];
#pragma unroll
      for (int d = 0; d < DT; ++d) ph[d] = __shfl(c[d], b, kWave);  // the tile still sits in the lanes
      if (has) {
        if (b < 32) mlo &= mlo - 1u;
        else mhi &= mhi - 1u;
        sink(count, j0 + b, ph);
        ++count;
        if (count >= room) mlo = mhi = 0u;
      }
    }
    j0 += kWave;
  }
  return count;
}

template <int DT>
__global__ __launch_bounds__(kBqBlock) void ball_query_kernel(
    const float* __restrict__ p1, const float* __restrict__ p2,
    const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2, int P1, int P2,
    int Drt, int K, float radius2, int tiles_per_cloud, const int* __restrict__ grid_flag,
    const int* __restrict__ qcount, const int* __restrict__ qlist, int64_t* __restrict__ idxs,
    float* __restrict__ dists) {
  const int D = DT > 0 ? DT : Drt;
  const int n = blockIdx.x / tiles_per_cloud;
  const int tile = blockIdx.x - n * tiles_per_cloud;
  int i = tile * kBqBlock + threadIdx.x;
  bool in_range = i < P1;
  const bool listed = grid_flag != nullptr && grid_flag[n];  // (workgroup-uniform)
  if (listed) {  // this cloud's queries come from a list: uncertified by the grid, or coarse-cell order
    if (tile * kBqBlock >= qcount[n]) return;
    in_range = i < qcount[n];
    i = in_range ? qlist[(int64_t)n * P1 + i] : 0;
  }
  const int len1 = (int)lengths1[n];
  int len2 = (int)lengths2[n];
  if (len2 > P2) len2 = P2;
  const int64_t row = (int64_t)n * P1 + (in_range ? i : 0);
  int64_t* __restrict__ orow_i = idxs + row * K;
  float* __restrict__ orow_d = dists + row * K;
  const bool active = in_range && i < len1;
  int count = 0;
  const float* __restrict__ q = p2 + (int64_t)n * P2 * D;

  if constexpr (DT > 0) {
    float a[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) a[d] = active ? p1[row * DT + d] : 0.0f;
    const int room = active ? K : 0;
    if (listed) {
      // a hit goes straight to the output row, its distance recomputed from the same operands (bit-identical)
      count = ball_tile_scan<DT>(a, active, q, len2, room, radius2, threadIdx.x & (kWave - 1),
                                 [&](int slot, int j, const float* ph) {
                                   orow_i[slot] = j;
                                   orow_d[slot] = pair_dist<DT, 2>(a, ph);
                                 });
    } else {
      // Queries in storage order (small calls without workspace): the wave's box is the cloud, nothing is
      // rejected, so every point goes through the scalar path (wave-uniform address -> s_load -> SGPR operands),
      // 32 points per round, hits collected as a per-lane bit mask (push_hit: the group's first candidate in the
      // highest used bit) and written by one expansion loop.
      int j = 0;
      while (j < len2 && __any(count < room)) {
        unsigned mask = 0u;
        const int jg = j;
        const int g_end = (j + 32 < len2) ? j + 32 : len2;
        for (; j + kBqTile <= g_end; j += kBqTile) {
          float t[kBqTile * DT];
  #pragma unroll
          for (int u = 0; u < kBqTile * DT; ++u) t[u] = q[(int64_t)j * DT + u];  // wave-uniform -> s_load
  #pragma unroll
          for (int jj = 0; jj < kBqTile; ++jj) push_hit(mask, radius2, pair_dist<DT, 2>(a, t + jj * DT));
        }
        for (; j < g_end; ++j) {
          float t[DT];
  #pragma unroll
          for (int u = 0; u < DT; ++u) t[u] = q[(int64_t)j * DT + u];
          push_hit(mask, radius2, pair_dist<DT, 2>(a, t));
        }
        const int top = g_end - jg - 1;  // bit of the group's first candidate
        if (count >= room) mask = 0u;
        while (__any(mask != 0u)) {
          if (mask != 0u) {
            const int b = 31 - __builtin_clz(mask);  // highest set bit = lowest index
            mask &= ~(1u << b);
            const int jh = jg + (top - b);
            float pb[DT];
  #pragma unroll
            for (int d = 0; d < DT; ++d) pb[d] = q[(int64_t)jh * DT + d];  // per-lane gather (L2-resident)
            orow_i[count] = jh;
            orow_d[count] = pair_dist<DT, 2>(a, pb);
            ++count;
            if (count >= room) mask = 0u;
          }
        }
      }
    }
  } else {
    if (active) {
      const float* __restrict__ a = p1 + row * D;
      for (int j = 0; j < len2 && count < K; ++j) {
        const float* __restrict__ b = q + (int64_t)j * D;
        float acc = 0.0f;
        for (int d = 0; d < D; ++d) {
          const float diff = a[d] - b[d];
          acc = acc + diff * diff;
        }
        if (acc < radius2) {
          orow_i[count] = j;
          orow_d[count] = acc;
          ++count;
        }
      }
    }
  }
  if (in_range) {
    for (int k = count; k < K; ++k) {
      orow_i[k] = -1;
      orow_d[k] = 0.0f;
    }
  }
}


// ---------------------------------------------------------------------------
// LISTED clouds with the hits STAGED IN LDS (D <= 3, K <= 64): one wave per workgroup, the tile scan of the
// kernel above, but a hit goes to the lane's row of an LDS image of the wave's 64 output rows (index as 32 bits +
// distance) instead of straight to memory, and every lane writes its finished row -- padding included -- with 16-byte
// stores.  The per-hit `orow_i[count] = j; orow_d[count] = d` of the kernel above is one 8-byte and one 4-byte store
// per lane into 64 different rows per instruction: measured at cfg3 (16 x 131072, r = 0.2, K = 32) WRITE_SIZE 3.2 GB
// for 0.8 GB of output, 70 % of the wave-cycles waiting for an issue slot behind the store queue
// (profiles/r03_ball_a_pmc.json).
// Row stride = 4 (2 ceil(K / 8) + 1) dwords: rows stay 16-byte aligned and the lanes' ds_read_b128 of their own rows
// fall into distinct banks.
// ---------------------------------------------------------------------------
__host__ __device__ inline int ball_stage_stride(int K) { return 4 * (2 * ((K + 7) / 8) + 1); }

#ifndef POINTOPS_BALL_LIST_WAVES
#define POINTOPS_BALL_LIST_WAVES 1
#endif
constexpr int kBqListWaves = POINTOPS_BALL_LIST_WAVES;  // independent waves per workgroup

template <int DT>
__global__ __launch_bounds__(kWave * kBqListWaves) void ball_query_list_kernel(
    const float* __restrict__ p1, const float* __restrict__ p2, const int64_t* __restrict__ lengths1,
    const int64_t* __restrict__ lengths2, int P1, int P2, int K, float radius2, const int* __restrict__ grid_flag,
    const int* __restrict__ qcount, const int* __restrict__ qlist, int64_t* __restrict__ idxs,
    float* __restrict__ dists) {
  extern __shared__ unsigned s_stage[];  // [64][stride] indices of the hits (distances are recomputed when the rows are
                                         // written: half the LDS, twice the waves per CU -- 5 resident of 8 possible
                                         // with the distances staged too, and the scan then waits on memory)
  const int n = blockIdx.y;
  const bool listed = grid_flag[n] != 0;  // (a cloud without a list -- empty, or ordering switched off: storage order)
  const int cnt = listed ? qcount[n] : P1;
  const int lane = threadIdx.x & (kWave - 1), wslot = threadIdx.x / kWave;
  const int base = (blockIdx.x * kBqListWaves + wslot) * kWave;
  if (base >= cnt) return;
  const bool in_range = base + lane < cnt;
  const int i = !in_range ? 0 : listed ? qlist[(int64_t)n * P1 + base + lane] : base + lane;
  const int len1 = (int)lengths1[n];
  int len2 = (int)lengths2[n];
  if (len2 > P2) len2 = P2;
  const int64_t row = (int64_t)n * P1 + i;
  const bool active = in_range && i < len1;
  const int stride = ball_stage_stride(K);
  unsigned* const my_i = s_stage + (wslot * kWave + lane) * stride;
  for (int k = 0; k < stride; k += 4)  // the row starts as padding: idx -1 (ball_query_cpu.cpp:20-21)
    *(uint4*)(my_i + k) = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
  const float* __restrict__ q = p2 + (int64_t)n * P2 * DT;
  float a[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) a[d] = active ? p1[row * DT + d] : 0.0f;
  // a hit's index goes to the lane's LDS row (the count is not needed: the row started as padding)
  ball_tile_scan<DT>(a, active, q, len2, active ? K : 0, radius2, lane,
                     [&](int slot, int j, const float*) { my_i[slot] = (unsigned)j; });
  // the lane's finished row: 16-byte pieces (two indices widened to int64, four distances recomputed from the chosen
  // points with the scan's expression -- the same operands, bit-identical); the caller guarantees K % 4 == 0, so
  // every row of the outputs is 16-byte aligned
  if (in_range) {
    int64_t* __restrict__ orow_i = idxs + row * K;
    float* __restrict__ orow_d = dists + row * K;
    for (int k = 0; k < K; k += 4) {
      const uint4 v = *(const uint4*)(my_i + k);
      const unsigned jv[4] = {v.x, v.y, v.z, v.w};
      float pt[4][DT];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned jx = jv[u] == 0xffffffffu ? 0u : jv[u];  // (padding: any valid address; its distance is 0)
#pragma unroll
        for (int d = 0; d < DT; ++d) pt[u][d] = q[(int64_t)jx * DT + d];
      }
      float dv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) dv[u] = jv[u] == 0xffffffffu ? 0.0f : pair_dist<DT, 2>(a, pt[u]);
      *(longlong2*)(orow_i + k) = make_longlong2((long long)(int)v.x, (long long)(int)v.y);
      *(longlong2*)(orow_i + k + 2) = make_longlong2((long long)(int)v.z, (long long)(int)v.w);
      *(float4*)(orow_d + k) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    }
  }
}

}  // namespace pointops

using namespace pointops;

// grid path considered (the per-cloud decision is made on the device): D <= 3, K <= 64, clouds large
// enough for the build passes to pay
static bool ball_grid_candidate(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  const long force = debug_knob("ball_grid", -1);  // 0 = never, 1 = whenever the shape allows (tests)
  if (force == 0) return false;
  // (its lane kernel keeps run bounds as (first, end) pairs: record indices up to the KNN grid's 2^24 - 16)
  if (force == 1) return D <= 3 && K <= 64 && N < 65536 && P2 <= knn_grid_max_points() && N > 0 && P1 > 0 && P2 > 0;
  return D <= 3 && K <= 64 && N < 65536 && P2 >= 4096 && P2 <= knn_grid_max_points() &&
         (double)N * (double)P1 * (double)P2 >= (double)(1LL << 27);
}

extern "C" size_t pointops_ball_query_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K) {
  if (!ball_grid_candidate(N, P1, P2, D, K)) return 0;
  return ball_grid_workspace_bytes(N, P1, P2);
}

extern "C" int pointops_ball_query(const float* p1, const float* p2, const int64_t* lengths1,
                                   const int64_t* lengths2, int64_t N, int64_t P1, int64_t P2,
                                   int64_t D, int64_t K, float radius, int64_t* idxs, float* dists,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
  POINTOPS_REQUIRE(N >= 0 && P1 >= 0 && P2 >= 0 && D >= 1 && K >= 0, "ball_query: bad sizes");
  POINTOPS_REQUIRE(P1 < (1LL << 31) && P2 < (1LL << 31) && K < (1LL << 31) && D < (1LL << 16),
                   "ball_query: sizes must fit int32");
  if (N == 0 || P1 == 0 || K == 0) return POINTOPS_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const float radius2 = radius * radius;  // fp32 product (ball_query_cpu.cpp:26)
  const int tiles = (int)ceil_div(P1, kBqBlock);
  POINTOPS_REQUIRE(N * tiles < (1LL << 31), "ball_query: grid too large");
  const int *flag = nullptr, *qcount = nullptr, *qlist = nullptr;
  const size_t need = pointops_ball_query_workspace_bytes(N, P1, P2, D, K);
  if (need > 0 && workspace != nullptr && workspace_bytes >= need) {
    const KnnArgs a = make_knn_args(p1, p2, lengths1, lengths2, N, P1, P2, D, K, tiles, idxs, dists, stream);
    const int rc = ball_grid_run(a, radius, workspace, &flag, &qcount, &qlist);
    if (rc != POINTOPS_OK) return rc;
  }
  if (flag == nullptr && ball_small_applies(N, P1, P2, D, K)) {  // few queries: one wave per query (ball_small.hip)
    launch_ball_small(p1, p2, lengths1, lengths2, N, P1, P2, D, K, radius2, idxs, dists, stream);
    return check_launch("ball_query(small)");
  }
  // listed clouds (every cloud once the lists exist) with hits staged in LDS: K a multiple of 4 up to 64
  const bool staged = flag != nullptr && D <= 3 && K <= 64 && K % 4 == 0 && debug_knob("ball_stage", 1) != 0;
  if (staged) {
    const size_t lds = (size_t)kBqListWaves * kWave * ball_stage_stride((int)K) * sizeof(unsigned);
    const dim3 lgrid((unsigned)ceil_div(P1, kWave * kBqListWaves), (unsigned)N);
    with_exact<3>(Ints<1, 2, 3>{}, (int)D, [&](auto DT) {
      hipLaunchKernelGGL((ball_query_list_kernel<DT>), lgrid, dim3(kWave * kBqListWaves), lds, stream, p1, p2, lengths1,
                         lengths2, (int)P1, (int)P2, (int)K, radius2, flag, qcount, qlist, idxs, dists);
    });
    return check_launch("ball_query(list)");
  }
  const dim3 grid((unsigned)(N * tiles)), block(kBqBlock);
  with_exact<0>(Ints<1, 2, 3, 4>{}, (int)D, [&](auto DT) {
    hipLaunchKernelGGL((ball_query_kernel<DT>), grid, block, 0, stream, p1, p2, lengths1, lengths2, (int)P1, (int)P2,
                       (int)D, (int)K, radius2, tiles, flag, qcount, qlist, idxs, dists);
  });
  return check_launch("ball_query");
}
