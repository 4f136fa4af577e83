// fps.hip -- iterative farthest point sampling for gfx950.
//
// Replaces FarthestPointSampling (reference:
// csrc/sample_farthest_points/sample_farthest_points.h:55-76) with the CPU path's
// semantics (sample_farthest_points_cpu.cpp:14-103): idx[n][0] = start_idxs[n];
// every further sample is the FIRST index with the largest running min-distance
// to the selected set (std::max_element), unfused fp32 distances, -1 padding
// beyond min(lengths[n], K[n]).
//
// Three kernels, one per way of holding a cloud's running min-distances:
//   fps_kernel<D>                     any D, any P: one workgroup per cloud, the distances in the workspace; also the
//                                     repair pass behind the clusters ("the single-workgroup kernel" of the notes below)
//   fps_single_kernel<D, PPT, BLOCK>  D in {2, 3}, a cloud that fits one workgroup's registers
//   fps_cluster_kernel<D, PPT>        D in {2, 3}, a cloud split over G > 1 workgroups that exchange their maxima
// The two register-resident ones share the argmax keys (fps_first_key, fps_update_keys); the cloud prologue is
// fps_open_cloud, which fps_single_kernel spells out for its schedule's sake (see there).
//
// MEMORY-MODEL NOTE on the cluster kernel's fastest exchange (fps_mode 2, the default where it verifies): members of
// a cloud publish their candidate with WORKGROUP-scope stores that OTHER workgroups poll with L1-bypassing loads.
// That hand-off is not promised by the HIP memory model; it works because gfx950's vector L1 is write-through and
// all members of a verified cloud share one XCD's L2.  It is therefore never trusted for correctness: a cloud only
// uses it after its members have proven (through the agent-scope protocol, row 0) that they run on one XCD, every
// spin is bounded, and a cloud whose exchange times out is flagged and recomputed by the single-workgroup kernel
// (tests force that with fps_spin_limit=0).  On another chip the guard would route every cloud to the agent-scope
// exchange or the repair pass -- slower, still exact.
#include <float.h>

#include "common.h"
#include "debug.h"
#include "zero_fill.h"

namespace pointops {

constexpr int kFpsBlock = 1024;
constexpr int kFpsWaves = kFpsBlock / kWave;
constexpr int kFpsSmallBlock = 256;  // clouds of up to 16 * 256 points: a wave per SIMD

// What every kernel needs of cloud n before its first iteration.
struct FpsCloud {
  int len, kn, last;  // points, samples (both clamped), start index
  int64_t* out;       // the cloud's row of idxs
};

// Fills `c` and, through the `block` lanes of a workgroup that `writer` nominates, writes the row's -1 padding beyond
// the samples this cloud produces and the start index.  A non-empty cloud always reports its start index, even with
// K[n] = 0 (sample_farthest_points_cpu.cpp:53-57 writes it before looking at K); an empty one is all -1.  Returns
// whether iterations remain.
__device__ __forceinline__ bool fps_open_cloud(FpsCloud& c, const int64_t* __restrict__ lengths,
                                               const int64_t* __restrict__ Ks, const int64_t* __restrict__ start_idxs,
                                               int64_t* __restrict__ idxs, int n, int P, int max_K, int tid, int block,
                                               bool writer) {
  c.len = (int)lengths[n];
  if (c.len > P) c.len = P;
  const int64_t kn64 = Ks[n];
  c.kn = (int)(kn64 < (int64_t)c.len ? kn64 : (int64_t)c.len);
  if (c.kn > max_K) c.kn = max_K;
  if (c.kn < 0) c.kn = 0;
  c.out = idxs + (int64_t)n * max_K;
  const int keep = c.len > 0 ? (c.kn > 1 ? c.kn : 1) : 0;
  if (writer) {
    for (int k = keep + tid; k < max_K; k += block) c.out[k] = -1;
  }
  if (c.len <= 0) return false;
  c.last = (int)start_idxs[n];
  if (c.last < 0 || c.last >= c.len) c.last = 0;  // guard (reference: undefined behaviour)
  if (writer && tid == 0) c.out[0] = c.last;
  return c.kn > 1;
}

__device__ __forceinline__ void argmax_combine(float& v, int& i, float ov, int oi) {
  // larger value wins; on equal values the lower index wins (first maximum)
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// ---------------------------------------------------------------------------
// v1 layout: one workgroup of 1024 lanes (16 wave64) per cloud; the running
// min-distance array lives in HBM/L2 (`min_dist_ws`, N*P floats), each lane owns
// the points p = tid, tid+1024, ... so no lane ever reads another lane's entry.
// Per iteration: update + per-lane argmax (strict > keeps the lowest index),
// wave argmax by xor-butterfly on (value, index) keys preferring the LOWER index on
// ties, one LDS exchange across the 16 waves, broadcast of the winner.
// ---------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kFpsBlock) void fps_kernel(
    const float* __restrict__ points, const int64_t* __restrict__ lengths,
    const int64_t* __restrict__ Ks, const int64_t* __restrict__ start_idxs, int P, int Drt,
    int max_K, int64_t* __restrict__ idxs, float* __restrict__ min_dist, const unsigned* __restrict__ only_flagged) {
  const int D = DT > 0 ? DT : Drt;
  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  // repair pass behind the cluster kernel: only the clouds whose exchange timed out are redone here
  if (only_flagged != nullptr && only_flagged[n] == 0u) return;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  FpsCloud cl;
  if (!fps_open_cloud(cl, lengths, Ks, start_idxs, idxs, n, P, max_K, tid, kFpsBlock, true)) return;
  const int len = cl.len;
  int64_t* __restrict__ out = cl.out;

  const float* __restrict__ pts = points + (int64_t)n * P * D;
  float* __restrict__ md = min_dist + (int64_t)n * P;
  for (int p = tid; p < len; p += kFpsBlock) md[p] = FLT_MAX;

  __shared__ float s_val[kFpsWaves];
  __shared__ int s_idx[kFpsWaves];
  __shared__ int s_last;

  int last = cl.last;
  for (int k = 1; k < cl.kn; ++k) {
    float best = -1.0f;
    int besti = 0x7fffffff;
    const float* __restrict__ c = pts + (int64_t)last * D;  // wave-uniform
    for (int p = tid; p < len; p += kFpsBlock) {
      const float* __restrict__ b = pts + (int64_t)p * D;
      float acc;
      {
        const float diff = c[0] - b[0];
        acc = diff * diff;
      }
      for (int d = 1; d < D; ++d) {
        const float diff = c[d] - b[d];
        acc = acc + diff * diff;
      }
      float m = md[p];
      if (acc < m) {
        m = acc;
        md[p] = m;
      }
      if (m > best) {
        best = m;
        besti = p;
      }
    }
    // wave64 argmax butterfly
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off, kWave);
      const int oi = __shfl_xor(besti, off, kWave);
      argmax_combine(best, besti, ov, oi);
    }
    if (lane == 0) {
      s_val[wave] = best;
      s_idx[wave] = besti;
    }
    __syncthreads();
    if (wave == 0) {
      float v = lane < kFpsWaves ? s_val[lane] : -2.0f;
      int ix = lane < kFpsWaves ? s_idx[lane] : 0x7fffffff;
#pragma unroll
      for (int off = kFpsWaves / 2; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, kWave);
        const int oi = __shfl_xor(ix, off, kWave);
        argmax_combine(v, ix, ov, oi);
      }
      if (lane == 0) {
        s_last = ix;
        out[k] = ix;
      }
    }
    __syncthreads();
    last = s_last;
  }
}

// ---------------------------------------------------------------------------
// Register-resident keys (D in {2, 3}).  Every lane keeps its PPT points AND their running min-distances in VGPRs,
// so an iteration touches no memory except the winner's coordinates and the reduction of the lanes' maxima.
//
// Argmax keys: (running min-distance bits << 32) | ~index.  Distances are >= +0 (padded slots carry -1.0f), so
// such a key, read as a double, is a non-NaN double whose order is the order we want: larger distance first,
// then the LOWER index (std::max_element's first maximum); a padded slot is a negative double, below every real
// one.  One v_max_f64 therefore replaces "compare distances, compare indices, two selects" -- and v_cndmask_b32
// pairs on a shared VCC cost ~22 cycles each on gfx950 (tools/valu_microbench.hip).
// ---------------------------------------------------------------------------
__device__ __forceinline__ double fps_max(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float fps_min(float a, float b) {  // IEEE minNum: a NaN distance never replaces the minimum
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// k = max(k, k of the lane that DPP control CTRL names); lanes outside the rows of ROWS keep k.  Two v_mov_b32_dpp and
// one v_max_f64: ~25 cycles a step, where the ds_bpermute pair of __shfl_xor costs ~120 (a trip through the LDS pipe)
template <int CTRL, int ROWS>
__device__ __forceinline__ double fps_dpp_max(double k) {
  const int hi = __double2hiint(k), lo = __double2loint(k);
  const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROWS, 0xf, false);
  const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROWS, 0xf, false);
  return fps_max(k, __hiloint2double(ohi, olo));
}
// maximum over each row of 16 lanes, in every lane of the row
__device__ __forceinline__ double fps_row_max(double k) {
  k = fps_dpp_max<0xB1, 0xf>(k);   // quad_perm [1,0,3,2]
  k = fps_dpp_max<0x4E, 0xf>(k);   // quad_perm [2,3,0,1]
  k = fps_dpp_max<0x124, 0xf>(k);  // row_ror 4
  k = fps_dpp_max<0x128, 0xf>(k);  // row_ror 8
  return k;
}
// maximum over the wave, wave-uniform (row maxima carried up the rows into lane 63, read back through SGPRs)
__device__ __forceinline__ double fps_wave_max(double k) {
  k = fps_row_max(k);
  k = fps_dpp_max<0x142, 0xa>(k);  // row_bcast15 into rows 1, 3
  k = fps_dpp_max<0x143, 0xc>(k);  // row_bcast31 into rows 2, 3
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(k), 63), __builtin_amdgcn_readlane(__double2loint(k), 63));
}
// the point a key's low word (~index) names
__device__ __forceinline__ int fps_key_index(unsigned lo) { return (int)(0xffffffffu - lo); }

// A point's first key: hi word = the running min-distance (FLT_MAX; the only part an iteration rewrites), lo word =
// ~index.  A slot beyond the cloud's length holds -1: never the maximum.
__device__ __forceinline__ double fps_first_key(bool valid, int p) {
  return __hiloint2double(__float_as_int(valid ? FLT_MAX : -1.0f), (int)(0xffffffffu - (unsigned)p));
}

// One iteration's arithmetic: the unfused squared distance of every owned point to the winner `c` goes into its key
// (padded slots keep -1: acc >= 0 is never below it); returns the wave's maximum key.
template <int DT, int PPT>
__device__ __forceinline__ double fps_update_keys(const float (&c)[DT], const float (&px)[PPT][DT], double (&mk)[PPT]) {
  double best = __hiloint2double(__float_as_int(-1.0f), 0);
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    float acc;
    {
      const float diff = c[0] - px[i][0];
      acc = diff * diff;
    }
#pragma unroll
    for (int d = 1; d < DT; ++d) {
      const float diff = c[d] - px[i][d];
      acc = acc + diff * diff;
    }
    const float m = fps_min(acc, __int_as_float(__double2hiint(mk[i])));
    mk[i] = __hiloint2double(__float_as_int(m), __double2loint(mk[i]));
    best = fps_max(best, mk[i]);
  }
  return fps_wave_max(best);
}

// ---------------------------------------------------------------------------
// One workgroup owns the cloud (up to PPT * BLOCK points): no exchange.  ONE barrier per iteration -- every wave
// reduces the waves' keys itself (double-buffered by iteration parity: a wave can be at most one barrier ahead of the
// slowest reader).  BLOCK = 1024: 16 waves, the clouds one cluster workgroup could hold; with four points per lane
// (up to 4096 points) the winner's coordinates come from an LDS copy of the cloud instead of a dependent load from
// global memory (~0.5 us of the 1.0 us iteration).  BLOCK = 256, clouds of up to 4096 points: FOUR waves -- a wave per
// SIMD --, always with the LDS copy, a barrier of 4 waves instead of 16 and, up to 1024 / 2048 points, a quarter / half
// of the arithmetic per iteration: 2 x 1024 points 0.84 -> 0.44 us per iteration, 2 x 4096 0.85 -> 0.77 (the
// reference's example sizes; tools/fps_small.py).
// ---------------------------------------------------------------------------
template <int DT, int PPT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void fps_single_kernel(
    const float* __restrict__ points, const int64_t* __restrict__ lengths, const int64_t* __restrict__ Ks,
    const int64_t* __restrict__ start_idxs, int P, int max_K, int64_t* __restrict__ idxs) {
  constexpr int kWaves = BLOCK / kWave;
  constexpr bool kLdsCopy = BLOCK == kFpsSmallBlock || PPT == 4;  // (48 KB at most)
  static_assert(kWaves <= 16 && (kWaves & (kWaves - 1)) == 0, "one DPP row holds the waves' keys");
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  __shared__ double s_key2[2][kWaves];
  __shared__ float s_pts[kLdsCopy ? PPT * BLOCK * DT : 1];
  // The cloud prologue in full, not through fps_open_cloud, and the start index stored behind the point loads: with
  // the shared helper inlined here the compiler orders the iteration's v_max_f64 chain differently, and the four-wave
  // instances -- one wave per SIMD, nothing to hide a stall behind -- took 1-1.7 % longer (profiles/fps_one_step_ab.txt).
  int len = (int)lengths[n];
  if (len > P) len = P;
  int64_t kn64 = Ks[n];
  int kn = (int)(kn64 < (int64_t)len ? kn64 : (int64_t)len);
  if (kn > max_K) kn = max_K;
  if (kn < 0) kn = 0;
  int64_t* __restrict__ out = idxs + (int64_t)n * max_K;
  const int keep = len > 0 ? (kn > 1 ? kn : 1) : 0;  // (the start index is reported even with K[n] = 0: fps_open_cloud)
  for (int k = keep + tid; k < max_K; k += BLOCK) out[k] = -1;
  if (len <= 0) return;
  if (kn <= 1) {
    int first = (int)start_idxs[n];
    if (first < 0 || first >= len) first = 0;
    if (tid == 0) out[0] = first;
    return;
  }
  const float* __restrict__ pts = points + (int64_t)n * P * DT;
  // this lane's points p = tid + i * BLOCK (ascending in i) and their keys
  float px[PPT][DT];
  double mk[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = tid + i * BLOCK;
    const bool valid = p < len;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      px[i][d] = valid ? pts[(int64_t)p * DT + d] : 0.0f;
      if constexpr (kLdsCopy) s_pts[p * DT + d] = px[i][d];
    }
    mk[i] = fps_first_key(valid, p);
  }
  int last = (int)start_idxs[n];
  if (last < 0 || last >= len) last = 0;
  if (tid == 0) out[0] = last;
  if constexpr (kLdsCopy) __syncthreads();
  for (int k = 1; k < kn; ++k) {
    float c[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) c[d] = kLdsCopy ? s_pts[last * DT + d] : pts[(int64_t)last * DT + d];
    const double best = fps_update_keys<DT, PPT>(c, px, mk);
    if (lane == 0) s_key2[k & 1][wave] = best;
    __syncthreads();
    const double v = fps_row_max(s_key2[k & 1][lane & (kWaves - 1)]);  // every lane: the workgroup's maximum
    last = __builtin_amdgcn_readfirstlane(fps_key_index((unsigned)__double2loint(v)));
    if (tid == 0) out[k] = last;
  }
}

// ---------------------------------------------------------------------------
// Clusters.  A cloud is split over G > 1 workgroups (G = ceil(P / (PPT*1024)), up to one workgroup per CU), each
// with its share of the points and keys in VGPRs, so an iteration touches no memory except the
// exchange: each workgroup reduces its local argmax and publishes it with ONE 8-byte store into its
// own slot of the (cloud, iteration) row -- key = distance bits << 32 | ~index, never 0; the key IS
// the message, so there is no flag, no counter and no fence (cdna guide G16, R2 "the data is the
// flag") -- then wave 0 polls the G slots of the row (L1-bypassing loads + s_sleep) until all are
// non-zero and takes their maximum: the largest distance and, on ties, the LOWEST index, i.e.
// std::max_element's first maximum.  Rows are per iteration, zeroed by a memset node before
// the launch; the points are read-only input.
//
// Placement (MODE, debug knob fps_mode).  Workgroups are dealt round-robin over the 8 XCDs, so blocks
// b and b + 8 share an XCD and its L2.  MODE 0 (round 1): member = blockIdx % G -- the G members of a
// cloud sit on all 8 XCDs, every exchange crosses the fabric and the dependent load of the winner's
// coordinates misses this XCD's L2 7 times out of 8.  MODE 1: the members of a cloud are blocks with
// equal blockIdx % 8 (one XCD when G <= CUs/8), same agent-scope exchange.  MODE 2: as 1, plus each
// cloud VERIFIES its placement once -- every member publishes its HW_REG_XCC_ID through the agent-scope
// protocol (row 0 of the cloud's slots, unused otherwise) -- and when all members report one XCD the
// per-iteration stores become workgroup-scope (written through the L1 into that XCD's L2, where the
// pollers' L1-bypassing loads find them) instead of agent-scope write-through to memory.  Placement is
// never assumed for correctness: an unverified cloud keeps the agent-scope protocol.
//
// Liveness.  All workgroups of the grid are resident by construction (grid <= CUs x occupancy of this
// kernel, queried from the runtime) unless another kernel or a CU mask takes CUs away; so every spin is
// bounded, a member whose wait times out flags ITS CLOUD in `timeout_flags` and abandons it, and the
// host enqueues the single-workgroup kernel behind this one for exactly the flagged clouds.  Results are
// therefore always the reference's; a timeout only costs time.
// Measured and dropped: four self-validating 8-byte units per slot (key + three tagged coordinates)
// so that the winner's coordinates arrive with its key instead of through the dependent load of
// pts[last] at the top of the iteration -- 3.07 -> 3.71 ms at 16 x 131072 -> 1024.
// ---------------------------------------------------------------------------
constexpr int kXcds = 8;

__device__ __forceinline__ unsigned xcc_id() {
  return __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xfu;  // HW_REG_XCC_ID[3:0]
}

// wave 0 of a member: wait until all G slots of `row` are non-zero, return their maximum (every lane);
// 0 after `spin_limit` polls without success.  Slot values are argmax keys (or the tiny placeholders 1 /
// 0x100 | xcc of the placement round): non-negative doubles, so the maximum is again v_max_f64.
__device__ __forceinline__ unsigned long long fps_gather_row(const unsigned long long* __restrict__ row, int G,
                                                             int lane, unsigned spin_limit) {
  double best = 0.0;
  bool ok = true;
  for (int base = 0; base < G && ok; base += kWave) {
    const int m = base + lane;
    unsigned long long mine = 1ull;
    unsigned spins = 0;
    for (;;) {
      mine = m < G ? __hip_atomic_load(row + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 1ull;
      if (__all(mine != 0ull)) break;
      __builtin_amdgcn_s_sleep(1);
      if (++spins > spin_limit) {  // exit condition every wave reaches
        ok = false;
        break;
      }
    }
    best = fps_max(best, __longlong_as_double((long long)mine));
  }
  best = fps_wave_max(best);
  return ok ? (unsigned long long)__double_as_longlong(best) : 0ull;
}

template <int DT, int PPT>
__global__ __launch_bounds__(kFpsBlock) void fps_cluster_kernel(
    const float* __restrict__ points, const int64_t* __restrict__ lengths,
    const int64_t* __restrict__ Ks, const int64_t* __restrict__ start_idxs, int N, int P, int max_K,
    int G, int n_clusters, int mode, unsigned spin_limit, unsigned long long* __restrict__ slots,
    unsigned* __restrict__ timeout_flags, int64_t* __restrict__ idxs) {
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  int cluster, member;
  if (mode == 0) {
    cluster = blockIdx.x / G;
    member = blockIdx.x - cluster * G;
  } else {
    // blocks with equal blockIdx % 8 share an XCD: deal each XCD's blocks to whole clusters
    const int x = blockIdx.x % kXcds, j = blockIdx.x / kXcds;  // j-th block of XCD group x
    cluster = (j / G) * kXcds + x;
    member = j % G;
  }
  if (cluster >= n_clusters) return;  // (grid rounded up to a multiple of 8 * G)
  __shared__ double s_key[kFpsWaves];
  __shared__ int s_last;
  __shared__ int s_flag;

  for (int n = cluster; n < N; n += n_clusters) {
    FpsCloud cl;  // (uniform over the cloud's members)
    if (!fps_open_cloud(cl, lengths, Ks, start_idxs, idxs, n, P, max_K, tid, kFpsBlock, member == 0)) continue;

    const float* __restrict__ pts = points + (int64_t)n * P * DT;
    // this lane's points: p = member*PPT*1024 + i*1024 + tid  (ascending in i) and their keys
    float px[PPT][DT];
    double mk[PPT];
    const int base = member * (PPT * kFpsBlock) + tid;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int p = base + i * kFpsBlock;
      const bool valid = p < cl.len;
#pragma unroll
      for (int d = 0; d < DT; ++d) px[i][d] = valid ? pts[(int64_t)p * DT + d] : 0.0f;
      mk[i] = fps_first_key(valid, p);
    }
    int64_t* __restrict__ out = cl.out;
    int last = cl.last;
    unsigned long long* __restrict__ cslots = slots + (int64_t)n * max_K * G;

    // MODE 2: one verified-placement round per cloud (row 0): all members on one XCD?
    bool same_xcd = false;
    bool dead = false;  // this member's wait timed out: abandon the cloud (the repair pass redoes it)
    if (mode == 2) {
      if (wave == 0) {
        const unsigned long long mine = 0x100ull | xcc_id();
        if (lane == 0) __hip_atomic_store(cslots + member, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long mx = fps_gather_row(cslots, G, lane, spin_limit);
        // all equal <=> max == every slot; re-read (they are final) and compare
        bool eq = mx != 0ull;
        for (int b2 = 0; b2 < G; b2 += kWave) {
          const int m = b2 + lane;
          const unsigned long long v = m < G ? __hip_atomic_load(cslots + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : mx;
          eq = eq && __all(v == mx);
        }
        if (lane == 0) s_flag = mx == 0ull ? -1 : (eq ? 1 : 0);
      }
      __syncthreads();
      same_xcd = s_flag == 1;
      dead = s_flag < 0;
    }

    for (int k = 1; k < cl.kn && !dead; ++k) {
      float c[DT];
#pragma unroll
      for (int d = 0; d < DT; ++d) c[d] = pts[(int64_t)last * DT + d];  // wave-uniform, read-only input
      const double best = fps_update_keys<DT, PPT>(c, px, mk);
      if (lane == 0) s_key[wave] = best;
      __syncthreads();
      if (wave == 0) {
        static_assert(kFpsWaves == 16, "one DPP row holds the waves' keys");
        double v = lane < kFpsWaves ? s_key[lane] : __hiloint2double(__float_as_int(-2.0f), 0);
        v = fps_row_max(v);  // (lanes 0..15: the workgroup's maximum)
        // this member's key: distance bits << 32 | ~index (never 0); 1 when it holds no valid point
        const unsigned long long key = __double2hiint(v) >= 0 ? (unsigned long long)__double_as_longlong(v) : 1ull;
        // Exchange, whole wave 0: lane 0 publishes this member's key with ONE store into its own slot
        // of the (cloud, iteration) row -- the 8-byte key IS the message -- then the lanes poll the G slots of
        // the row (one 128-byte line for G = 16) until all are non-zero and take the maximum: largest
        // distance, lowest index on ties.
        unsigned long long* __restrict__ rowk = cslots + (int64_t)k * G;
        if (lane == 0) {
          if (same_xcd) __hip_atomic_store(rowk + member, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          else __hip_atomic_store(rowk + member, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned long long bestk = fps_gather_row(rowk, G, lane, spin_limit);
        int win = fps_key_index((unsigned)(bestk & 0xffffffffull));
        if (bestk == 0ull) {
          win = -1;
          if (lane == 0) __hip_atomic_store(timeout_flags + n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
          s_last = win;
          if (member == 0 && win >= 0) out[k] = win;
        }
      }
      __syncthreads();
      last = s_last;
      if (last < 0) dead = true;  // (workgroup-uniform)
    }
    if (dead && tid == 0) __hip_atomic_store(timeout_flags + n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();  // s_last / s_key / s_flag reuse by the next cloud of this cluster
  }
}

}  // namespace pointops

using namespace pointops;

static int fps_num_cus() {
  // per DEVICE (a process may drive several GPUs; round 2 remembered the first device's count for all of them)
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cus[dev] == 0) {
    hipDeviceProp_t prop;
    int c = 0;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) c = prop.multiProcessorCount;
    cus[dev] = c > 0 ? c : 64;
  }
  return cus[dev];
}

// cluster geometry of the register-resident kernels: points per lane and workgroups per cloud.
// Round 3: a cloud that needs an exchange anyway (more than 8192 points) takes FOUR points per lane -- twice the
// workgroups, half the arithmetic per iteration and workgroup -- while the batch still gets a CU per workgroup and a cloud
// still fits one XCD: 1 x 131072 -> 1024: 1.50 -> 1.35 ms, 4 x 32768 -> 512: 0.73 -> 0.64, 32 x 16384 -> 256: 0.38 -> 0.34.
// Not beyond that: two workgroups per CU (the <3, 4> kernel held to 64 VGPRs) do not overlap each other's latency
// (16 x 131072: 1.51 -> 1.73 ms), and a cloud that fits one workgroup is fastest without an exchange (64 x 8192 -> 256:
// 0.26 against 0.33 ms).  tools/fps_plan_sweep.py, profiles/r03_fps_plan_sweep.txt.
static void fps_plan(int64_t N, int64_t P, int64_t D, int* ppt, int* G) {
  const int cus = fps_num_cus();
  int p = P <= 8 * (int64_t)kFpsBlock * cus ? 8 : 16;
  if (P <= 4 * (int64_t)kFpsBlock) p = 4;
  if (p == 8 && D == 3 && debug_knob("fps_small_ppt", 1) != 0) {
    const int64_t g4 = ceil_div(P, (int64_t)4 * kFpsBlock);
    if (P > 8 * (int64_t)kFpsBlock && N * g4 <= (int64_t)cus && g4 <= (int64_t)cus / 8) p = 4;
  }
  const long forced = debug_knob("fps_ppt", 0);  // experiments: 4 | 8 | 16
  if (forced == 4 || forced == 8 || forced == 16) p = (int)forced;
  *ppt = p;
  *G = (int)ceil_div(P > 0 ? P : 1, (int64_t)p * kFpsBlock);
}

// the (D, points per lane) instances of the single-workgroup and the cluster kernels: D in {2, 3}, the smallest
// PPT >= ppt
constexpr Ints<4, 8, 16> kFpsPpt{};
template <class F>
static auto with_fps_instance(int D, int ppt, F&& f) {
  return with_exact<2>(Ints<3, 2>{}, D, [&](auto DT) {
    return with_bucket(kFpsPpt, ppt, [&](auto PPT) { return f(DT, PPT); });
  });
}

// workgroups per cloud of the plan for the worst D (the size query has no D): only D = 3 may take fewer points per lane
static int fps_max_groups(int64_t N, int64_t P) {
  int ppt, G;
  fps_plan(N, P, 3, &ppt, &G);
  return G;
}

struct FpsWs {
  float* min_dist;            // v1 running min-distance array (N*P floats)
  unsigned long long* slots;  // v2 exchange rows: one u64 slot per (cloud, iteration, cluster member), directly
  unsigned* timeout_flags;    // followed by one timeout word per cloud (zeroed together)
  size_t slot_bytes;
};

static size_t fps_carve(FpsWs* ws, void* base, int64_t N, int64_t P, int64_t max_K, int G) {
  Carver c(base);
  FpsWs w;
  w.slot_bytes = sizeof(unsigned long long) * (size_t)(N * max_K) * (size_t)(G > 1 ? G : 1);
  w.min_dist = (float*)c.take(sizeof(float) * (size_t)(N * P));
  char* ex = c.take(w.slot_bytes + sizeof(unsigned) * (size_t)N + 64);
  w.slots = (unsigned long long*)ex;
  w.timeout_flags = (unsigned*)(ex ? ex + w.slot_bytes : nullptr);
  if (ws) *ws = w;
  return c.off;
}

extern "C" size_t pointops_fps_workspace_bytes(int64_t N, int64_t P, int64_t max_K) {
  return fps_carve(nullptr, nullptr, N, P, max_K, fps_max_groups(N, P));
}

// what the entry hands to each launch function
struct FpsArgs {
  const float* points;
  const int64_t *lengths, *K, *start_idxs;
  int N, P, D, max_K;
  int64_t* idxs;
  hipStream_t stream;
};

// any D: one workgroup per cloud, min-distances in the workspace; with `only_flagged`, the repair pass behind the
// clusters: a cloud that was not flagged returns at once
static int fps_launch_generic(const FpsArgs& a, const FpsWs& ws, const unsigned* only_flagged) {
  with_exact<0>(Ints<2, 3>{}, a.D, [&](auto DT) {
    hipLaunchKernelGGL((fps_kernel<DT>), dim3((unsigned)a.N), dim3(kFpsBlock), 0, a.stream, a.points, a.lengths, a.K,
                       a.start_idxs, a.P, a.D, a.max_K, a.idxs, ws.min_dist, only_flagged);
  });
  return check_launch(only_flagged ? "sample_farthest_points(repair)" : "sample_farthest_points");
}

// D in {2, 3}, P <= ppt * BLOCK: one workgroup of BLOCK lanes per cloud
template <int BLOCK>
static int fps_launch_single(const FpsArgs& a, int ppt) {
  with_fps_instance(a.D, ppt, [&](auto DT, auto PPT) {
    hipLaunchKernelGGL((fps_single_kernel<DT, PPT, BLOCK>), dim3((unsigned)a.N), dim3(BLOCK), 0, a.stream, a.points,
                       a.lengths, a.K, a.start_idxs, a.P, a.max_K, a.idxs);
  });
  return check_launch(BLOCK == kFpsSmallBlock ? "sample_farthest_points(small)" : "sample_farthest_points");
}

// workgroups of the cluster instance the device can hold at once: CUs x the runtime's occupancy answer (the exchange
// needs every workgroup of the grid resident); one 1024-lane workgroup per CU is what the plan uses
static int fps_cluster_resident(int D, int ppt) {
  return with_fps_instance(D, ppt, [&](auto DT, auto PPT) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fps_cluster_kernel<DT, PPT>, kFpsBlock, 0) != hipSuccess ||
        per_cu < 1) {
      (void)hipGetLastError();
      return 0;
    }
    return fps_num_cus();
  });
}

// D in {2, 3}, 1 < G <= resident: G workgroups per cloud over zeroed exchange slots and timeout words
static int fps_launch_clusters(const FpsArgs& a, const FpsWs& ws, int ppt, int G, int resident) {
  int mode = (int)debug_knob("fps_mode", 2);
  const int per_xcd = resident / kXcds;  // blocks that share an XCD under round-robin dispatch
  if (G > per_xcd || per_xcd < 1) mode = 0;  // a cloud does not fit one XCD: spread it (agent-scope exchange)
  int n_clusters = mode == 0 ? resident / G : (per_xcd / G) * kXcds;
  if (n_clusters > a.N) n_clusters = a.N;
  if (n_clusters < 1) n_clusters = 1;
  const int64_t words = (int64_t)(ws.slot_bytes / sizeof(unsigned)) + a.N;  // the slots and the timeout words
  const int zrc = zero_words_async(ws.slots, words, a.stream, "fps(zero)");
  if (zrc != POINTOPS_OK) return zrc;
  // XCD-local numbering: cluster c = (j / G) * 8 + x for the j-th block of XCD group x
  const int blocks = mode == 0 ? n_clusters * G : (int)ceil_div(n_clusters, kXcds) * G * kXcds;
  const unsigned spin_limit = (unsigned)debug_knob("fps_spin_limit", 1 << 20);
  with_fps_instance(a.D, ppt, [&](auto DT, auto PPT) {
    hipLaunchKernelGGL((fps_cluster_kernel<DT, PPT>), dim3((unsigned)blocks), dim3(kFpsBlock), 0, a.stream, a.points,
                       a.lengths, a.K, a.start_idxs, a.N, a.P, a.max_K, G, n_clusters, mode, spin_limit, ws.slots,
                       ws.timeout_flags, a.idxs);
  });
  return check_launch("sample_farthest_points");
}

extern "C" int pointops_sample_farthest_points(const float* points, const int64_t* lengths,
                                               const int64_t* K, const int64_t* start_idxs,
                                               int64_t N, int64_t P, int64_t D, int64_t max_K,
                                               int64_t* idxs, void* workspace, size_t workspace_bytes,
                                               void* stream_) {
  POINTOPS_REQUIRE(N >= 0 && P >= 0 && D >= 1 && max_K >= 0, "sample_farthest_points: bad sizes");
  POINTOPS_REQUIRE(P < (1LL << 31) && max_K < (1LL << 31) && D < (1LL << 16) && N < (1LL << 31),
                   "sample_farthest_points: sizes must fit int32");
  if (N == 0 || max_K == 0) return POINTOPS_OK;
  const size_t need = pointops_fps_workspace_bytes(N, P, max_K);
  POINTOPS_REQUIRE_WORKSPACE(workspace_fits(workspace, workspace_bytes, need),
                             "sample_farthest_points: workspace of %zu bytes required", need);
  int ppt, G;
  fps_plan(N, P, D, &ppt, &G);
  FpsWs ws;
  fps_carve(&ws, workspace, N, P, max_K, G);
  const FpsArgs a = {points, lengths, K, start_idxs, (int)N, (int)P, (int)D, (int)max_K, idxs, (hipStream_t)stream_};

  if ((D == 3 || D == 2) && P >= 1) {  // register-resident keys
    if (P <= 16 * kFpsSmallBlock && debug_knob("fps_small", 1) != 0)
      return fps_launch_single<kFpsSmallBlock>(a, (int)ceil_div(P, kFpsSmallBlock));
    if (G == 1) return fps_launch_single<kFpsBlock>(a, ppt);
    const int resident = fps_cluster_resident(a.D, ppt);
    if (G <= resident) {
      const int rc = fps_launch_clusters(a, ws, ppt, G, resident);
      if (rc != POINTOPS_OK) return rc;
      // clouds whose exchange timed out (CUs taken away by another kernel or a CU mask) are redone
      return fps_launch_generic(a, ws, ws.timeout_flags);
    }
  }
  return fps_launch_generic(a, ws, nullptr);
}
