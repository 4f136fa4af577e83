// cluster_union_main.cpp -- host check of csrc/cluster_union.h: the lock-free union-find of cluster_dbscan.  The
// functions are __host__ __device__ and the __hip_atomic builtins work in hipcc's host pass: this program runs the host
// side of exactly the code cluster_union_kernel runs, under host threads (and, in its second build, under
// ThreadSanitizer).  Launches no kernel; needs no GPU.  Prints the first violation and exits non-zero.
//
// Threads: 8 threads union 60 000 pseudo-random edges over 20 000 nodes, each thread a strided share, all at once; the
//   threads are joined; then find(i) of EVERY node must equal the smallest index of i's component, computed by a plain
//   sequential union-find over the same edges.  (Root = smallest index is what makes cluster_dbscan's labels canonical.)
//   Along the way: parent[i] <= i for every i, before and after.
// Chains: the edges (i, i + 1), i in [0, n - 1) for n = 20 000, once ascending and once descending, one thread, then
//   find(i) of every node, from node 0 up and from node n - 1 down: all roots are 0, and the number of loads of parent[]
//   stays within a bound.
//   Bound.  Ascending, every union finds two trees of depth <= 1: O(1) loads each.  Descending, every union hooks one
//   root under another without a single halving -- a path of depth n - 1 is built -- and the n finds that follow have
//   to flatten it.  Without halving, taken from the far end, they walk n (n - 1) / 2 = 2 * 10^8 edges.  With halving,
//   Tarjan and van Leeuwen ("Worst-case analysis of set union algorithms", JACM 31 (2), 1984) bound m finds on n nodes, under ANY linking
//   rule, by O(n + m log_(1 + m/n) n) iterations; here m = 2 (n - 1) + n finds (two per union, n at the end), so
//   log_(1 + m/n) n <= log_2 n.  An iteration of uf_find is two loads, and the last one of a find may be one.  The
//   program allows  loads <= 2 * 4 * (n + m) * (log2(n) + 1)  -- the 4 is slack for the constant the theorem hides --
//   which is 8 * 80 000 * 15.3 < 10^7: a factor 20 under the walk without halving, so a lost halving step fails here.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

namespace {
thread_local long long g_loads = 0;
}
#if defined(__HIP_DEVICE_COMPILE__)
#define POINTOPS_UF_ON_LOAD()
#else
#define POINTOPS_UF_ON_LOAD() (++g_loads)
#endif
#include "../../pytorch3d_pointops_amd/csrc/cluster_union.h"

namespace {

int violations = 0;
void fail(const char* what, long long got, long long want) {
  if (violations++ < 10) printf("VIOLATION %s: %lld (want %lld)\n", what, got, want);
}

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int seq_find(std::vector<int>& p, int i) {
  while (p[i] != i) {
    p[i] = p[p[i]];
    i = p[i];
  }
  return i;
}

void check_order(const std::vector<int>& parent, const char* what) {
  for (int i = 0; i < (int)parent.size(); ++i)
    if (parent[i] > i || parent[i] < 0) fail(what, parent[i], i);
}

void check_threads() {
  constexpr int kNodes = 20000, kEdges = 60000, kThreads = 8;
  std::vector<int> eu(kEdges), ev(kEdges);
  for (int e = 0; e < kEdges; ++e) {
    // half of the edges are local (long chains of nearby indices), half anywhere: both many components and big ones
    eu[e] = (int)(next_u64() % kNodes);
    ev[e] = (e & 1) ? (int)(next_u64() % kNodes) : std::min(kNodes - 1, eu[e] + 1 + (int)(next_u64() % 3));
    if (e % 4 == 3) eu[e] = ev[e] = (int)(next_u64() % (kNodes / 50)) * 50;  // self-loops: few edges, many singletons
  }
  std::vector<int> want(kNodes);
  for (int i = 0; i < kNodes; ++i) want[i] = i;
  for (int e = 0; e < kEdges; ++e) {  // sequential: hook the larger root under the smaller
    const int a = seq_find(want, eu[e]), b = seq_find(want, ev[e]);
    if (a != b) want[std::max(a, b)] = std::min(a, b);
  }
  std::vector<int> parent(kNodes);
  for (int i = 0; i < kNodes; ++i) parent[i] = i;
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([&, t]() {
      for (int e = t; e < kEdges; e += kThreads) pointops::uf_union(parent.data(), eu[e], ev[e]);
    });
  for (auto& th : threads) th.join();
  check_order(parent, "parent[i] > i after the threads");
  int components = 0;
  for (int i = 0; i < kNodes; ++i) {
    const int r = pointops::uf_find(parent.data(), i), w = seq_find(want, i);
    if (r != w) fail("root is not the smallest index of the component", r, w);
    components += w == i;
  }
  check_order(parent, "parent[i] > i after the finds");
  printf("threads: %d nodes, %d edges, %d threads, %d components\n", kNodes, kEdges, kThreads, components);
}

void check_chain(bool ascending, bool deep_first) {
  constexpr int n = 20000;
  std::vector<int> parent(n);
  for (int i = 0; i < n; ++i) parent[i] = i;
  g_loads = 0;
  for (int k = 0; k < n - 1; ++k) {
    const int i = ascending ? k : n - 2 - k;
    pointops::uf_union(parent.data(), i, i + 1);
  }
  for (int k = 0; k < n; ++k) {
    const int r = pointops::uf_find(parent.data(), deep_first ? n - 1 - k : k);
    if (r != 0) fail("chain root", r, 0);
  }
  const long long m = 2LL * (n - 1) + n;
  const long long bound = (long long)(2.0 * 4.0 * (double)(n + m) * (std::log2((double)n) + 1.0));
  printf("chain %s, finds from the %s end: %lld loads of parent[] (bound %lld, without halving ~%lld)\n",
         ascending ? "ascending" : "descending", deep_first ? "far" : "near", g_loads, bound, (long long)n * (n - 1) / 2);
  if (g_loads > bound) fail("chain loads", g_loads, bound);
  check_order(parent, "parent[i] > i after a chain");
}

}  // namespace

int main() {
  check_threads();
  for (int k = 0; k < 4; ++k) check_chain(k < 2, k % 2 == 1);
  if (violations) {
    printf("%d VIOLATIONS\n", violations);
    return 1;
  }
  printf("cluster_union: threaded unions, ascending and descending chains: no violation\n");
  return 0;
}
