// cluster_union.h -- lock-free union-find over an int parent array (cluster.hip: the connected components of
// cluster_dbscan).  __host__ __device__: tests/native/cluster_union_main.cpp runs the host side of exactly this code
// under host threads.
//
// Every access to parent[] is a RELAXED, AGENT-scope atomic (loads, compare-exchange); there is no fence and no lane
// ever waits for another: a failed compare-exchange means somebody else made progress, and the caller starts over from
// find.  On gfx950 these are vector atomics and sc1 loads served by the memory side, so the per-XCD L2s, which are not
// coherent with each other, never hold a stale copy that matters (and none is needed: see "stale reads" below).
//
// Invariants (parent[i] == i initially; i is a ROOT while parent[i] == i):
//   I1  parent[i] <= i, always.
//   I2  parent[i] only decreases.
//   I3  a non-root never becomes a root again.
//   Writes are of two kinds, both a compare-exchange that replaces the value the writer has READ by a smaller one:
//     hook     CAS(parent[a], a, b) with b < a: a was a root and is one no more (I3: nothing ever stores i to parent[i]);
//     halving  CAS(parent[i], p, g) with g = a read of parent[p] < p < i: i was a non-root already, g is an ancestor of i.
//   A compare-exchange that finds another value does nothing, so I2 holds whatever the interleaving, and I1 with it.
// Stale reads: by I2 and I3 every value ever read from parent[i] is an ancestor-or-self of i in the forest of that
//   moment and of every later moment (a hook only adds an edge above a root, a halving replaces an edge by a path's
//   shortcut).  find therefore returns an ancestor that was a root when it was read; if it has been hooked since, the
//   hook of uf_union fails or links two nodes of what is one set already -- both harmless.
// Result: by I1 the root of a tree is its smallest index.  Once every edge has been through uf_union and all writers
//   have finished, every component is one tree, so find(i) = the smallest index of i's component, whatever the order of
//   arrival: the labelling is bit-reproducible despite the atomics.
// Path halving keeps a chain hooked in index order (depth P without it) from costing P loads per find; its writes go
//   to non-roots only, which never race with a hook (a hook's compare-exchange expects a root).
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define POINTOPS_UF_HD __host__ __device__ __forceinline__
#else
#error "cluster_union.h needs hipcc (the __hip_atomic builtins), also for its host side"
#endif

// a host test program counts the loads of parent[] through this hook
#ifndef POINTOPS_UF_ON_LOAD
#define POINTOPS_UF_ON_LOAD()
#endif

namespace pointops {

POINTOPS_UF_HD int uf_load(int* parent, int i) {
  POINTOPS_UF_ON_LOAD();
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[i]: expected -> desired; false when parent[i] held something else (nothing is written then)
POINTOPS_UF_HD bool uf_cas(int* parent, int i, int expected, int desired) {
  return __hip_atomic_compare_exchange_strong(parent + i, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
}

// An ancestor-or-self of i that was a root when it was read; THE root once all unions have finished.  Path halving:
// every other node of the walked path is re-pointed at its grandparent.
POINTOPS_UF_HD int uf_find(int* parent, int i) {
  for (;;) {
    const int p = uf_load(parent, i);
    if (p == i) return i;
    const int g = uf_load(parent, p);
    if (g == p) return p;
    (void)uf_cas(parent, i, p, g);  // g < p < i; a failure means parent[i] is smaller already
    i = g;
  }
}

// Merge the sets of a and b: the larger of the two roots is hooked under the smaller.  Returns that smaller root: an
// ancestor of both from now on, from which a caller with more edges at a may start its next union.
POINTOPS_UF_HD int uf_union(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return a;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    if (uf_cas(parent, a, a, b)) return b;  // a was still a root
  }
}

}  // namespace pointops
