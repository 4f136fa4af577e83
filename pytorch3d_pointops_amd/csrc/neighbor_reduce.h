// neighbor_reduce.h -- the host half of csrc/neighbor_reduce.hip: how a row of C channels is dealt over the lanes of a
// 256-lane workgroup (the NEIGHBOUR REDUCE block of include/pointops_amd.h is the definition of the operator).  Plain
// C++ with no HIP header, so tests/native/neighbor_reduce_main.cpp compiles it alone.
//
// A lane holds V channels of its row at a time: V = 4 (one 16-byte load) when C is a multiple of 4, else V = 1 (the
// dword variant).  A group of G lanes owns one row; G is the power of two >= ceil(C / V), capped at 64 (a wave: the
// cross-lane sum of grad_w never leaves it).  A row wider than V G channels is walked in `chunks` pieces of V G
// channels, the last one a tail: lane j holds channels [(c G + j) V, (c G + j) V + V) of chunk c, and is idle where
// that starts at or beyond C (with V = 4 a lane is never partly filled, since C % 4 == 0).
// The K slots of the 256 / G rows of a workgroup are staged in LDS `tile` slots of every row at a time, in at most
// kNrTileEntries entries (16 KiB of sources + 16 KiB of weights): one tile whenever K <= tile, which with G = 64 (the
// only width with more than one chunk) is K <= 1024.
#pragma once
#include <stdint.h>

namespace pointops {

constexpr int kNrBlock = 256;         // lanes of a workgroup
constexpr int kNrMaxGroup = 64;       // lanes of a row at the most
constexpr int kNrUnroll = 4;          // independent row loads in flight per lane before the first add
constexpr int kNrTileEntries = 4096;  // staged (row, slot) entries per workgroup
constexpr int kNrMaxK = 255;          // `max`: the slot goes into a byte, 255 = none
constexpr int kNrMaxC = 1 << 16;

enum { kNrSum = 0, kNrMean = 1, kNrMax = 2 };

struct NrPlan {
  int V;       // channels per lane and load: 4 or 1
  int G;       // lanes per row
  int rows;    // rows per workgroup = kNrBlock / G
  int chunks;  // pieces of V G channels per row
  int tile;    // slots of a row staged at a time (>= 1)
};

inline NrPlan nr_plan(int64_t C, int64_t K) {
  NrPlan p;
  p.V = (C % 4 == 0) ? 4 : 1;
  const int64_t units = (C + p.V - 1) / p.V;
  p.G = 1;
  while (p.G < kNrMaxGroup && p.G < units) p.G *= 2;
  p.rows = kNrBlock / p.G;
  p.chunks = (int)((units + p.G - 1) / p.G);
  const int64_t room = kNrTileEntries / p.rows;
  p.tile = (int)(K < 1 ? 1 : (K < room ? K : room));
  return p;
}

// bytes of dynamic LDS of the forward kernel: the sources, and the weights when there are any
inline size_t nr_lds_bytes(const NrPlan& p, bool weighted) {
  return (size_t)p.rows * (size_t)p.tile * (weighted ? 8 : 4);
}

}  // namespace pointops
