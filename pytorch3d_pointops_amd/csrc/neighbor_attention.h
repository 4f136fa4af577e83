// neighbor_attention.h -- the host half of csrc/neighbor_attention.hip: how the heads of a query row are dealt over the
// lanes of a 256-lane workgroup (the NEIGHBOUR ATTENTION block of include/pointops_amd.h is the definition of the
// operator).  Plain C++ with no HIP header, so tests/native/neighbor_attention_main.cpp compiles it alone.
//
// A lane holds 4 channels (one 16-byte load; D % 4 == 0).  A head of D channels is Gh = D / 4 CONSECUTIVE lanes, Gh a
// power of two <= 64, so a head never straddles a wave and every per-head sum is a butterfly over Gh lanes whose order
// depends on D alone.  A group of G = min(64, pow2 >= heads Gh) lanes owns one query row and holds Hg = G / Gh whole
// heads at a time; a row with more heads is walked in `chunks` pieces of Hg heads, the last one a tail: lane j holds
// channels [4 (j % Gh), 4 (j % Gh) + 4) of head c Hg + j / Gh in chunk c, and is idle where that head is >= heads.
// The K slots of the 256 / G rows of a workgroup are staged in LDS `tile` slots of every row at a time: an int32 source
// and the Hg bias values of the heads in flight per (row, slot), in at most kNaTileWords words (32 KiB).
#pragma once
#include <stdint.h>

namespace pointops {

constexpr int kNaBlock = 256;         // lanes of a workgroup
constexpr int kNaMaxGroup = 64;       // lanes of a row at the most (a wave)
constexpr int kNaVec = 4;             // channels per lane and load
constexpr int kNaUnroll = 4;          // slots whose k row and v row are requested before the first dot
constexpr int kNaTileWords = 8192;    // staged words per workgroup: (1 + Hg) per (row, slot)
constexpr int kNaMaxD = 256;          // a head is at most a wave
constexpr int kNaMaxC = 1 << 16;

struct NaPlan {
  int Gh;      // lanes per head = D / 4
  int G;       // lanes per row
  int Hg;      // heads per group at a time = G / Gh
  int rows;    // rows per workgroup = kNaBlock / G
  int chunks;  // pieces of Hg heads per row
  int tile;    // slots of a row staged at a time (>= 1)
};

// D in {4, 8, 16, 32, 64, 128, 256}
inline bool na_head_ok(int64_t D) { return D >= kNaVec && D <= kNaMaxD && (D & (D - 1)) == 0; }

inline NaPlan na_plan(int64_t heads, int64_t D, int64_t K) {
  NaPlan p;
  p.Gh = (int)(D / kNaVec);
  p.G = p.Gh;
  while (p.G < kNaMaxGroup && p.G < heads * p.Gh) p.G *= 2;
  p.Hg = p.G / p.Gh;
  p.rows = kNaBlock / p.G;
  p.chunks = (int)((heads + p.Hg - 1) / p.Hg);
  const int64_t room = kNaTileWords / (p.rows * (1 + p.Hg));
  p.tile = (int)(K < 1 ? 1 : (K < room ? K : room));
  return p;
}

// bytes of dynamic LDS of the row kernels: the sources, then the bias of the heads in flight
inline size_t na_lds_bytes(const NaPlan& p) { return (size_t)p.rows * (size_t)p.tile * (size_t)(1 + p.Hg) * 4; }

}  // namespace pointops
