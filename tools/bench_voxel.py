#!/usr/bin/env python3
"""voxel_downsample: the fused path against the usual torch composition of the same pooling (one GPU).

    python tools/bench_voxel.py [--out FILE] [--only-fused] [--shapes small]

Scenes: bench_cluster.py's (40 % uniform background, 60 % Gaussian blobs).  Per shape (N clouds of P points) two voxel
sizes, found by bisection on cloud 0 with the fused call itself: about 8 points per voxel and about 1 point per voxel
(points per voxel = P / num_voxels); per voxel size C = 0 and C = 3 (normals).  One JSON line per case with HIP-event
times, the median of 5 calls after 2 warm-ups:
  fused_ms   voxel_downsample(points, voxel_size=v[, features=normals]): csrc/voxel.hip, one native call, static shapes
  torch_ms   floor((x - o) / v) in float64 with the same origin rule, torch.unique(dim=0, return_inverse=True) over
             (cloud, z, y, x), index_add_ of points (and features) and of ones, a divide: data-dependent output shape (a
             host synchronisation inside torch.unique), atomic float sums
with the voxel counts asserted equal and the composition's centroids compared with the fused ones (max abs difference
reported: the composition sums in float32 atomics).  --only-fused times the fused path alone (for a kernel trace).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_cluster import scene, timeit  # noqa: E402
from pytorch3d_pointops_amd.functions import voxel_downsample  # noqa: E402

SHAPES = [(8, 65536), (16, 131072), (2, 4096), (1, 16384)]  # (N, P)
TARGETS = (8.0, 1.05)  # points per voxel ("about 1": the smallest voxel size at which 5 % of the points share a voxel)


def pick_voxel_size(points, target):
    """v with P / num_voxels of cloud 0 closest to `target` from above (bisection in log space, 24 steps; a size so small
    that the cloud is refused counts as below the target)."""
    p = points[:1]
    lo, hi = 1e-7, 2.0  # one point per voxel ... one voxel per cloud
    for _ in range(24):
        mid = (lo * hi) ** 0.5
        voxels = int(voxel_downsample(p, voxel_size=mid).num_voxels[0])
        if voxels == 0 or p.shape[1] / voxels < target:
            lo = mid
        else:
            hi = mid
    return hi


def torch_composition(points, v, features=None):
    """-> (num_voxels (N,), centroids (V_total, 3), pooled (V_total, C) or None, inverse (N * P,)) in plain torch ops."""
    N, P, _ = points.shape
    v64 = torch.tensor(v, dtype=torch.float32, device=points.device).double()
    o = points.min(1, keepdim=True).values.double() - 0.5 * v64
    cell = torch.floor((points.double() - o) / v64).to(torch.int64)
    cloud = torch.arange(N, device=points.device)[:, None, None].expand(N, P, 1)
    keys = torch.cat([cloud, cell.flip(-1)], 2).reshape(N * P, 4)  # (cloud, z, y, x): unique sorts rows this way
    uniq, inverse = torch.unique(keys, dim=0, return_inverse=True)
    V = uniq.shape[0]
    values = points if features is None else torch.cat([points, features], 2)
    sums = torch.zeros(V, values.shape[2], dtype=torch.float32, device=points.device)
    sums.index_add_(0, inverse, values.reshape(N * P, -1))
    counts = torch.zeros(V, dtype=torch.float32, device=points.device)
    counts.index_add_(0, inverse, torch.ones(N * P, dtype=torch.float32, device=points.device))
    mean = sums / counts[:, None]
    num = torch.bincount(uniq[:, 0], minlength=N)
    return num, mean[:, :3], (None if features is None else mean[:, 3:]), inverse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--shapes", default="all", choices=["all", "small"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for N, P in (SHAPES[2:] if args.shapes == "small" else SHAPES):
        points = torch.from_numpy(scene(N, P)).to(dev)
        normals = torch.nn.functional.normalize(torch.randn(N, P, 3, device=dev, generator=torch.Generator(dev).manual_seed(3)), dim=2)
        for target in TARGETS:
            v = pick_voxel_size(points, target)
            for feats in (None, normals):
                fused = lambda: voxel_downsample(points, voxel_size=v, features=feats)  # noqa: E731
                sol = fused()
                total = int(sol.num_voxels.sum())
                row = dict(N=N, P=P, C=0 if feats is None else 3, voxel_size=v, points_per_voxel=N * P / total,
                           voxels=total, largest_voxel=int(sol.counts.max()))
                row["fused_ms"] = timeit(fused)
                row["fused_ns_per_point"] = row["fused_ms"] * 1e6 / (N * P)
                if not args.only_fused:
                    num, mean, pooled, _ = torch_composition(points, v, feats)
                    assert torch.equal(num, sol.num_voxels), "the composition finds other voxel counts"
                    keep = torch.arange(P, device=dev)[None, :] < sol.num_voxels[:, None]  # (both in (cloud, z, y, x) order)
                    row["centroid_max_abs_diff"] = float((sol.points[keep] - mean).abs().max())
                    row["torch_ms"] = timeit(lambda: torch_composition(points, v, feats))
                    row["speedup"] = row["torch_ms"] / row["fused_ms"]
                line = json.dumps(row)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del sol
        del points, normals
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
