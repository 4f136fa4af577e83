#!/usr/bin/env python3
"""Normals / local frames: the fused path against the five-stage torch composition (one GPU).

    python tools/bench_normals.py [--out FILE] [--only-fused]

Per shape (B clouds of P points of a synth.py distribution, K neighbours) one JSON line with HIP-event times:
  fused_ms      estimate_pointcloud_local_coord_frames (centring + knn_points + csrc/local_frames.hip)
  torch_ms      the composition a user builds today: centring, knn_points(return_nn=True) writing the (B,P,K,3)
                neighbourhood, the fused covariance over it, torch.linalg.eigh, the disambiguation in elementwise torch
  knn_ms        knn_points alone (idx only) on the centred cloud
  frames_ms     the fused local-frames kernel alone, on that knn_points' indices
and the agreement of the two paths: max |curvature difference| over the largest curvature, and the fraction of
points whose normals agree in sign (both disambiguated).  `frames_algo_bytes` is what the fused stage must move at
least: the (B,P,K) int64 indices, one 12-byte neighbour row per index, the query row and 48 bytes of output per point.
--only-fused times the fused path alone (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd import _C, synth  # noqa: E402
from pytorch3d_pointops_amd.functions import knn_points  # noqa: E402
from pytorch3d_pointops_amd.functions.points_normals import (  # noqa: E402
    centre_clouds, estimate_pointcloud_local_coord_frames)

SHAPES = [  # (B, P, K, distribution)
    (8, 65536, 16, "uniform"),
    (8, 65536, 50, "uniform"),
    (2, 4096, 16, "uniform"),
    (8, 65536, 16, "sphere"),
    (8, 65536, 16, "planes"),
]


def timeit(fn, warmup=2, iters=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def torch_composition(points, lengths, K):
    """Today's route to normals: five stages, the (B,P,K,3) neighbourhood written once and read twice."""
    c = centre_clouds(points, lengths)
    knn = knn_points(c, c, lengths, lengths, K=K, return_nn=True).knn
    cov = _C.point_covariances(knn)
    curvatures, frames = torch.linalg.eigh(cov)
    proj = ((knn - c[:, :, None, :])[..., None] * frames[:, :, None]).sum(3)  # (B,P,K,3): (x_k - x_i) . v_j
    flip = (proj > 0).sum(2) < 0.5 * K
    frames = frames * torch.where(flip, -1.0, 1.0)[:, :, None, :]
    n, z = frames[..., 0], frames[..., 2]
    return curvatures, torch.stack((n, torch.cross(n, z, dim=-1), z), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for B, P, K, dist in SHAPES:
        pts = torch.from_numpy(np.stack([synth.distribution(dist, 900 + b, P) for b in range(B)])).to(dev)
        lengths = torch.full((B,), P, dtype=torch.int64, device=dev)
        row = dict(B=B, P=P, K=K, distribution=dist)
        row["fused_ms"] = timeit(lambda: estimate_pointcloud_local_coord_frames(pts, K))
        if not args.only_fused:
            c = centre_clouds(pts, lengths)
            idx = knn_points(c, c, lengths, lengths, K=K).idx
            row["knn_ms"] = timeit(lambda: knn_points(c, c, lengths, lengths, K=K))
            row["frames_ms"] = timeit(lambda: _C.local_frames(c, lengths, idx, True))
            row["torch_ms"] = timeit(lambda: torch_composition(pts, lengths, K), warmup=1, iters=3)
            row["speedup"] = row["torch_ms"] / row["fused_ms"]
            nbytes = B * P * (K * 8 + K * 12 + 12 + 48)
            row["frames_algo_bytes"] = nbytes
            row["frames_algo_GBs"] = nbytes / row["frames_ms"] / 1e6
            lam, fr = estimate_pointcloud_local_coord_frames(pts, K)
            lam_t, fr_t = torch_composition(pts, lengths, K)
            row["max_curvature_rel_diff"] = float((lam - lam_t).abs().max() / lam_t.abs().max())
            row["normal_sign_agreement"] = float(((fr[..., 0] * fr_t[..., 0]).sum(-1) > 0).float().mean())
            del lam_t, fr_t, lam, fr, idx, c
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del pts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
