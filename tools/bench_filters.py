#!/usr/bin/env python3
"""remove_radius_outlier and remove_statistical_outlier: the fused paths against the compositions a user had before
them, of the same definitions (one GPU).

    python tools/bench_filters.py [--out FILE] [--only radius|statistical] [--fused-only] [--shapes small|one]

Scenes: uniform points in the unit cube; the radius holds 15 other points on average (4/3 pi r^3 P = 15).
Per shape (N clouds of P points) one JSON line with HIP-event times, the median of 20 calls after 3 warm-ups:
  radius_ms         remove_radius_outlier(points, radius=r, min_neighbors=5): csrc/filters.hip, the early-exit walk and
                    the compaction, one native call
  radius_counts_ms  the same with return_counts=True: every walk finishes
  dbscan_ms         cluster_dbscan(points, r, 6).core_mask -- the same mask, with the union, flatten and relabel passes
  ball_ms           ball_query(points, points, K=6, radius=r) and its hits counted -- the same mask through a table
  argsort_ms        keypoints_to_padded(mask): the argsort compaction (a host read-back inside) mask_to_index replaces
  compact_ms        mask_to_index(mask)
  per K1 in (17, 31):
  stat_ms           remove_statistical_outlier(points, nb_neighbors=K1 - 1, std_ratio=2): knn_points + one native call
  knn_ms            knn_points(points, points, K=K1) alone: the share of stat_ms that is the search
  torch_ms          the composition: knn_points, sqrt / sum / mean / std / compare in torch, keypoints_to_padded
  mask_mismatches   rows where the composition's mask differs (its float32 reductions round differently: rows at the
                    threshold), of N * P
The masks of the radius compositions are asserted equal in the same run.  --fused-only times the fused paths alone
(for a kernel trace); --shapes one: 8 x 65536 only.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_cluster import timeit as _timeit  # noqa: E402
from pytorch3d_pointops_amd.functions import (ball_query, cluster_dbscan, keypoints_to_padded, knn_points,  # noqa: E402
                                              mask_to_index, remove_radius_outlier, remove_statistical_outlier)

SHAPES = [(8, 65536), (16, 131072), (2, 4096), (1, 16384)]  # (N, P)
NEIGHBOURS = 15.0
MIN_NEIGHBORS = 5
K1S = (17, 31)
STD_RATIO = 2.0


def timeit(fn):
    return _timeit(fn, warmup=3, iters=20)


def torch_statistical(points, K1, std_ratio):
    """PCL's definition in plain torch ops behind this library's knn_points -> (mask, idx, num)."""
    d = knn_points(points, points, K=K1).dists
    m = d.sqrt().sum(2) / (K1 - 1)
    thr = m.mean(1) + std_ratio * m.std(1)
    mask = m <= thr[:, None]
    return (mask,) + keypoints_to_padded(mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="all", choices=["all", "radius", "statistical"])
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--shapes", default="all", choices=["all", "small", "one"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_filters.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    shapes = {"all": SHAPES, "small": SHAPES[2:], "one": SHAPES[:1]}[args.shapes]
    for N, P in shapes:
        points = torch.from_numpy(np.random.default_rng(9900).uniform(0, 1, (N, P, 3)).astype(np.float32)).to(dev)
        r = (NEIGHBOURS / (P * 4.0 / 3.0 * math.pi)) ** (1.0 / 3.0)
        row = dict(N=N, P=P, radius=r, min_neighbors=MIN_NEIGHBORS)
        if args.only in ("all", "radius"):
            def fused(counts=False):
                return remove_radius_outlier(points, radius=r, min_neighbors=MIN_NEIGHBORS, return_counts=counts)

            sol = fused(True)
            row.update(radius_kept=int(sol.num_kept[0]), mean_count=float(sol.counts[0].float().mean()))
            row["radius_ms"] = timeit(fused)
            row["radius_counts_ms"] = timeit(lambda: fused(True))
            if not args.fused_only:
                core = cluster_dbscan(points, r, MIN_NEIGHBORS + 1).core_mask
                hits = (ball_query(points, points, K=MIN_NEIGHBORS + 1, radius=r, return_nn=False).idx >= 0).sum(2)
                assert torch.equal(core, sol.mask) and torch.equal(hits >= MIN_NEIGHBORS + 1, sol.mask)
                row["radius_masks_equal"] = True
                row["dbscan_ms"] = timeit(lambda: cluster_dbscan(points, r, MIN_NEIGHBORS + 1).core_mask)
                row["ball_ms"] = timeit(lambda: (ball_query(points, points, K=MIN_NEIGHBORS + 1, radius=r,
                                                            return_nn=False).idx >= 0).sum(2) >= MIN_NEIGHBORS + 1)
                idx, num = keypoints_to_padded(sol.mask)
                assert torch.equal(idx, sol.index[:, :idx.shape[1]]) and torch.equal(num, sol.num_kept)
                row["argsort_ms"] = timeit(lambda: keypoints_to_padded(sol.mask))
                row["compact_ms"] = timeit(lambda: mask_to_index(sol.mask))
                row["radius_vs_dbscan"] = row["dbscan_ms"] / row["radius_ms"]
                row["radius_vs_ball"] = row["ball_ms"] / row["radius_ms"]
            del sol
        if args.only in ("all", "statistical"):
            for K1 in K1S:
                def stat():
                    return remove_statistical_outlier(points, nb_neighbors=K1 - 1, std_ratio=STD_RATIO)

                s = stat()
                row[f"stat_kept_k{K1}"] = int(s.num_kept[0])
                row[f"stat_ms_k{K1}"] = timeit(stat)
                if not args.fused_only:
                    row[f"knn_ms_k{K1}"] = timeit(lambda: knn_points(points, points, K=K1))
                    row[f"knn_share_k{K1}"] = row[f"knn_ms_k{K1}"] / row[f"stat_ms_k{K1}"]
                    mask, idx, num = torch_statistical(points, K1, STD_RATIO)
                    row[f"mask_mismatches_k{K1}"] = int((mask != s.mask).sum())
                    row[f"torch_ms_k{K1}"] = timeit(lambda: torch_statistical(points, K1, STD_RATIO))
                    row[f"stat_speedup_k{K1}"] = row[f"torch_ms_k{K1}"] / row[f"stat_ms_k{K1}"]
                del s
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del points
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
