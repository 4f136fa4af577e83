#!/usr/bin/env python3
"""ICP: the fused path against the torch composition over this package's own knn_points / knn_gather (one GPU).

    python tools/bench_icp.py [--out FILE] [--only-fused] [--iterations K]

Per shape (B clouds of P points of a synth.py distribution registered onto B clouds of P points: X is Y under a small
rigid motion, rows shuffled) one JSON line with HIP-event times.  Both paths run the same inputs for exactly
`iterations` iterations (relative_rmse_thr = -1):
  fused_ms_per_iter   iterative_closest_point (csrc/points_alignment.hip, the run's own reused search grid)
  torch_ms_per_iter   the composition a user writes from the public ops: knn_points, knn_gather, weighted means,
                      centring, bmm, torch.linalg.svd, det, apply, residual, .all()
  knn_ms              the K=1 search alone, rebuilt every call (reuse = 0)
  knn_reuse_ms        the K=1 search alone on a kept grid (reuse = 1); equals knn_ms where the shape is not the grid's
  kernels_ms          the new kernels alone: one iteration without its search (moments, solve, apply, finish)
  alignment_ms        corresponding_points_alignment alone (moments + solve)
and the agreement of the two paths after the last iteration (max |R| and |T| difference).
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
from pytorch3d_pointops_amd.functions import points_alignment as pa  # noqa: E402

SHAPES = [  # (B, P, distribution)
    (8, 65536, "uniform"),
    (8, 65536, "sphere"),
    (2, 4096, "uniform"),
    (2, 4096, "sphere"),
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


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def clouds(B, P, dist, dev):
    Y = np.stack([synth.distribution(dist, 1300 + b, P) for b in range(B)]).astype(np.float64)
    X = np.empty_like(Y)
    for b in range(B):
        R = rotation([1.0, 0.5 + b, -0.3], 0.02)
        perm = np.argsort(synth.splitmix64(77 + b, P))
        X[b] = (Y[b][perm] - 0.5 - np.array([0.004, -0.003, 0.002])) @ R.T + 0.5
    return torch.from_numpy(X.astype(np.float32)).to(dev), torch.from_numpy(Y.astype(np.float32)).to(dev)


def composition(X, Y, lengths, iterations):
    return pa._icp_torch(X, X, Y, lengths, lengths, iterations, -1.0, False, False, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--iterations", type=int, default=10)
    args = ap.parse_args()
    K = args.iterations
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for B, P, dist in SHAPES:
        X, Y = clouds(B, P, dist, dev)
        lengths = torch.full((B,), P, dtype=torch.int64, device=dev)
        row = dict(B=B, P=P, distribution=dist, iterations=K)
        fused = lambda: pa.iterative_closest_point(X, Y, max_iterations=K, relative_rmse_thr=-1)  # noqa: E731
        row["fused_ms_per_iter"] = timeit(fused) / K
        if not args.only_fused:
            with torch.no_grad():
                row["torch_ms_per_iter"] = timeit(lambda: composition(X, Y, lengths, K), warmup=1, iters=3) / K
            row["speedup"] = row["torch_ms_per_iter"] / row["fused_ms_per_iter"]
            state = _C.IcpState(X, X.clone(), Y, lengths, lengths, 1, False, False, -1.0)
            row["uses_grid"] = state.uses_grid

            def search(reuse):
                N, P1, P2, D = state.shape
                _C._call.knn_points_idx_reuse("knn", state.dev, state.Xt, state.Y, lengths, lengths, N, P1, P2, D, 2, 1, -1,
                                              state.idx, state.dists, state.knn_ws, state.knn_ws_bytes, reuse)

            row["knn_ms"] = timeit(lambda: search(0))
            row["knn_reuse_ms"] = timeit(lambda: search(1 if state.uses_grid else 0))

            def kernels():
                state.steps = 0
                state.step(search=False)

            row["kernels_ms"] = timeit(kernels)
            idx = state.idx.clone()
            row["alignment_ms"] = timeit(lambda: _C.points_alignment(X, Y, idx, lengths, None, False, False, 1e-9))
            a = fused()
            with torch.no_grad():
                _, _, _, hist = composition(X, Y, lengths, K)
            row["max_R_diff"] = float((a.RTs.R - hist[-1].R).abs().max())
            row["max_T_diff"] = float((a.RTs.T - hist[-1].T).abs().max())
            row["final_rmse"] = float(a.rmse.max())
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del X, Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
