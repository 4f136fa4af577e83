#!/usr/bin/env python3
"""smooth_mls: the fused path, iss_keypoints at the same radius as a yardstick (the same walk with comparable
arithmetic, plus its suppression walk), and a plain-torch composition of the same definition (one GPU).

    python tools/bench_mls.py [--out FILE] [--only-fused] [--shapes small]

Scenes: N clouds of P points uniform in the unit cube (seeded).  Two radii per shape, r = (3 k / (4 pi P))^(1/3) for
k = 15 and k = 30 expected points per support.  Per shape and radius one JSON line with HIP-event times -- after 3
warm-ups, calls are timed one by one until 20 of them and 0.3 s of device time are in; the median and the fastest:
  fused_ms       smooth_mls(points, radius=r): csrc/mls.hip, one native call (iterations=2: fused2_ms)
  iss_ms         iss_keypoints(points, salient_radius=r, non_max_radius=2/3 r) on the same points in the same session
  allpairs_ms    the fused path with POINTOPS_DEBUG=mls_grid=0, at the shapes where that takes milliseconds, and whether
                 its bytes are the grid path's
  torch_ms       the definition composed in torch: a ball_query table with K = the largest support (read from the fused
                 path's num_neighbors: a composition with a smaller K truncates), a gather to (N, P, K, 3), the float32
                 weights and float64 quantized offsets, their float64 moments (sums of integers below 2^53: exact),
                 torch.linalg.eigh and the projection -- where the table fits: N P K <= 2^28
  torch_equal    the fraction of rows whose points are the fused path's bytes (eigh and the Jacobi differ in last bits),
                 torch_max_diff the largest difference
and the mean support, table_K and the status counts.  --only-fused times the fused path alone (for a kernel trace).
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
from bench_cluster import with_debug  # noqa: E402
from pytorch3d_pointops_amd.functions import ball_query, iss_keypoints, smooth_mls  # noqa: E402

SHAPES = [(2, 4096), (1, 16384), (8, 65536), (16, 131072)]  # (N, P)
NEIGHBOURS = (15, 30)
TABLE_LIMIT = 2 ** 28  # N P K of the composition's gathered tensor


def timeit(fn, warmup=3, min_calls=20, min_ms=300.0, max_calls=2000):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    while len(ts) < max_calls and (len(ts) < min_calls or sum(ts) < min_ms):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), len(ts)


def scene(N, P, seed=0):
    return np.random.default_rng(7700 + seed).uniform(0.0, 1.0, (N, P, 3)).astype(np.float32)


def mls_scale(r):
    m, k = math.frexp(float(np.float32(r)))
    return 2.0 ** (15 - (k - 1 if m == 0.5 else k))


def torch_composition(points, r, K, min_neighbors=3):
    """The definition of include/pointops_amd.h for a batch (N, P, 3) in plain torch ops (and this library's ball_query
    for the table) -> (points, normals, curvature, status)."""
    s = mls_scale(r)
    r32 = torch.tensor(r, dtype=torch.float32, device=points.device)
    r2 = r32 * r32
    idx = ball_query(points, points, K=K, radius=r, return_nn=False).idx  # (N, P, K), -1 padded
    hit = idx >= 0
    nb = torch.gather(points[:, None].expand(-1, points.shape[1], -1, -1), 2,
                      idx.clamp(min=0)[..., None].expand(-1, -1, -1, 3))  # (N, P, K, 3)
    d = points[:, :, None, :] - nb
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    u = 1.0 - d2 / r2
    w = u * u
    w = w * w
    wq = torch.round(w.double() * 4096.0) * hit  # (half to even)
    q = torch.round((nb.double() - points.double()[:, :, None, :]) * s) * hit[..., None]
    W = wq.sum(2)
    safe = W.clamp(min=1.0)
    wqq = wq[..., None] * q
    m = wqq.sum(2) / safe[..., None]
    M2 = torch.einsum("npka,npkb->npab", wqq, q)
    C = (M2 / safe[..., None, None] - m[..., :, None] * m[..., None, :]) * ((1.0 / s) * (1.0 / s))
    lam, vec = torch.linalg.eigh(C)
    n = vec[..., :, 0]
    big = n.abs().argmax(-1, keepdim=True)
    n = torch.where(torch.gather(n, -1, big) < 0, -n, n)
    n = n.float().double()  # the returned normal: the point moves along it
    delta = m / s
    h = (delta[..., 0] * n[..., 0] + delta[..., 1] * n[..., 1]) + delta[..., 2] * n[..., 2]
    nn = hit.sum(2)
    status = torch.where(nn < min_neighbors, 1, torch.where(lam[..., 1] <= 2.0 ** -20 * lam[..., 2], 2, 0))
    ok = (status == 0)[..., None]
    moved = (points.double() + h[..., None] * n).float()
    curv = (lam[..., 0] / ((lam[..., 0] + lam[..., 1]) + lam[..., 2])).float()
    zero = torch.full((), 0.0, device=points.device)
    return (torch.where(ok, moved, points), torch.where(ok, n.float(), zero), torch.where(ok[..., 0], curv, zero),
            status.to(torch.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--shapes", default="all", choices=["all", "small"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mls.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for N, P in (SHAPES[:2] if args.shapes == "small" else SHAPES):
        points = torch.from_numpy(scene(N, P)).to(dev)
        for k in NEIGHBOURS:
            r = (3.0 * k / (4.0 * math.pi * P)) ** (1.0 / 3.0)

            def fused(iterations=1):
                return smooth_mls(points, radius=r, iterations=iterations)

            sol = fused()
            status = torch.bincount(sol.status.flatten().long(), minlength=3).tolist()
            row = dict(N=N, P=P, neighbours=k, radius=r, mean_support=float(sol.num_neighbors.double().mean()),
                       table_K=int(sol.num_neighbors.max()), status_counts=status)
            row["fused_ms"], row["fused_min_ms"], row["fused_calls"] = timeit(fused)
            row["fused_ns_per_point"] = row["fused_ms"] * 1e6 / (N * P)
            if not args.only_fused:
                row["fused2_ms"] = timeit(lambda: fused(2))[0]
                row["iss_ms"], row["iss_min_ms"], _ = timeit(
                    lambda: iss_keypoints(points, salient_radius=r, non_max_radius=r * 2.0 / 3.0))
                if N * P * P <= 2 * 16384 * 16384:
                    row["allpairs_ms"] = timeit(with_debug("mls_grid=0", fused))[0]
                    other = with_debug("mls_grid=0", fused)()
                    row["allpairs_equal"] = bool(all(torch.equal(a, b) for a, b in zip(sol, other)))
                K = row["table_K"]
                if N * P * K <= TABLE_LIMIT:
                    got = torch_composition(points, r, K)
                    same = (got[0] == sol.points).all(-1)
                    row.update(torch_equal=float(same.float().mean()),
                               torch_max_diff=float((got[0] - sol.points).abs().max()),
                               torch_status_equal=bool(torch.equal(got[3], sol.status)))
                    del got, same
                    row["torch_ms"], row["torch_min_ms"], _ = timeit(lambda: torch_composition(points, r, K), warmup=2,
                                                                     min_calls=5, min_ms=0.0)
                    row["speedup"] = row["torch_ms"] / row["fused_ms"]
            line = json.dumps(row)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del sol
            torch.cuda.empty_cache()
        del points


if __name__ == "__main__":
    main()
