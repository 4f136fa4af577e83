#!/usr/bin/env python3
"""cluster_dbscan: the fused path, and at one shape a plain-torch composition of the same definition (one GPU).

    python tools/bench_cluster.py [--out FILE] [--only-fused] [--shapes small]

Scene: every cloud is 40 % uniform background in the unit cube and 60 % Gaussian blobs (32 per cloud, sigma 0.04); eps is
the median distance to the 15th nearest point (itself included) of 4096 sampled points of cloud 0, so a point has ~15
neighbours; min_points = 10.  Per shape (N clouds of P points) one JSON line with HIP-event times, the median of 5 calls
after 2 warm-ups:
  fused_ms           cluster_dbscan(points, eps, 10): csrc/cluster.hip, one native call
  allpairs_ms        the same with POINTOPS_DEBUG=cluster_grid=0 (every cloud by all pairs), at the shapes where that
                     takes milliseconds
  torch_ms           at 1 x 16384 only: the definition composed in torch -- the P x P `d2 < r2` in blocks of rows, core
                     counts, min-label propagation over the core graph until nothing moves, border labels, relabel --
                     with label equality asserted
  sklearn_cpu_ms     where scikit-learn is importable: its DBSCAN on the CPU, for context (one run, wall clock)
and clusters / core / noise counts of cloud 0.  --only-fused times the fused path alone (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd.functions import cluster_dbscan  # noqa: E402

SHAPES = [(8, 65536), (16, 131072), (2, 4096), (1, 16384)]  # (N, P)
TORCH_SHAPE = (1, 16384)
MIN_POINTS = 10
NEIGHBOURS = 15


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


def scene(N, P, seed=0):
    rng = np.random.default_rng(9900 + seed)
    out = np.empty((N, P, 3), np.float32)
    for n in range(N):
        c = rng.uniform(0.1, 0.9, (32, 3))
        p = c[rng.integers(0, 32, P)] + rng.normal(0, 0.04, (P, 3))
        nb = (2 * P) // 5
        p[:nb] = rng.uniform(0, 1, (nb, 3))
        out[n] = p[rng.permutation(P)]
    return out


def pick_eps(points):
    """Median distance to the NEIGHBOURS-th nearest point (itself included) over 4096 sampled points of cloud 0."""
    p = points[0]
    q = p[torch.randperm(p.shape[0], device=p.device, generator=torch.Generator(p.device).manual_seed(1))[:4096]]
    d = torch.cdist(q, p)
    return float(d.topk(NEIGHBOURS, dim=1, largest=False).values[:, -1].median())


def torch_composition(points, eps, min_points, block=2048):
    """The definition of include/pointops_amd.h for ONE cloud (P, 3) in plain torch: labels (P,), core (P,), clusters."""
    P = points.shape[0]
    r2 = torch.tensor(eps, dtype=torch.float32, device=points.device) ** 2
    adj = torch.empty((P, P), dtype=torch.bool, device=points.device)
    for a in range(0, P, block):
        d = points[a:a + block, None, :] - points[None, :, :]
        adj[a:a + block] = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] < r2
    core = adj.sum(1) >= min_points
    big = torch.iinfo(torch.int64).max
    idx = torch.arange(P, device=points.device)
    lab = torch.where(core, idx, torch.full_like(idx, big))
    while True:  # min-label propagation over the core graph, with pointer jumping, until stable
        m = torch.cat([torch.where(adj[a:a + block] & core[None, :], lab[None, :], big).min(1).values
                       for a in range(0, P, block)])
        new = torch.where(core, torch.minimum(m, lab), lab)
        new = torch.where(core, new[new.clamp(max=P - 1)], new)
        if torch.equal(new, lab):  # (a host read-back per sweep: the composition cannot know the diameter)
            break
        lab = new
    roots = torch.unique(lab[core])
    labels = torch.full((P,), -1, dtype=torch.int64, device=points.device)
    labels[core] = torch.searchsorted(roots, lab[core])
    for a in range(0, P, block):  # border points
        m = torch.where(adj[a:a + block] & core[None, :], labels[None, :], big).min(1).values
        take = ~core[a:a + block] & (m != big)
        labels[a:a + block] = torch.where(take, m, labels[a:a + block])
    return labels, core, roots.numel()


def with_debug(value, fn):
    def run():
        old = os.environ.get("POINTOPS_DEBUG")
        os.environ["POINTOPS_DEBUG"] = value
        try:
            return fn()
        finally:
            if old is None:
                del os.environ["POINTOPS_DEBUG"]
            else:
                os.environ["POINTOPS_DEBUG"] = old
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--shapes", default="all", choices=["all", "small"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cluster.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for N, P in (SHAPES[2:] if args.shapes == "small" else SHAPES):
        host = scene(N, P)
        points = torch.from_numpy(host).to(dev)
        eps = pick_eps(points)

        def fused():
            return cluster_dbscan(points, eps, MIN_POINTS)

        sol = fused()
        row = dict(N=N, P=P, eps=eps, min_points=MIN_POINTS, clusters=int(sol.num_clusters[0]),
                   core=int(sol.core_mask[0].sum()), noise=int((sol.labels[0] < 0).sum()))
        row["fused_ms"] = timeit(fused)
        row["fused_ns_per_point"] = row["fused_ms"] * 1e6 / (N * P)
        if not args.only_fused:
            if N * P * P <= 2 * 16384 * 16384:
                row["allpairs_ms"] = timeit(with_debug("cluster_grid=0", fused))
                other = with_debug("cluster_grid=0", fused)()
                row["allpairs_equal"] = bool(all(torch.equal(a, b) for a, b in zip(sol, other)))
            if (N, P) == TORCH_SHAPE:
                labels, core, num = torch_composition(points[0], eps, MIN_POINTS)
                assert torch.equal(labels, sol.labels[0]) and torch.equal(core, sol.core_mask[0]), "labels differ"
                assert num == int(sol.num_clusters[0])
                row["labels_equal"] = True
                row["torch_ms"] = timeit(lambda: torch_composition(points[0], eps, MIN_POINTS))
                row["speedup"] = row["torch_ms"] / row["fused_ms"]
            try:
                from sklearn.cluster import DBSCAN
            except ImportError:
                DBSCAN = None
            if DBSCAN is not None and P <= 65536:
                t0 = time.perf_counter()
                sk = DBSCAN(eps=eps, min_samples=MIN_POINTS).fit(host[0].astype(np.float64))
                row["sklearn_cpu_ms"] = (time.perf_counter() - t0) * 1e3 * N  # one cloud timed, N clouds meant
                row["sklearn_clusters"] = int(sk.labels_.max() + 1)
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del points, sol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
