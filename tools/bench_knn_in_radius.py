#!/usr/bin/env python3
"""knn_in_radius on the MI355X against the two searches beside it -- `knn_points` followed by the mask of the identity,
and `ball_query` with the same K and radius (another result: the first K in index order) -- one JSON line per
(shape, K, radius) into profiles/knn_in_radius_bench.jsonl (--out).

Uniform clouds in the unit cube, queries and targets drawn independently, full lengths.  The radius is swept in units of
the mean point spacing P^(-1/3): the cube a query walks holds about 27 (1.001 m)^3 target rows at m spacings, so the sweep
shows where the walk loses to the exact search -- the ratio a later exact-or-bounded rule would rest on.

Times are HIP-event times over `steps` consecutive calls (as many as fit in about 50 ms, at most 20), the three variants
timed in alternation `--rounds` times; the median is reported with the minimum and the maximum."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd.functions import ball_query, knn_in_radius, knn_points  # noqa: E402

SHAPES = ((8, 65536), (16, 131072), (2, 4096), (1, 16384))
KS = (1, 8, 16)
SPACINGS = (0.5, 1.0, 2.0, 4.0, 8.0)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def bench(N, P, K, m, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    p1 = torch.rand(N, P, 3, generator=g, device=dev)
    p2 = torch.rand(N, P, 3, generator=g, device=dev)
    radius = float(np.float32(m * P ** (-1.0 / 3.0)))
    r2 = float(np.float32(radius) * np.float32(radius))

    def masked():
        nn = knn_points(p1, p2, K=K)
        keep = nn.dists < r2
        return torch.where(keep, nn.idx, -1), torch.where(keep, nn.dists, 0.0), keep.sum(2)

    variants = {"knn_in_radius": lambda: knn_in_radius(p1, p2, K=K, radius=radius),
                "knn_points_mask": masked,
                "ball_query": lambda: ball_query(p1, p2, K=K, radius=radius, return_nn=False)}
    r = variants["knn_in_radius"]()
    i, d, c = masked()
    assert torch.equal(r.idx, i) and torch.equal(r.dists, d) and torch.equal(r.counts.long(), c)
    steps = {}
    for k, fn in variants.items():  # warm, and size the timed window
        fn()
        steps[k] = int(min(20, max(1, 50.0 / max(timed(fn, 1), 1e-3))))
    times = {k: [] for k in variants}
    for _ in range(rounds):  # in alternation: the variants share whatever else the machine is doing
        for k, fn in variants.items():
            times[k].append(timed(fn, steps[k]))
    row = dict(N=N, P1=P, P2=P, K=K, spacings=m, radius=radius, rounds=rounds,
               mean_count=round(float(r.counts.float().mean()), 3))
    for k, v in times.items():
        row[f"ms_{k}"] = round(float(np.median(v)), 4)
        row[f"ms_min_{k}"] = round(float(np.min(v)), 4)
        row[f"ms_max_{k}"] = round(float(np.max(v)), 4)
    row["knn_points_mask_over_knn_in_radius"] = round(row["ms_knn_points_mask"] / row["ms_knn_in_radius"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "knn_in_radius_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn_in_radius needs a GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    with open(args.out, "w") as f:
        for N, P in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
            for K in KS:
                for m in SPACINGS:
                    line = json.dumps(bench(N, P, K, m, args.rounds, dev))
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
