#!/usr/bin/env python3
"""knn_features' search on the MI355X: the K <= 32 MFMA screen (POINTOPS_DEBUG=topk_screen=1, with topk_split=1 and 4
where K allows it) against the exact search on the same inputs -- `knn_points`, the parent's path for these bytes.  One
JSON line per (shape, D, K) into profiles/feature_topk_bench.jsonl (--out).  The default dispatch of
csrc/feature_topk.hip takes the screen, and picks S, only where this table has it faster than the exact search by more
than the spread; `default_is_screen` records what the default took.

Rows are unit-norm normal rows, queries and targets drawn independently, full lengths.  The outputs of every variant are
compared byte for byte with knn_points' before anything is timed.  The knobs are read at call time, so the variants run
in one process, in alternation, `--rounds` times; times are HIP-event times over `steps` consecutive calls (as many as
fit in about 50 ms, at most 20); the median is reported with the minimum and the maximum.  `uncertified_S*` is the share
of rows the screen sent to its exact fallback (from `stats`)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd import _C_feature_topk  # noqa: E402
from pytorch3d_pointops_amd.functions import knn_points  # noqa: E402

SHAPES = ((32, 1024), (16, 4096), (8, 65536))
DIMS = (32, 64, 128)
KS = (8, 16, 20, 32)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def under(knobs, fn):
    def run():
        os.environ["POINTOPS_DEBUG"] = knobs
        try:
            return fn()
        finally:
            os.environ.pop("POINTOPS_DEBUG", None)
    return run


def bench(N, P, D, K, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(1000 + N + D)
    f1, f2 = (torch.randn(N, P, D, generator=g, device=dev) for _ in range(2))
    f1, f2 = ((x / x.norm(dim=-1, keepdim=True)).contiguous() for x in (f1, f2))
    lengths = torch.full((N,), P, dtype=torch.int64, device=dev)
    search = lambda: _C_feature_topk.feature_topk(f1, f2, lengths, lengths, K)  # noqa: E731
    variants = {"exact": lambda: knn_points(f1, f2, lengths, lengths, K=K)}
    for S in ((1, 4) if K <= 16 else (4,)):
        variants[f"screen_S{S}"] = under(f"topk_screen=1,topk_split={S}", search)
    want = variants["exact"]()
    row = dict(N=N, P1=P, P2=P, D=D, K=K, rounds=rounds, default_is_screen=int(search()[2][0, 0]))
    for k, fn in variants.items():
        if k != "exact":
            idx, dists, stats = fn()
            assert torch.equal(idx, want.idx) and torch.equal(dists.view(torch.int32), want.dists.view(torch.int32)), k
            row[f"uncertified_{k[7:]}"] = round(float(stats[:, 2].sum()) / (N * P), 6)
    steps = {k: int(min(20, max(1, 50.0 / max(timed(fn, 1), 1e-3)))) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(rounds):  # in alternation: the variants share whatever else the machine is doing
        for k, fn in variants.items():
            times[k].append(timed(fn, steps[k]))
    for k, v in times.items():
        row[f"ms_{k}"] = round(float(np.median(v)), 4)
        row[f"ms_min_{k}"] = round(float(np.min(v)), 4)
        row[f"ms_max_{k}"] = round(float(np.max(v)), 4)
        if k != "exact":
            row[f"exact_over_{k}"] = round(row["ms_exact"] / row[f"ms_{k}"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "feature_topk_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--dims", default=",".join(str(d) for d in DIMS))
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feature_topk needs a GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    with open(args.out, "w") as f:
        for N, P in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
            for D in (int(d) for d in args.dims.split(",")):
                for K in (int(k) for k in args.ks.split(",")):
                    line = json.dumps(bench(N, P, D, K, args.rounds, dev))
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
