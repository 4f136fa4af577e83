#!/usr/bin/env python3
"""match_features on the MI355X: the search alone and the whole operator, screened on the matrix cores
(POINTOPS_DEBUG=match_screen=1) against the exact search (match_screen=0), which is the parent's path for the same
bytes -- `knn_points(K=2)`, the reverse `knn_points(K=1)` and the torch filters.  One JSON line per (shape, D) into
profiles/match_bench.jsonl (--out).  The default dispatch of csrc/feature_match.hip takes the screen only where this
table has it faster; `default_is_screen` records what the default took.  The split by kernel is not this tool's: run it
under `rocprofv3 --kernel-trace --stats` (profiles/match_kernel_stats.csv).  The rescoring is fused into the screen
kernel, so the trace shows norms, screen + rescoring, fallback and stats.

Rows are descriptor-like: three 11-bin histograms that sum to 100 at D = 33, unit-norm normal rows at D = 32 and 128;
queries and targets drawn independently, full lengths.  The knob is read at call time, so all four variants run in one
process, in alternation, `--rounds` times; times are HIP-event times over `steps` consecutive calls (as many as fit in
about 50 ms, at most 20); the median is reported with the minimum and the maximum.  `uncertified` is the share of rows
the screen sent to its exact fallback (from `stats`)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd import _C_match  # noqa: E402
from pytorch3d_pointops_amd.functions import match_features  # noqa: E402

SHAPES = ((2, 4096), (8, 4096), (1, 16384), (8, 65536), (16, 131072))
DIMS = (32, 33, 128)
FILTERS = dict(mutual=True, ratio=0.9, max_distance=None)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def rows(N, P, D, g, dev):
    if D == 33:
        x = torch.distributions.Gamma(torch.full((N, P, 3, 11), 0.5, device=dev), 1.0).sample()
        return (x / x.sum(-1, keepdim=True) * 100.0).reshape(N, P, 33).contiguous()
    x = torch.randn(N, P, D, generator=g, device=dev)
    return (x / x.norm(dim=-1, keepdim=True)).contiguous()


def under(mode, fn):
    def run():
        os.environ["POINTOPS_DEBUG"] = f"match_screen={mode}"
        try:
            return fn()
        finally:
            os.environ.pop("POINTOPS_DEBUG", None)
    return run


def bench(N, P, D, rounds, dev):
    torch.manual_seed(1000 + N + D)
    g = torch.Generator(device=dev).manual_seed(1000 + N + D)
    f1, f2 = rows(N, P, D, g, dev), rows(N, P, D, g, dev)
    lengths = torch.full((N,), P, dtype=torch.int64, device=dev)
    search = lambda: _C_match.feature_knn(f1, f2, lengths, lengths, 2)  # noqa: E731
    match = lambda: match_features(f1, f2, **FILTERS)  # noqa: E731
    variants = {"search_screen": under(1, search), "search_exact": under(0, search),
                "match_screen": under(1, match), "match_exact": under(0, match)}
    si, sd, stats = variants["search_screen"]()
    ei, ed, _ = variants["search_exact"]()
    assert torch.equal(si, ei) and torch.equal(sd.view(torch.int32), ed.view(torch.int32)), "the paths differ"
    a, b = variants["match_screen"](), variants["match_exact"]()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the operators differ"
    default_path = int(_C_match.feature_knn(f1, f2, lengths, lengths, 2)[2][0, 0])
    steps = {}
    for k, fn in variants.items():  # warm (done above), and size the timed window
        steps[k] = int(min(20, max(1, 50.0 / max(timed(fn, 1), 1e-3))))
    times = {k: [] for k in variants}
    for _ in range(rounds):  # in alternation: the variants share whatever else the machine is doing
        for k, fn in variants.items():
            times[k].append(timed(fn, steps[k]))
    row = dict(N=N, P1=P, P2=P, D=D, rounds=rounds, default_is_screen=default_path,
               uncertified=round(float(stats[:, 2].sum()) / (N * P), 6), matches=int(a.num_matches.sum()))
    for k, v in times.items():
        row[f"ms_{k}"] = round(float(np.median(v)), 4)
        row[f"ms_min_{k}"] = round(float(np.min(v)), 4)
        row[f"ms_max_{k}"] = round(float(np.max(v)), 4)
    row["search_exact_over_screen"] = round(row["ms_search_exact"] / row["ms_search_screen"], 3)
    row["match_exact_over_screen"] = round(row["ms_match_exact"] / row["ms_match_screen"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "match_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--dims", default=",".join(str(d) for d in DIMS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_match needs a GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    with open(args.out, "w") as f:
        for N, P in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
            for D in (int(d) for d in args.dims.split(",")):
                try:
                    line = json.dumps(bench(N, P, D, args.rounds, dev))
                except torch.cuda.OutOfMemoryError:
                    line = json.dumps(dict(N=N, P1=P, P2=P, D=D, skipped="out of memory"))
                    torch.cuda.empty_cache()
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
