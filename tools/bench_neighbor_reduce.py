#!/usr/bin/env python3
"""neighbor_reduce on the MI355X against the parent's path for the same result: `knn_gather` followed by the torch
reduction over K (and its autograd backward).  One JSON line per (shape, K, C, pass) into
profiles/neighbor_reduce_bench.jsonl (--out).

The table is uniform random rows of the cloud itself (L = M = P, full lengths): no locality between the rows a query
gathers, which is what a search over unsorted points returns.  K = 3 is the weighted sum of knn_interpolate, the other K
the max of EdgeConv.  The two paths run in one process, in alternation, `--rounds` times; times are HIP-event times over
`steps` consecutive calls (as many as fit in about 50 ms, at most 20); the median is reported with the minimum and the
maximum.  `fwd` is the forward alone under no_grad, `fwd_bwd` forward + backward to grad_x (and grad_w when weighted).
Before anything is timed the outputs are compared (max: byte for byte; sum: 1e-5 relative to the largest magnitude).
    bytes_fwd        what the forward has to move: the gathered rows, idx (and weights), out (and arg)
    bytes_once       the same with every row of x counted once: what HBM has to deliver where the caches hold the re-reads
    old_error        the composition's scatter backward refused the shape (its launch error): that pass is not timed
    gbps_*           bytes_fwd over the forward time of either path -- the composition moves the (N, L, K, C) tensor twice
                     on top of that -- and hbm_fraction_* that rate over the 8 TB/s HBM peak; the rows of x are re-read
                     from the caches where x fits them, so this is a rate of useful bytes, not an HBM counter
    peak_mib_*       torch.cuda.max_memory_allocated over one call, above what was allocated before it
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd.functions import knn_gather, neighbor_reduce  # noqa: E402

SHAPES = ((8, 65536), (16, 131072), (2, 4096), (32, 1024))
KS = (3, 16, 20)
CS = (3, 64, 128)
HBM_PEAK = 8.0e12


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def bench(N, P, K, C, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(1000 + N + K + C)
    x = torch.randn(N, P, C, generator=g, device=dev).requires_grad_(True)
    idx = torch.randint(0, P, (N, P, K), generator=g, device=dev)
    w = torch.rand(N, P, K, generator=g, device=dev).requires_grad_(True) if K == 3 else None
    up = torch.randn(N, P, C, generator=g, device=dev)
    reduce = "sum" if K == 3 else "max"

    def new():
        return neighbor_reduce(x, idx, None, reduce, w)

    def old():
        rows = knn_gather(x, idx)
        return (rows * w[..., None]).sum(2) if w is not None else rows.max(2).values

    leaves = [x] + ([w] if w is not None else [])
    paths = {"new": new, "old": old}
    with torch.no_grad():
        a, b = new(), old()
    if reduce == "max":
        assert torch.equal(a, b), "max differs"
    else:
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), "sum differs"
    old_backward_error = None
    ga = torch.autograd.grad(new(), leaves, up)
    try:
        gb = torch.autograd.grad(old(), leaves, up)
    except RuntimeError as e:  # the composition's scatter backward refuses some shapes: reported, not timed
        old_backward_error, gb = str(e).splitlines()[0], ga
    worst = max(float((u - v).abs().max()) / float(v.abs().max()) for u, v in zip(ga, gb))
    if worst > 1e-5 and reduce == "max":
        # every upstream element of `max` goes to exactly one row of x: the path whose grad_x sums to the upstream's sum
        # is the one that scattered all of it (the composition's scatter has been seen to lose entries beyond 2^32)
        total, sums = float(up.double().sum()), [float(t[0].double().sum()) for t in (ga, gb)]
        assert abs(sums[0] - total) <= 1e-6 * float(up.double().abs().sum()), "the new path loses gradient"
        old_backward_error = f"grad_x of the composition sums to {sums[1]:.6g}, the upstream to {total:.6g} (new path: {sums[0]:.6g})"
    else:
        assert worst <= 1e-5, "gradient differs"
    del a, b, ga, gb
    table_out = K * 8 + (K * 4 if w is not None else 0) + C * 4 + (C if reduce == "max" else 0)
    bytes_fwd = N * P * (K * C * 4 + table_out)
    bytes_once = N * P * (C * 4 + table_out)  # x read once: what HBM has to deliver when the caches hold the re-reads
    rows_out = []
    for what in ("fwd", "fwd_bwd"):
        if what == "fwd":
            def run(fn):
                with torch.no_grad():
                    fn()
        else:
            def run(fn):
                torch.autograd.grad(fn(), leaves, up)
        calls = {k: (lambda fn=fn: run(fn)) for k, fn in paths.items()}
        row = dict(N=N, P=P, K=K, C=C, reduce=reduce, weighted=w is not None, what=what, rounds=rounds,
                   bytes_fwd=bytes_fwd, bytes_once=bytes_once)
        if what == "fwd_bwd" and old_backward_error is not None:
            row["old_error"] = old_backward_error
            del calls["old"]
        for k, fn in calls.items():
            row[f"peak_mib_{k}"] = peak_mib(fn)
        steps = {k: int(min(20, max(1, 50.0 / max(timed(fn, 1), 1e-3)))) for k, fn in calls.items()}
        times = {k: [] for k in calls}
        for _ in range(rounds):  # in alternation: the paths share whatever else the machine is doing
            for k, fn in calls.items():
                times[k].append(timed(fn, steps[k]))
        for k, v in times.items():
            row[f"ms_{k}"] = round(float(np.median(v)), 4)
            row[f"ms_min_{k}"] = round(float(np.min(v)), 4)
            row[f"ms_max_{k}"] = round(float(np.max(v)), 4)
            if what == "fwd":
                row[f"gbps_{k}"] = round(bytes_fwd / (row[f"ms_{k}"] * 1e-3) / 1e9, 1)
                row[f"hbm_fraction_{k}"] = round(bytes_fwd / (row[f"ms_{k}"] * 1e-3) / HBM_PEAK, 4)
        if "old" in calls:
            row["old_over_new"] = round(row["ms_old"] / row["ms_new"], 3)
        rows_out.append(row)
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "neighbor_reduce_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--cs", default=",".join(str(c) for c in CS))
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_neighbor_reduce needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    with open(args.out, "w") as f:
        for N, P in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
            for C in (int(c) for c in args.cs.split(",")):
                for K in (int(k) for k in args.ks.split(",")):
                    for row in bench(N, P, K, C, args.rounds, dev):
                        line = json.dumps(row)
                        print(line, flush=True)
                        f.write(line + "\n")
                        f.flush()
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
