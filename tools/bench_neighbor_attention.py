#!/usr/bin/env python3
"""neighbor_attention on the MI355X against the torch composition for the same result: `knn_gather` of k and of v,
einsum, softmax, einsum (and its autograd backward), and against `neighbor_reduce(sum)` of v on the same table as the
yardstick of a one-row-per-slot gather.  One JSON line per (shape, K, heads, D, pass) into
profiles/neighbor_attention_bench.jsonl (--out).

The table is uniform random rows of the cloud itself (L = M = P, full lengths): no locality between the rows a query
gathers.  The paths run in one process, in alternation, `--rounds` times; times are HIP-event times over `steps`
consecutive calls (as many as fit in about 50 ms, at most 20); the median is reported with the minimum and the maximum.
`fwd` is the forward alone under no_grad, `fwd_bwd` forward + backward to grad_q, grad_k and grad_v.  Before anything is
timed the outputs and the gradients of the two attention paths are compared (1e-5 relative to the largest magnitude).
    bytes_fwd        what the forward has to move: the gathered rows of k and v, idx, q, out
    old_error        the composition refused the shape (out of memory, or the launch error of its scatter backward):
                     that pass is not timed
    gbps_*           bytes_fwd over the forward time of either attention path, and hbm_fraction_* that rate over the 8 TB/s
                     HBM peak; the rows are re-read from the caches where k and v fit them, so this is a rate of useful
                     bytes, not an HBM counter
    new_over_reduce  the fused forward as a multiple of neighbor_reduce(sum) on v alone (attention moves two rows per slot)
    peak_mib_*       torch.cuda.max_memory_allocated over one call, above what was allocated before it
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd.functions import knn_gather, neighbor_attention, neighbor_reduce  # noqa: E402

SHAPES = ((8, 65536), (16, 131072), (2, 4096), (32, 1024))
HEADS = ((4, 16), (8, 32), (1, 64))
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


def bench(N, P, K, heads, D, rounds, dev):
    C = heads * D
    gen = torch.Generator(device=dev).manual_seed(1000 + N + K + C)
    q, k, v = (torch.randn(N, P, C, generator=gen, device=dev).requires_grad_(True) for _ in range(3))
    idx = torch.randint(0, P, (N, P, K), generator=gen, device=dev)
    up = torch.randn(N, P, C, generator=gen, device=dev)
    scale = D ** -0.5

    def new():
        return neighbor_attention(q, k, v, idx, None, heads)

    def old():
        kr = knn_gather(k, idx).view(N, P, K, heads, D)
        vr = knn_gather(v, idx).view(N, P, K, heads, D)
        w = torch.softmax(torch.einsum("nlhd,nlkhd->nlkh", q.view(N, P, heads, D), kr) * scale, dim=2)
        return torch.einsum("nlkh,nlkhd->nlhd", w, vr).reshape(N, P, C)

    def reduce():
        return neighbor_reduce(v, idx, None, "sum")

    leaves = [q, k, v]
    old_error = {}
    try:
        with torch.no_grad():
            a, b = new(), old()
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), "forward differs"
        del a, b
    except (RuntimeError, torch.OutOfMemoryError) as e:
        old_error["fwd"] = old_error["fwd_bwd"] = str(e).splitlines()[0]
    ga = torch.autograd.grad(new(), leaves, up)
    if not old_error:
        try:
            gb = torch.autograd.grad(old(), leaves, up)
            worst = max(float((s - t).abs().max()) / float(t.abs().max()) for s, t in zip(ga, gb))
            assert worst <= 1e-5, f"gradient differs: {worst:.3g}"
            del gb
        except (RuntimeError, torch.OutOfMemoryError) as e:
            old_error["fwd_bwd"] = str(e).splitlines()[0]
    del ga
    torch.cuda.empty_cache()
    bytes_fwd = N * P * (2 * K * C * 4 + K * 8 + 2 * C * 4)
    rows_out = []
    for what in ("fwd", "fwd_bwd"):
        if what == "fwd":
            def run(fn, _leaves):
                with torch.no_grad():
                    fn()
        else:
            def run(fn, leaves_):
                torch.autograd.grad(fn(), leaves_, up)
        calls = {"new": lambda: run(new, leaves), "old": lambda: run(old, leaves), "reduce": lambda: run(reduce, [v])}
        row = dict(N=N, P=P, K=K, heads=heads, D=D, C=C, what=what, rounds=rounds, bytes_fwd=bytes_fwd)
        if what in old_error:
            row["old_error"] = old_error[what]
            del calls["old"]
        for name, fn in calls.items():
            row[f"peak_mib_{name}"] = peak_mib(fn)
        steps = {name: int(min(20, max(1, 50.0 / max(timed(fn, 1), 1e-3)))) for name, fn in calls.items()}
        times = {name: [] for name in calls}
        for _ in range(rounds):  # in alternation: the paths share whatever else the machine is doing
            for name, fn in calls.items():
                times[name].append(timed(fn, steps[name]))
        for name, t in times.items():
            row[f"ms_{name}"] = round(float(np.median(t)), 4)
            row[f"ms_min_{name}"] = round(float(np.min(t)), 4)
            row[f"ms_max_{name}"] = round(float(np.max(t)), 4)
            if what == "fwd" and name != "reduce":
                row[f"gbps_{name}"] = round(bytes_fwd / (row[f"ms_{name}"] * 1e-3) / 1e9, 1)
                row[f"hbm_fraction_{name}"] = round(bytes_fwd / (row[f"ms_{name}"] * 1e-3) / HBM_PEAK, 4)
        if "old" in calls:
            row["old_over_new"] = round(row["ms_old"] / row["ms_new"], 3)
        row["new_over_reduce"] = round(row["ms_new"] / row["ms_reduce"], 3)
        rows_out.append(row)
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "neighbor_attention_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--heads", default=",".join(f"{h}x{d}" for h, d in HEADS))
    ap.add_argument("--k", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_neighbor_attention needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    with open(args.out, "w") as f:
        for N, P in (tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")):
            for heads, D in (tuple(int(x) for x in s.split("x")) for s in args.heads.split(",")):
                for row in bench(N, P, args.k, heads, D, args.rounds, dev):
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
