#!/usr/bin/env python3
"""neighbor_mlp_max on the MI355X against (a) the torch composition of the same definition (`_neighbor_mlp_max_torch`:
gather, add, relu, matmul, max over K, and its autograd backward), (b) one rocBLAS matmul of (N L K, C1) x (C1, C2)
alone, the floor of the matrix work, and (c) `neighbor_reduce(max)` on a pre-multiplied x (N, M, C2), the floor of the
gather.  One JSON line per (shape, C1, C2, pass) into profiles/neighbor_mlp_bench.jsonl (--out).  `--only-new`: the new
path alone, forward + backward (for a rocprofv3 --kernel-trace --stats run).

The table is uniform random rows of the cloud itself (L = M points, K = 16, full lengths): no locality between the rows
a query gathers.  The paths run in one process, in alternation, `--rounds` times, each warmed first; times are HIP-event
times over `steps` consecutive calls (as many as fit in about 50 ms, at most 20); the median is reported with the minimum
and the maximum.  `fwd` is the forward alone under no_grad, `fwd_bwd` forward + backward to x, center, weight and bias.
Before anything is timed the outputs of the two paths are compared (1e-4 relative to the largest magnitude), and the
gradients: the two paths round y differently, so a near-tie may select another slot, and at most a fraction 1e-5 C2 of the
elements of grad_x and grad_center may differ by more than that (grad_weight and grad_bias: 1e-2 of the largest).
    flop             2 N L K C1 C2 (the matrix work of the forward)
    old_error        the composition refused the shape (out of memory, or the launch error of its scatter backward):
                     that pass is not timed
    tflops_new       flop over the fused forward time
    new_over_gemm, new_over_reduce    the fused forward as a multiple of either floor
    peak_mib_*       torch.cuda.max_memory_allocated over one call, above what was allocated before it
`--dtype bfloat16|float16` times csrc/neighbor_mlp16.hip instead (into profiles/neighbor_mlp16_bench.jsonl): `old` is then
the composition in that dtype (the route these inputs took before the 16-bit kernels), `f32` the float32 kernels on the
same values, `gemm` one matmul in that dtype, and there is no `reduce`.  Before anything is timed the forward is compared
with the float32 kernels' and the composition's (2^-5 relative to the largest magnitude: h and out are rounded to the type); the gradients are
the tests' business.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd.functions import neighbor_mlp_max, neighbor_reduce  # noqa: E402
from pytorch3d_pointops_amd.functions.neighbor_mlp import _neighbor_mlp_max_torch  # noqa: E402

from bench_neighbor_attention import peak_mib, timed  # noqa: E402

SHAPES = ((8, 65536), (16, 131072), (2, 4096), (32, 1024))
CONFIGS = ((32, 64), (64, 64), (64, 128), (128, 128))  # C1, C2
K = 16


def bench(N, L, C1, C2, rounds, dev, only_new=False, dtype=torch.float32):
    gen = torch.Generator(device=dev).manual_seed(1000 + N + C1 + C2)
    half = dtype != torch.float32
    x = torch.randn(N, L, C1, generator=gen, device=dev).to(dtype).requires_grad_(True)
    center = torch.randn(N, L, C1, generator=gen, device=dev).to(dtype).requires_grad_(True)
    weight = (torch.randn(C1, C2, generator=gen, device=dev) / C1 ** 0.5).to(dtype).requires_grad_(True)
    bias = torch.randn(C2, generator=gen, device=dev).to(dtype).requires_grad_(True)
    idx = torch.randint(0, L, (N, L, K), generator=gen, device=dev)
    up = torch.randn(N, L, C2, generator=gen, device=dev).to(dtype)
    leaves = [x, center, weight, bias]
    leaves32 = [t.detach().float().requires_grad_(True) for t in leaves] if half else None

    def new():
        return neighbor_mlp_max(x, idx, weight, bias, center)

    if only_new:
        for _ in range(3):
            torch.autograd.grad(new(), leaves, up)
        torch.cuda.synchronize()
        return []

    def old():
        return _neighbor_mlp_max_torch(x, idx, weight, bias, center, None, True)[0]

    def f32():
        return neighbor_mlp_max(leaves32[0], idx, leaves32[2], leaves32[3], leaves32[1])

    old_error = {}
    if half:
        with torch.no_grad():
            a, b = new().float(), f32()
        assert float((a - b).abs().max()) <= 2.0 ** -5 * float(b.abs().max()), "forward differs from the float32 kernels"
        del a, b
    try:
        with torch.no_grad():
            a, b = new().float(), old().float()
        assert float((a - b).abs().max()) <= (2.0 ** -5 if half else 1e-4) * float(b.abs().max()), "forward differs"
        del a, b
    except (RuntimeError, torch.OutOfMemoryError) as e:
        old_error["fwd"] = old_error["fwd_bwd"] = str(e).splitlines()[0]
    ga = torch.autograd.grad(new(), leaves, up)
    if half and not old_error:
        try:
            torch.autograd.grad(old(), leaves, up)
        except (RuntimeError, torch.OutOfMemoryError) as e:
            old_error["fwd_bwd"] = str(e).splitlines()[0]
    elif not old_error:
        try:
            gb = torch.autograd.grad(old(), leaves, up)
            # (the two paths round y differently, so a near-tie may pick another slot: the top two of K = 16 values of
            # unit spread lie within a few 1e-6 of each other for a few in 1e6 (row, column) pairs, and one such column
            # moves the whole row of grad_center and two rows of grad_x: such elements are counted, 1e-5 C2 allowed)
            worst = max(float(((s - t).abs() > 1e-4 * t.abs().max()).float().mean()) for s, t in zip(ga[:2], gb[:2]))
            assert worst <= 1e-5 * C2, f"gradient differs in a fraction {worst:.3g} of the elements"
            worst = max(float((s - t).abs().max()) / float(t.abs().max()) for s, t in zip(ga[2:], gb[2:]))
            # (sums of N L K signed terms in fp32 on either side: chains of ~1500 roundings of partial sums that are
            # sqrt(N L) times the result's size, about 2e-3 of it at 2^19 rows; the tests hold the kernels to float64)
            assert worst <= 1e-2, f"gradient of weight or bias differs: {worst:.3g}"
            del gb
        except (RuntimeError, torch.OutOfMemoryError) as e:
            old_error["fwd_bwd"] = str(e).splitlines()[0]
    del ga
    torch.cuda.empty_cache()
    flop = 2 * N * L * K * C1 * C2
    rows_out = []
    for what in ("fwd", "fwd_bwd"):
        if what == "fwd":
            def run(fn):
                with torch.no_grad():
                    fn()
        else:
            def run(fn):
                torch.autograd.grad(fn(), leaves32 if fn is f32 else leaves, up.float() if fn is f32 else up)
        calls = {"new": lambda: run(new), "old": lambda: run(old)}
        if half:
            calls["f32"] = lambda: run(f32)
        row = dict(N=N, L=L, K=K, C1=C1, C2=C2, what=what, rounds=rounds, flop=flop,
                   dtype=str(dtype).replace("torch.", ""))
        if what in old_error:
            row["old_error"] = old_error[what]
            del calls["old"]
        if what == "fwd":
            if not half:
                xw = torch.randn(N, L, C2, generator=gen, device=dev)
                calls["reduce"] = lambda: neighbor_reduce(xw, idx, None, "max")
            try:
                A2 = torch.randn(N * L * K, C1, generator=gen, device=dev).to(dtype)
                W2 = weight.detach()
                calls["gemm"] = lambda: torch.matmul(A2, W2)
            except (RuntimeError, torch.OutOfMemoryError) as e:
                row["gemm_error"] = str(e).splitlines()[0]
        for name, fn in calls.items():
            if name in ("new", "old", "f32"):
                row[f"peak_mib_{name}"] = peak_mib(fn)
        steps = {name: int(min(20, max(1, 50.0 / max(timed(fn, 1), 1e-3)))) for name, fn in calls.items()}  # (warms too)
        times = {name: [] for name in calls}
        for _ in range(rounds):  # in alternation: the paths share whatever else the machine is doing
            for name, fn in calls.items():
                times[name].append(timed(fn, steps[name]))
        for name, t in times.items():
            row[f"ms_{name}"] = round(float(np.median(t)), 4)
            row[f"ms_min_{name}"] = round(float(np.min(t)), 4)
            row[f"ms_max_{name}"] = round(float(np.max(t)), 4)
        if what == "fwd":
            row["tflops_new"] = round(flop / (row["ms_new"] * 1e-3) / 1e12, 2)
            if "reduce" in calls:
                row["new_over_reduce"] = round(row["ms_new"] / row["ms_reduce"], 3)
        if "old" in calls:
            row["old_over_new"] = round(row["ms_old"] / row["ms_new"], 3)
        if "f32" in calls:
            row["f32_over_new"] = round(row["ms_f32"] / row["ms_new"], 3)
        if "gemm" in calls:
            row["new_over_gemm"] = round(row["ms_new"] / row["ms_gemm"], 3)
            del A2
        rows_out.append(row)
    return rows_out


CONFIGS2 = ((64, 64, 128), (128, 128, 256), (64, 64, 64))  # C1, C2, C3


def bench2(N, L, C1, C2, C3, rounds, dev, only_new, dtype):
    """--layers 2: `new` the fused two-layer path, `old` the torch composition in the same dtype, `parent` the best route
    without weight2 (torch ops up to the hidden pre-activation as an (N, L K, C2) tensor, then neighbor_mlp_max over an
    identity table), `gemm` the two matmuls of the edge matrix.  flop = 2 N L K (C1 C2 + C2 C3)."""
    gen = torch.Generator(device=dev).manual_seed(2000 + N + C1 + C3)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=gen, device=dev) * scale).to(dtype).requires_grad_(True)  # noqa: E731
    x, center, weight, bias = rnd(N, L, C1), rnd(N, L, C1), rnd(C1, C2, scale=C1 ** -0.5), rnd(C2)
    weight2, bias2 = rnd(C2, C3, scale=C2 ** -0.5), rnd(C3)
    idx = torch.randint(0, L, (N, L, K), generator=gen, device=dev)
    own = torch.arange(L * K, device=dev).reshape(1, L, K).expand(N, L, K).contiguous()
    up = torch.randn(N, L, C3, generator=gen, device=dev).to(dtype)
    leaves = [x, center, weight, bias, weight2, bias2]

    def new():
        return neighbor_mlp_max(x, idx, weight, bias, center, weight2=weight2, bias2=bias2)

    def old():
        return _neighbor_mlp_max_torch(x, idx, weight, bias, center, None, True, weight2, bias2)[0]

    def parent():
        a = x.gather(1, idx.reshape(N, L * K, 1).expand(-1, -1, C1)).reshape(N, L, K, C1) + center[:, :, None, :]
        z = (torch.relu(a) @ weight + bias).reshape(N, L * K, C2)
        return neighbor_mlp_max(z, own, weight2, bias2)

    if only_new:
        for _ in range(3):
            torch.autograd.grad(new(), leaves, up)
        torch.cuda.synchronize()
        return []
    rows_out, flop = [], 2 * N * L * K * (C1 * C2 + C2 * C3)
    for what in ("fwd", "fwd_bwd"):
        if what == "fwd":
            def run(fn):
                with torch.no_grad():
                    return fn()
        else:
            def run(fn):
                return torch.autograd.grad(fn(), leaves, up)
        calls = {"new": lambda: run(new), "old": lambda: run(old), "parent": lambda: run(parent)}
        row = dict(N=N, L=L, K=K, C1=C1, C2=C2, C3=C3, what=what, rounds=rounds, flop=flop, layers=2,
                   dtype=str(dtype).replace("torch.", ""))
        for name in ("old", "parent"):  # a path that cannot hold its edge tensors is recorded, not timed
            try:
                got = calls[name]()
                if what == "fwd":
                    ref = calls["new"]().float()
                    assert float((got.float() - ref).abs().max()) <= 2.0 ** -4 * float(ref.abs().max()), name + " differs"
                    del ref
                del got
            except (RuntimeError, torch.OutOfMemoryError) as e:
                row[f"{name}_error"] = str(e).splitlines()[0]
                del calls[name]
            torch.cuda.empty_cache()
        if what == "fwd":
            try:
                A, W1, W2 = torch.randn(N * L * K, C1, generator=gen, device=dev).to(dtype), weight.detach(), weight2.detach()
                calls["gemm"] = lambda: torch.matmul(torch.matmul(A, W1), W2)
            except (RuntimeError, torch.OutOfMemoryError) as e:
                row["gemm_error"] = str(e).splitlines()[0]
        for name, fn in calls.items():
            if name != "gemm":
                row[f"peak_mib_{name}"] = peak_mib(fn)
        steps = {name: int(min(20, max(1, 50.0 / max(timed(fn, 1), 1e-3)))) for name, fn in calls.items()}  # (warms too)
        times = {name: [] for name in calls}
        for _ in range(rounds):
            for name, fn in calls.items():
                times[name].append(timed(fn, steps[name]))
        for name, t in times.items():
            row[f"ms_{name}"] = round(float(np.median(t)), 4)
            row[f"ms_min_{name}"] = round(float(np.min(t)), 4)
            row[f"ms_max_{name}"] = round(float(np.max(t)), 4)
            if name != "new":
                row[f"{'new_over' if name == 'gemm' else name + '_over'}_{'gemm' if name == 'gemm' else 'new'}"] = round(
                    row["ms_new"] / row[f"ms_{name}"] if name == "gemm" else row[f"ms_{name}"] / row["ms_new"], 3)
        if what == "fwd":
            row["tflops_new"] = round(flop / (row["ms_new"] * 1e-3) / 1e12, 2)
        calls.clear()
        rows_out.append(row)
        torch.cuda.empty_cache()
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=1, choices=(1, 2),
                    help="2: the weight2 form (16-bit dtypes), into profiles/neighbor_mlp2_bench.jsonl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", default=None, help="indices into CONFIGS, comma-separated")
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--dtype", default="float32", choices=("float32", "bfloat16", "float16"))
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least 3 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_neighbor_mlp needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    dtype = getattr(torch, args.dtype)
    all_configs = CONFIGS if dtype == torch.float32 else CONFIGS + ((256, 256),)  # (the 16-bit kernels go to 256)
    configs = [all_configs[int(i)] for i in args.configs.split(",")] if args.configs else all_configs
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.layers == 2:
        if dtype == torch.float32:
            raise SystemExit("--layers 2 times the 16-bit kernels: give --dtype bfloat16 or float16")
        configs = [CONFIGS2[int(i)] for i in args.configs.split(",")] if args.configs else CONFIGS2
        out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                       "neighbor_mlp2_bench.jsonl")
        with open(os.devnull if args.only_new else out, "w") as f:
            for N, L in shapes:
                for cfg in configs:
                    for row in bench2(N, L, *cfg, args.rounds, dev, args.only_new, dtype):
                        print(json.dumps(row), flush=True)
                        f.write(json.dumps(row) + "\n")
                        f.flush()
        return
    if args.only_new:  # nothing is measured: no file is opened
        for N, L in shapes:
            for C1, C2 in configs:
                bench(N, L, C1, C2, args.rounds, dev, only_new=True, dtype=dtype)
        return
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                   "neighbor_mlp_bench.jsonl" if dtype == torch.float32 else "neighbor_mlp16_bench.jsonl")
    with open(out, "w") as f:
        for N, L in shapes:
            for C1, C2 in configs:
                for row in bench(N, L, C1, C2, args.rounds, dev, dtype=dtype):
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
