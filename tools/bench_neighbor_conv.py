#!/usr/bin/env python3
"""neighbor_conv on the MI355X against the torch composition of the same definition: `knn_gather`, einsum over the
slots, one matmul (and its autograd backward), and against one rocBLAS matmul of (rows, P Cin) x (P Cin, Cout) alone,
the floor of the matrix stage.  One JSON line per (shape, K, P, Cin, Cout, coeff, pass) into
profiles/neighbor_conv_bench.jsonl (--out).  `--dtype bfloat16|float16` times csrc/neighbor_conv16.hip instead (into
profiles/neighbor_conv16_bench.jsonl): `old` is then the torch composition of functions/neighbor_conv.py in that dtype (the
route these inputs took before the 16-bit kernels), `f32` the float32 kernels on the same values (where they take the
size), `gemm` the 16-bit matmul, and one Cin = Cout = 256 configuration is added; the paths are compared to 2^-4 of the
largest magnitude (the composition rounds to T after every slot; the tests hold the kernels to float64).  `--only-new`: the new path alone, forward + backward (for a rocprofv3 --kernel-trace --stats run).

The table is uniform random rows of the cloud itself (L = M = P points, full lengths): no locality between the rows a
query gathers.  The paths run in one process, in alternation, `--rounds` times; times are HIP-event times over `steps`
consecutive calls (as many as fit in about 50 ms, at most 20); the median is reported with the minimum and the maximum.
`fwd` is the forward alone under no_grad, `fwd_bwd` forward + backward to every leaf.  Before anything is timed the
outputs and the gradients of the two paths are compared (1e-4 relative to the largest magnitude).
    flop             2 rows P Cin Cout (the matrix stage) + 2 rows K P Cin with coeff (the gather stage)
    old_error        the composition refused the shape (out of memory, or the launch error of its scatter backward):
                     that pass is not timed
    tflops_new       flop over the fused forward time
    new_over_gemm    the fused forward as a multiple of the matmul alone
    peak_mib_*       torch.cuda.max_memory_allocated over one call, above what was allocated before it
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd import _C_neighbor_conv  # noqa: E402
from pytorch3d_pointops_amd.functions import knn_gather, neighbor_conv  # noqa: E402
from pytorch3d_pointops_amd.functions.neighbor_conv import _neighbor_conv_torch  # noqa: E402

from bench_neighbor_attention import peak_mib, timed  # noqa: E402

SHAPES = ((8, 65536), (16, 131072), (2, 4096), (32, 1024))
CONFIGS = ((16, 15, 64, 64, True), (16, 15, 128, 128, True), (27, 27, 32, 64, False))  # K, P, Cin, Cout, coeff
CONFIGS16 = CONFIGS + ((16, 15, 256, 256, True),)


def bench(N, L, K, P, Cin, Cout, with_coeff, rounds, dev, dtype=torch.float32, only_new=False):
    gen = torch.Generator(device=dev).manual_seed(1000 + N + K + Cin)
    x = torch.randn(N, L, Cin, generator=gen, device=dev).to(dtype).requires_grad_(True)
    weight = (torch.randn(P, Cin, Cout, generator=gen, device=dev) / (P * Cin) ** 0.5).to(dtype).requires_grad_(True)
    coeff = torch.rand(N, L, K, P, generator=gen, device=dev).to(dtype).requires_grad_(True) if with_coeff else None
    idx = torch.randint(0, L, (N, L, K), generator=gen, device=dev)
    up = torch.randn(N, L, Cout, generator=gen, device=dev).to(dtype)
    leaves = [t for t in (x, weight, coeff) if t is not None]
    half = dtype != torch.float32
    tol = 2.0 ** -4 if half else 1e-4  # (the composition rounds to T after every slot and scatters in T)

    def new():
        return neighbor_conv(x, idx, weight, None, coeff)

    if only_new:
        for _ in range(3):
            torch.autograd.grad(new(), leaves, up)
        torch.cuda.synchronize()
        return []

    def old():
        if half:
            return _neighbor_conv_torch(x, idx, weight, None, coeff)
        rows = knn_gather(x, idx)
        A = rows if coeff is None else torch.einsum("nlkp,nlkc->nlpc", coeff, rows)
        return A.reshape(N, L, P * Cin) @ weight.reshape(P * Cin, Cout)

    f32_leaves = [t.detach().float().requires_grad_(True) for t in leaves] if half else []
    f32_up = up.float() if half else None

    def f32():  # the float32 kernels on the same values
        return neighbor_conv(f32_leaves[0], idx, f32_leaves[1], None, f32_leaves[2] if with_coeff else None)

    old_error = {}
    try:
        with torch.no_grad():
            a, b = new(), old()
        assert float((a.float() - b.float()).abs().max()) <= tol * float(b.float().abs().max()), "forward differs"
        del a, b
    except (RuntimeError, torch.OutOfMemoryError) as e:
        old_error["fwd"] = old_error["fwd_bwd"] = str(e).splitlines()[0]
    ga = torch.autograd.grad(new(), leaves, up)
    if not old_error:
        try:
            gb = torch.autograd.grad(old(), leaves, up)
            worst = max(float((s.float() - t.float()).abs().max()) / float(t.float().abs().max()) for s, t in zip(ga, gb))
            assert worst <= tol, f"gradient differs: {worst:.3g}"
            del gb
        except (RuntimeError, torch.OutOfMemoryError) as e:
            old_error["fwd_bwd"] = str(e).splitlines()[0]
    del ga
    torch.cuda.empty_cache()
    flop = 2 * N * L * P * Cin * (Cout + (K if with_coeff else 0))
    rows_out = []
    for what in ("fwd", "fwd_bwd"):
        if what == "fwd":
            def run(fn):
                with torch.no_grad():
                    fn()
        else:
            def run(fn):
                torch.autograd.grad(fn(), leaves, up)
        calls = {"new": lambda: run(new), "old": lambda: run(old)}
        if half and _C_neighbor_conv.supported(N, L, L, K, P, Cin, Cout):
            if what == "fwd":
                calls["f32"] = lambda: run(f32)
            else:
                calls["f32"] = lambda: torch.autograd.grad(f32(), f32_leaves, f32_up)
        row = dict(N=N, L=L, K=K, P=P, Cin=Cin, Cout=Cout, coeff=with_coeff, what=what, rounds=rounds, flop=flop,
                   dtype=str(dtype).replace("torch.", ""))
        if what in old_error:
            row["old_error"] = old_error[what]
            del calls["old"]
        if what == "fwd":
            try:
                A2 = torch.randn(N * L, P * Cin, generator=gen, device=dev).to(dtype)
                W2 = weight.detach().reshape(P * Cin, Cout)
                calls["gemm"] = lambda: torch.matmul(A2, W2)
            except (RuntimeError, torch.OutOfMemoryError) as e:
                row["gemm_error"] = str(e).splitlines()[0]
        for name, fn in calls.items():
            if name != "gemm":
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
        if what == "fwd":
            row["tflops_new"] = round(flop / (row["ms_new"] * 1e-3) / 1e12, 2)
        if "old" in calls:
            row["old_over_new"] = round(row["ms_old"] / row["ms_new"], 3)
        if "f32" in calls:
            row["f32_over_new"] = round(row["ms_f32"] / row["ms_new"], 3)
        if "gemm" in calls:
            row["new_over_gemm"] = round(row["ms_new"] / row["ms_gemm"], 3)
            del A2
        rows_out.append(row)
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", default="float32", choices=("float32", "bfloat16", "float16"))
    ap.add_argument("--configs", default=None, help="indices into the configuration list, comma-separated")
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_neighbor_conv needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    dtype = getattr(torch, args.dtype)
    configs = CONFIGS if dtype == torch.float32 else CONFIGS16
    if args.configs:
        configs = [configs[int(i)] for i in args.configs.split(",")]
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                   "neighbor_conv_bench.jsonl" if dtype == torch.float32 else "neighbor_conv16_bench.jsonl")
    with open(out, "w") as f:
        for N, L in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
            for K, P, Cin, Cout, with_coeff in configs:
                for row in bench(N, L, K, P, Cin, Cout, with_coeff, args.rounds, dev, dtype, args.only_new):
                    line = json.dumps(row)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
