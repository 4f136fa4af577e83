#!/usr/bin/env python3
"""FPFH descriptors: the fused path against a plain-torch composition of the same definition (one GPU).

    python tools/bench_fpfh.py [--out FILE] [--only-fused] [--shapes small]

Per shape (B clouds of P uniform points with unit normals, K neighbours) one JSON line with HIP-event times:
  fused_search_ms   fpfh_features(points, normals, K=K): knn_points + both passes of csrc/fpfh.hip
  fused_ms          fpfh_features(points, normals, idx=idx): the two passes alone
  torch_ms          the composition on the same table: gathers into (B,P,K,3) tensors, atan2, three scatter_adds, a
                    (B,P,K,33) gather of SPFH rows and its weighted sum
  knn_ms            knn_points alone
  spfh_ms, fpfh_ms  each pass alone; spfh_lanes1_ms / spfh_lanes8_ms: pass 1 as one lane per point and as eight
                    lanes per point (POINTOPS_DEBUG=spfh_lanes=...), in alternating rounds of one process
and per pass the algorithmic bytes (the int64 table, one gathered row per slot, the point's own rows, the output) and
the fraction of the 8.0 TB/s HBM peak they were moved at.  `max_abs_diff` is fused against composition (values in
[0, 200]; bins differ where a feature sits on a bin edge).  --only-fused times the fused path alone (for a
rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd import _C_descriptors, synth  # noqa: E402
from pytorch3d_pointops_amd.functions import fpfh_features, knn_points  # noqa: E402

SHAPES = [(2, 4096, 16), (2, 4096, 50), (8, 65536, 16), (8, 65536, 50)]  # (B, P, K)
HBM_PEAK = 8.0e12  # bytes / s (datasheet)


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


def _sum3(a, b):
    return (a * b).sum(-1)


def torch_composition(points, normals, idx, lengths):
    """The definition of include/pointops_amd.h in elementwise torch: (fpfh, spfh)."""
    N, P, K = idx.shape
    rows = torch.arange(P, device=idx.device)[None, :, None]
    len_ = lengths[:, None, None]
    ok = (rows < len_) & (idx >= 0) & (idx < len_) & (idx != rows)
    j = torch.where(ok, idx, 0).reshape(N, P * K, 1)
    pj = points.gather(1, j.expand(-1, -1, 3)).view(N, P, K, 3)
    nj = normals.gather(1, j.expand(-1, -1, 3)).view(N, P, K, 3)
    ni = normals[:, :, None, :].expand_as(nj)
    dp = pj - points[:, :, None, :]
    d2 = _sum3(dp, dp)
    live = ok & (d2 > 0)
    d = d2.sqrt()
    a1, a2 = _sum3(ni, dp) / d, _sum3(nj, dp) / d
    swap = a1.abs() < a2.abs()
    sw = swap[..., None]
    ns, nt, dps = torch.where(sw, nj, ni), torch.where(sw, ni, nj), torch.where(sw, -dp, dp)
    f3 = torch.where(swap, -a2, a1)
    v = torch.cross(dps, ns, dim=-1)
    vn = _sum3(v, v).sqrt()
    counted = live & (vn > 0)
    v = v / vn[..., None]
    w = torch.cross(ns, v, dim=-1)
    f2 = _sum3(v, nt)
    f1 = torch.atan2(_sum3(w, nt), _sum3(ns, nt))
    c1 = float(np.float32(11.0 / (2.0 * math.pi)))
    b1 = torch.nan_to_num((f1 + math.pi) * c1).floor().clamp(0, 10).long()
    b2 = torch.nan_to_num((f2 + 1.0) * 5.5).floor().clamp(0, 10).long() + 11
    b3 = torch.nan_to_num((f3 + 1.0) * 5.5).floor().clamp(0, 10).long() + 22
    one = counted.to(points.dtype)
    hist = torch.zeros((N, P, 33), dtype=points.dtype, device=points.device)
    for b in (b1, b2, b3):
        hist.scatter_add_(2, b, one)
    m = counted.sum(-1).to(points.dtype)
    spfh = hist * torch.where(m > 0, 100.0 / m, torch.zeros_like(m))[..., None]
    rows33 = spfh.gather(1, j.expand(-1, -1, 33)).view(N, P, K, 33)
    weight = torch.where(live, 1.0 / d2, torch.zeros_like(d2))
    acc = (rows33 * weight[..., None]).sum(2).view(N, P, 3, 11)
    S = acc.sum(-1, keepdim=True)
    fpfh = torch.where(S > 0, acc * 100.0 / S, torch.zeros_like(acc)).view(N, P, 33) + spfh
    return fpfh, spfh


def pass_bytes(B, P, K):
    """Algorithmic bytes of the two passes as fpfh_features runs them (no pair-feature output)."""
    spfh = B * P * (8 * K + 24 * K + 24 + 132)          # table, neighbour point + normal, own point + normal, row out
    fpfh = B * P * (8 * K + 12 * K + 132 * K + 12 + 132 + 132)  # table, neighbour point, neighbour row, own, row out
    return spfh, fpfh


def with_lanes(lanes, fn):
    def run():
        old = os.environ.get("POINTOPS_DEBUG")
        os.environ["POINTOPS_DEBUG"] = f"spfh_lanes={lanes}"
        try:
            fn()
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
        raise SystemExit("bench_fpfh.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for B, P, K in (SHAPES[:2] if args.shapes == "small" else SHAPES):
        pts = torch.from_numpy(np.stack([synth.distribution("uniform", 1300 + b, P) for b in range(B)])).to(dev)
        nrm = torch.from_numpy(synth.unit_normals(1400, (B, P, 3))).to(dev)
        lengths = torch.full((B,), P, dtype=torch.int64, device=dev)
        row = dict(B=B, P=P, K=K)
        row["fused_search_ms"] = timeit(lambda: fpfh_features(pts, nrm, lengths, K=K))
        if not args.only_fused:
            idx = knn_points(pts, pts, lengths, lengths, K=K).idx
            spfh = _C_descriptors.spfh(pts, nrm, idx, lengths)[1]
            row["knn_ms"] = timeit(lambda: knn_points(pts, pts, lengths, lengths, K=K))
            row["fused_ms"] = timeit(lambda: fpfh_features(pts, nrm, lengths, idx=idx))
            row["spfh_ms"] = timeit(lambda: _C_descriptors.spfh(pts, nrm, idx, lengths))
            row["fpfh_ms"] = timeit(lambda: _C_descriptors.fpfh(pts, idx, lengths, spfh))
            variants = {lanes: with_lanes(lanes, lambda: _C_descriptors.spfh(pts, nrm, idx, lengths)) for lanes in (1, 8)}
            rounds = {lanes: [] for lanes in variants}
            for _ in range(3):  # alternating rounds of one process
                for lanes, fn in variants.items():
                    rounds[lanes].append(timeit(fn, warmup=1, iters=3))
            for lanes, ts in rounds.items():
                row[f"spfh_lanes{lanes}_ms"] = float(np.median(ts))
            row["torch_ms"] = timeit(lambda: torch_composition(pts, nrm, idx, lengths), warmup=1, iters=3)
            row["speedup"] = row["torch_ms"] / row["fused_ms"]
            sb, fb = pass_bytes(B, P, K)
            row.update(spfh_algo_bytes=sb, fpfh_algo_bytes=fb,
                       spfh_hbm_fraction=sb / (row["spfh_ms"] * 1e-3) / HBM_PEAK,
                       fpfh_hbm_fraction=fb / (row["fpfh_ms"] * 1e-3) / HBM_PEAK)
            got = fpfh_features(pts, nrm, lengths, idx=idx)
            want, _ = torch_composition(pts, nrm, idx, lengths)
            diff = (got - want).abs().amax(-1)
            row["max_abs_diff"] = float(diff.max())
            row["rows_above_1e-3"] = float((diff > 1e-3).float().mean())
            del got, want, diff, idx, spfh
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del pts, nrm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
