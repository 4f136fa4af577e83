#!/usr/bin/env python3
"""segment_plane: the fused path against a plain-torch composition of the same definition (one GPU).

    python tools/bench_plane.py [--out FILE] [--only-fused] [--shapes small] [--block 64]

Per shape (N clouds of P points, 40 % of them on one planted floor with noise of 0.1 thr, the rest in the unit cube; H
hypotheses, two refits) one JSON line with HIP-event times:
  fused_ms            segment_plane(points, ...): csrc/plane.hip, one native call
  fused_<variant>_ms  the same with the scoring kernel's variants (POINTOPS_DEBUG=plane_lds / plane_hpl): scalar path or
                      LDS tile; one or two hypotheses per lane, in alternating rounds of one process
  torch_ms            the composition on the SAME triples: gather the triples, the cross product and the validity test
                      in float64, the residuals of every hypothesis against every point in blocks of `--block`
                      hypotheses (an (N, block, P) tensor; all H at once is 8.6 GB at the large shape), counts, argmax,
                      and two refits through torch.linalg.eigh of the inliers' covariance with the accept rule as
                      torch.where
  residuals           N H P, and fused_ns_per_residual = fused_ms / residuals
and the agreement of the two paths (`best` equal, `inliers` equal, max |plane| difference).
--only-fused times the fused path alone (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd.functions import segment_plane  # noqa: E402

SHAPES = [(8, 65536, 1024), (16, 131072, 1024), (2, 4096, 256)]  # (N, P, H)
THR = 0.02
REFINE = 2
VARIANTS = {f"{path}_hpl{k}": f"plane_lds={lds},plane_hpl={k}" for path, lds in (("scalar", 0), ("lds", 1)) for k in (1, 2)}


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
    """points (N,P,3): 40 % of the rows on a planted plane per cloud (noise 0.1 thr), the rest uniform in the cube."""
    rng = np.random.default_rng(8900 + seed)
    X = rng.uniform(-0.5, 0.5, (N, P, 3))
    for n in range(N):
        nrm = rng.standard_normal(3)
        nrm /= np.linalg.norm(nrm)
        k = int(np.argmin(np.abs(nrm)))
        b1 = np.cross(nrm, np.eye(3)[k])
        b1 /= np.linalg.norm(b1)
        b2 = np.cross(nrm, b1)
        rows = rng.permutation(P)[:(2 * P) // 5]
        u, v = rng.uniform(-0.5, 0.5, len(rows)), rng.uniform(-0.5, 0.5, len(rows))
        s = rng.uniform(-0.1, 0.1, len(rows)) * THR
        X[n, rows] = rng.uniform(-0.1, 0.1, 3) + u[:, None] * b1 + v[:, None] * b2 + s[:, None] * nrm
    return X.astype(np.float32)


def orient(n, d):
    """The sign rule without an axis: the component of largest magnitude (lowest index among equals) is positive."""
    a = n.abs()
    k = torch.where(a[..., 1] > a[..., 0], 1, 0)
    k = torch.where(a[..., 2] > a.gather(-1, k[..., None])[..., 0], 2, k)
    flip = n.gather(-1, k[..., None])[..., 0] < 0
    return torch.where(flip[..., None], -n, n), torch.where(flip, -d, d)


def inlier_mask(planes, X, thr):
    """planes (N,h,4) float32 against X (N,P,3): (N,h,P) bool, in the definition's order (eager torch fuses nothing, so
    the counts are the kernels' to the bit; an einsum would be free to reorder and could move a row across thr)."""
    x, y, z = X[:, None, :, 0], X[:, None, :, 1], X[:, None, :, 2]
    r = ((x * planes[..., 0:1] + y * planes[..., 1:2]) + z * planes[..., 2:3]) + planes[..., 3:4]
    return r.abs() <= thr


def fit(X, mask):
    """Float64 least-squares planes (N,4) of the masked rows."""
    w = mask.to(torch.float64)[..., None]
    x = X.to(torch.float64)
    cnt = w.sum(1).clamp(min=1.0)
    m = (w * x).sum(1) / cnt
    q = (x - m[:, None]) * w
    cov = torch.einsum("npa,npb->nab", q, q) / cnt[..., None]
    _, vec = torch.linalg.eigh(cov)
    n = vec[..., 0]
    n, d = orient(n, -(n * m).sum(-1))
    return torch.cat([n, d[..., None]], -1).to(torch.float32)


def torch_composition(X, samples, block):
    """The definition of include/pointops_amd.h in batched torch on the given triples: (planes, best, mask)."""
    N, H, _ = samples.shape
    p = X.gather(1, samples.reshape(N, H * 3, 1).expand(-1, -1, 3)).view(N, H, 3, 3).to(torch.float64)
    e1, e2 = p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0]
    c = torch.linalg.cross(e1, e2)
    sq = (c * c).sum(-1)
    ok = sq > 1e-12 * (e1 * e1).sum(-1) * (e2 * e2).sum(-1)
    n = c / sq.sqrt()[..., None]
    n, d = orient(n, -(n * p[:, :, 0]).sum(-1))
    planes = torch.where(ok[..., None], torch.cat([n, d[..., None]], -1), torch.zeros((), dtype=n.dtype, device=n.device))
    planes = planes.to(torch.float32)
    counts = torch.cat([inlier_mask(planes[:, a:a + block], X, THR).sum(-1) for a in range(0, H, block)], 1)
    counts = torch.where(ok, counts, torch.full_like(counts, -1))
    best = counts.argmax(1)
    plane = planes[torch.arange(N, device=X.device), best]
    mask = inlier_mask(plane[:, None], X, THR)[:, 0]
    num = mask.sum(1)
    live = torch.ones_like(num, dtype=torch.bool)
    for _ in range(REFINE):
        pc = fit(X, mask)
        mc = inlier_mask(pc[:, None], X, THR)[:, 0]
        nc = mc.sum(1)
        live = live & (nc >= num)
        plane = torch.where(live[:, None], pc, plane)
        mask, num = torch.where(live[:, None], mc, mask), torch.where(live, nc, num)
    return plane, best, mask


def with_debug(value, fn):
    def run():
        old = os.environ.get("POINTOPS_DEBUG")
        os.environ["POINTOPS_DEBUG"] = value
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
    ap.add_argument("--block", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plane.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for N, P, H in (SHAPES[2:] if args.shapes == "small" else SHAPES):
        X = torch.from_numpy(scene(N, P)).to(dev)

        def fused(hyp=False):
            return segment_plane(X, distance_threshold=THR, num_hypotheses=H, refine_steps=REFINE, seed=1,
                                 return_hypotheses=hyp)

        row = dict(N=N, P=P, H=H, residuals=N * H * P)
        row["fused_ms"] = timeit(fused)
        row["fused_ns_per_residual"] = row["fused_ms"] * 1e6 / row["residuals"]
        if not args.only_fused:
            variants = {k: with_debug(v, fused) for k, v in VARIANTS.items()}
            rounds = {k: [] for k in variants}
            for _ in range(3):  # alternating rounds of one process
                for k, fn in variants.items():
                    rounds[k].append(timeit(fn, warmup=1, iters=3))
            for k, ts in rounds.items():
                row[f"fused_{k}_ms"] = float(np.median(ts))
            sol = fused(hyp=True)
            row["torch_ms"] = timeit(lambda: torch_composition(X, sol.samples, args.block), warmup=1, iters=3)
            row["speedup"] = row["torch_ms"] / row["fused_ms"]
            plane, best, mask = torch_composition(X, sol.samples, args.block)
            row["best_equal"] = bool(torch.equal(best, sol.best))
            row["inliers_equal"] = bool(torch.equal(mask, sol.inliers))
            row["num_inliers"] = sol.num_inliers.tolist()
            row["max_dplane"] = float((plane - sol.planes).abs().max())
            del sol, plane, best, mask
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
