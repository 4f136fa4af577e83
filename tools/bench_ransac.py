#!/usr/bin/env python3
"""ransac_alignment: the fused path against a plain-torch composition of the same definition (one GPU).

    python tools/bench_ransac.py [--out FILE] [--only-fused] [--shapes small] [--block 512]

Per shape (N clouds of P1 rows of which C carry a match, 20 % of those under one planted rigid motion with noise of
0.2 thr, the rest matched to random points; H hypotheses, two refinement steps) one JSON line with HIP-event times:
  fused_ms          ransac_alignment(X, Y, corr, ...): csrc/ransac.hip, one native call
  fused_lds_ms      the same with the scoring kernel reading its records from an LDS tile
                    (POINTOPS_DEBUG=ransac_lds=1), in alternating rounds of one process with fused_scalar_ms
  torch_ms          the composition on the SAME triples: gather the triples, a batched `_alignment_torch` (an (N H)
                    batched torch.linalg.svd), the edge test, the residuals of every hypothesis against every matched
                    row in blocks of `--block` hypotheses (an (N, block, C, 3) tensor; all H at once is 26 GB at the
                    large shape), counts, argmax, and two weighted refits with the accept rule as torch.where.  The
                    composition is handed the C matched rows already compacted (not timed): it never sees padding.
  residuals         N H C, and fused_ns_per_residual = fused_ms / residuals
and the agreement of the two paths (`best` equal, `num_inliers` equal, max |R| and |T| difference).
--only-fused times the fused path alone (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd.functions import ransac_alignment  # noqa: E402
from pytorch3d_pointops_amd.functions.points_alignment import _alignment_torch  # noqa: E402

SHAPES = [(8, 65536, 8192, 4096), (8, 65536, 65536, 4096), (2, 1024, 1024, 1024)]  # (N, P1, C, H)
THR = 0.02
RATIO = 0.9
REFINE = 2


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


def scene(N, P1, C, seed=0):
    """X (N,P1,3), Y (N,P1,3), corr (N,P1) with C matched rows per cloud (a random subset), 20 % of them planted."""
    rng = np.random.default_rng(8800 + seed)
    X = rng.uniform(0, 1, (N, P1, 3)).astype(np.float32)
    Y = rng.uniform(-0.5, 1.5, (N, P1, 3)).astype(np.float32)
    corr = np.full((N, P1), -1, np.int64)
    for n in range(N):
        rows = np.sort(rng.permutation(P1)[:C])
        corr[n, rows] = rng.permutation(P1)[:C]
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        inl = rows[rng.permutation(C)[:C // 5]]
        noise = rng.standard_normal((len(inl), 3))
        noise *= 0.2 * THR * rng.uniform(0, 1, (len(inl), 1)) / np.linalg.norm(noise, axis=1, keepdims=True)
        Y[n, corr[n, inl]] = (X[n, inl].astype(np.float64) @ q + rng.uniform(-1, 1, 3) + noise).astype(np.float32)
    return X, Y, corr


def residual_counts(A, T, Xv, Yv, thr2):
    """A (N,h,3,3), T (N,h,3) against the matched rows Xv, Yv (N,C,3): inlier mask (N,h,C)."""
    Xt = torch.einsum("ncj,nhjk->nhck", Xv, A) + T[:, :, None, :]
    return ((Xt - Yv[:, None]) ** 2).sum(-1) <= thr2


def torch_composition(X, Y, corr, Xv, Yv, samples, block):
    """The definition of include/pointops_amd.h in batched torch on the given triples: (R, T, s, best, num_inliers)."""
    N, H, _ = samples.shape
    thr2 = THR * THR
    rows = samples.reshape(N, H * 3, 1)
    x3 = X.gather(1, rows.expand(-1, -1, 3)).view(N * H, 3, 3)
    y3 = Y.gather(1, corr.gather(1, rows[..., 0])[..., None].expand(-1, -1, 3)).view(N * H, 3, 3)
    ok = torch.ones(N * H, dtype=torch.bool, device=X.device)
    q = RATIO * RATIO
    for a, b in ((0, 1), (0, 2), (1, 2)):
        lx, ly = ((x3[:, a] - x3[:, b]) ** 2).sum(-1), ((y3[:, a] - y3[:, b]) ** 2).sum(-1)
        ok &= (lx >= q * ly) & (ly >= q * lx)
    R, T, s, _ = _alignment_torch(x3, y3, torch.ones_like(x3[..., 0]), False, False, 1e-9)
    A, T = (s[:, None, None] * R).view(N, H, 3, 3), T.view(N, H, 3)
    counts = torch.cat([residual_counts(A[:, a:a + block], T[:, a:a + block], Xv, Yv, thr2).sum(-1)
                        for a in range(0, H, block)], 1)
    counts = torch.where(ok.view(N, H), counts, torch.full_like(counts, -1))
    best = counts.argmax(1)
    n = torch.arange(N, device=X.device)
    R, T, s = R.view(N, H, 3, 3)[n, best], T[n, best], s.view(N, H)[n, best]
    mask = residual_counts((s[:, None, None] * R)[:, None], T[:, None], Xv, Yv, thr2)[:, 0]
    num = mask.sum(1)
    live = torch.ones_like(num, dtype=torch.bool)
    for _ in range(REFINE):
        Rc, Tc, sc, _ = _alignment_torch(Xv, Yv, mask.to(Xv.dtype), False, False, 1e-9)
        mc = residual_counts((sc[:, None, None] * Rc)[:, None], Tc[:, None], Xv, Yv, thr2)[:, 0]
        nc = mc.sum(1)
        live = live & (nc >= num)
        R, T, s = torch.where(live[:, None, None], Rc, R), torch.where(live[:, None], Tc, T), torch.where(live, sc, s)
        mask, num = torch.where(live[:, None], mc, mask), torch.where(live, nc, num)
    return R, T, s, best, num


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
    ap.add_argument("--block", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ransac.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for N, P1, C, H in (SHAPES[2:] if args.shapes == "small" else SHAPES):
        X, Y, corr = (torch.from_numpy(a).to(dev) for a in scene(N, P1, C))

        def fused(hyp=False):
            return ransac_alignment(X, Y, corr, inlier_threshold=THR, num_hypotheses=H, edge_length_ratio=RATIO,
                                    refine_steps=REFINE, seed=1, return_hypotheses=hyp)

        row = dict(N=N, P1=P1, C=C, H=H, residuals=N * H * C)
        row["fused_ms"] = timeit(fused)
        row["fused_ns_per_residual"] = row["fused_ms"] * 1e6 / row["residuals"]
        if not args.only_fused:
            variants = {"scalar": with_debug("ransac_lds=0", fused), "lds": with_debug("ransac_lds=1", fused)}
            rounds = {k: [] for k in variants}
            for _ in range(3):  # alternating rounds of one process
                for k, fn in variants.items():
                    rounds[k].append(timeit(fn, warmup=1, iters=3))
            for k, ts in rounds.items():
                row[f"fused_{k}_ms"] = float(np.median(ts))
            sol = fused(hyp=True)
            keep = corr >= 0  # C per cloud: the compacted rows of the composition (not timed)
            Xv = X[keep].view(N, C, 3)
            Yv = Y.gather(1, corr.clamp(min=0)[..., None].expand(-1, -1, 3))[keep].view(N, C, 3)
            row["torch_ms"] = timeit(lambda: torch_composition(X, Y, corr, Xv, Yv, sol.samples, args.block),
                                     warmup=1, iters=3)
            row["speedup"] = row["torch_ms"] / row["fused_ms"]
            R, T, s, best, num = torch_composition(X, Y, corr, Xv, Yv, sol.samples, args.block)
            row["best_equal"] = bool(torch.equal(best, sol.best))
            row["num_inliers_equal"] = bool(torch.equal(num, sol.num_inliers))
            row["num_inliers"] = sol.num_inliers.tolist()
            row["max_dR"] = float((R - sol.RTs.R).abs().max())
            row["max_dT"] = float((T - sol.RTs.T).abs().max())
            del Xv, Yv, sol, R, T, s, best, num
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del X, Y, corr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
