#!/usr/bin/env python3
"""iss_keypoints: the fused path, cluster_dbscan at the same shape as a yardstick, and at one shape a plain-torch
composition of the same definition (one GPU).

    python tools/bench_iss.py [--out FILE] [--only-fused] [--shapes small]

Scenes: bench_cluster.py's (40 % uniform background, 60 % Gaussian blobs).  rs is the median distance to the 30th
nearest point (itself included) of 4096 sampled points of cloud 0, rn = 2/3 rs, the other parameters are the defaults.
Per shape (N clouds of P points) one JSON line with HIP-event times, the median of 5 calls after 2 warm-ups:
  fused_ms      iss_keypoints(points, salient_radius=rs, non_max_radius=rn): csrc/iss.hip, one native call
  cluster_ms    cluster_dbscan(points, rs, 10) on the same points in the same session: one full walk too (the union
                pass), plus its atomics, plus a counting walk and a border walk
  allpairs_ms   the fused path with POINTOPS_DEBUG=iss_grid=0, at the shapes where that takes milliseconds
  torch_ms      at 1 x 16384 only: the definition composed in torch -- a ball_query table with K = the largest support, a
                gather, the quantized offsets and their float64 covariance, torch.linalg.eigvalsh, the decision in
                float32, the suppression through a second table -- with the mask asserted equal to the fused one
                wherever the composition's eigenvalues round to the device's (for the row and all its rn-neighbours)
and the keypoint / salient counts of cloud 0.  --only-fused times the fused path alone (for a kernel trace).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_cluster import scene, timeit, with_debug  # noqa: E402
from pytorch3d_pointops_amd import _C_iss  # noqa: E402
from pytorch3d_pointops_amd.functions import ball_query, cluster_dbscan, iss_keypoints  # noqa: E402

SHAPES = [(8, 65536), (16, 131072), (2, 4096), (1, 16384)]  # (N, P)
TORCH_SHAPE = (1, 16384)
NEIGHBOURS = 30
G21 = G32 = 0.975
MIN_NEIGHBORS = 5


def pick_radius(points):
    """Median distance to the NEIGHBOURS-th nearest point (itself included) over 4096 sampled points of cloud 0."""
    p = points[0]
    q = p[torch.randperm(p.shape[0], device=p.device, generator=torch.Generator(p.device).manual_seed(1))[:4096]]
    return float(torch.cdist(q, p).topk(NEIGHBOURS, dim=1, largest=False).values[:, -1].median())


def iss_scale(rs):
    m, k = torch.frexp(torch.tensor(rs, dtype=torch.float32))
    return 2.0 ** (19 - (int(k) - 1 if float(m) == 0.5 else int(k)))


def torch_composition(points, rs, rn, K):
    """The definition of include/pointops_amd.h for a batch (N, P, 3) in plain torch ops (and this library's
    ball_query for the two tables) -> (mask, saliency, eigenvalues float32, the second table)."""
    s = iss_scale(rs)
    idx = ball_query(points, points, K=K, radius=rs, return_nn=False).idx  # (N, P, K), -1 padded
    hit = idx >= 0
    nb = torch.gather(points[:, None].expand(-1, points.shape[1], -1, -1), 2,
                      idx.clamp(min=0)[..., None].expand(-1, -1, -1, 3))  # (N, P, K, 3)
    q = torch.round((nb.double() - points.double()[:, :, None, :]) * s) * hit[..., None]  # (half to even)
    n = hit.sum(2).double().clamp(min=1)
    m = q.sum(2) / n[..., None]
    M2 = torch.einsum("npka,npkb->npab", q, q)  # float64 sums of integers below 2^53: exact
    C = (M2 / n[..., None, None] - m[..., :, None] * m[..., None, :]) * ((1.0 / s) * (1.0 / s))
    eig = torch.linalg.eigvalsh(C).float()
    l0, l1, l2 = eig.unbind(-1)
    ok = (l0 > 2.0 ** -20 * l2) & (l1 < torch.tensor(G21, device=eig.device) * l2) & \
         (l0 < torch.tensor(G32, device=eig.device) * l1)
    sal = torch.where(ok, l0, torch.full((), 0.0, device=eig.device))
    idx2 = ball_query(points, points, K=K, radius=rn, return_nn=False).idx  # (rn <= rs: K is enough)
    near = idx2 >= 0
    sj = torch.gather(sal[:, None].expand(-1, sal.shape[1], -1), 2, idx2.clamp(min=0))
    me = torch.arange(sal.shape[1], device=sal.device)[None, :, None]
    beats = near & ((sj > sal[..., None]) | ((sj == sal[..., None]) & (idx2 < me)))
    mask = (sal > 0) & (near.sum(2) >= MIN_NEIGHBORS) & ~beats.any(2)
    return mask, sal, eig, idx2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--shapes", default="all", choices=["all", "small"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iss.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    out = open(args.out, "w") if args.out else None
    for N, P in (SHAPES[2:] if args.shapes == "small" else SHAPES):
        points = torch.from_numpy(scene(N, P)).to(dev)
        rs = pick_radius(points)
        rn = rs * 2.0 / 3.0

        def fused():
            return iss_keypoints(points, salient_radius=rs, non_max_radius=rn, gamma_21=G21, gamma_32=G32,
                                 min_neighbors=MIN_NEIGHBORS)

        sol = fused()
        row = dict(N=N, P=P, salient_radius=rs, non_max_radius=rn, keypoints=int(sol.num_keypoints[0]),
                   salient=int((sol.saliency[0] > 0).sum()))
        row["fused_ms"] = timeit(fused)
        row["fused_ns_per_point"] = row["fused_ms"] * 1e6 / (N * P)
        if not args.only_fused:
            row["cluster_ms"] = timeit(lambda: cluster_dbscan(points, rs, 10))
            if N * P * P <= 2 * 16384 * 16384:
                row["allpairs_ms"] = timeit(with_debug("iss_grid=0", fused))
                other = with_debug("iss_grid=0", fused)()
                row["allpairs_equal"] = bool(all(torch.equal(a, b) for a, b in zip(sol, other)))
            if (N, P) == TORCH_SHAPE:
                moments = _C_iss.iss_keypoints(points, None, rs, rn, G21, G32, MIN_NEIGHBORS, want_moments=True)[3]
                K = int(moments[..., 0].max())  # the largest support: what a table needs to drop no neighbour
                mask, sal, eig, idx2 = torch_composition(points, rs, rn, K)
                same = (eig == sol.eigenvalues).all(-1)
                around = torch.gather(same[:, None].expand(-1, P, -1), 2, idx2.clamp(min=0)) | (idx2 < 0)
                settled = same & around.all(2)  # the row and all its rn-neighbours have the device's eigenvalues
                assert torch.equal(mask[settled], sol.mask[settled]), "masks differ where the eigenvalues agree"
                row.update(table_K=K, eigenvalues_equal=float(same.float().mean()),
                           rows_compared=float(settled.float().mean()), masks_equal=bool(torch.equal(mask, sol.mask)))
                row["torch_ms"] = timeit(lambda: torch_composition(points, rs, rn, K))
                row["speedup"] = row["torch_ms"] / row["fused_ms"]
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del points, sol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
