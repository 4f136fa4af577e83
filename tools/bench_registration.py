#!/usr/bin/env python3
"""registration_icp on the MI355X: per-step time of both estimations against the step of iterative_closest_point and
against the torch composition of the same definition, and iterations / total time to freeze -- one JSON line per
shape into profiles/registration_bench.jsonl (--out).

Two scenes (--scenes).  "surface" is the one of tests/registration_ref.py on the GPU: the target is P points on
z = 0.2 sin 3x cos 2y over [-1, 1]^2, the source a moved subset of 3/4 P of its rows plus 1/4 P rows of clutter 1.5 above
the surface (partial overlap); the motion is 0.12 rad with |t| ~ 0.035, the threshold 0.08.  "uniform" is the kind of
cloud the search's own figures were taken on: uniform points in a cube, full overlap, a small motion.

Step times are HIP-event times over `--steps` consecutive steps on one state (the grid over the target is built by an
untimed first step), thresholds at -1 so that no cloud freezes and every step does all its work; the four variants are
timed in alternation, `--rounds` times, and the median is reported with the minimum.  Totals are host-clock times around
one whole call that ends in a synchronise, after one untimed call at the same shape."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch3d_pointops_amd import _C, _C_registration  # noqa: E402
from pytorch3d_pointops_amd.functions import (iterative_closest_point, knn_gather, knn_points,  # noqa: E402
                                              registration_icp)

R_MAX = 0.08
SHAPES = ((8, 65536), (16, 131072), (2, 4096), (1, 16384))


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K).T


def uniform_scene(N, P, seed, dev):
    """The clouds the README's search figures were taken on: P uniform points in [-1, 1]^3 as the target, all of its
    rows, shuffled and moved by 0.01 rad and |t| ~ 0.009, as the source; unit normals in random directions."""
    g = torch.Generator(device=dev).manual_seed(seed)
    Y = torch.rand(N, P, 3, generator=g, device=dev, dtype=torch.float64) * 2 - 1
    nr = torch.randn(N, P, 3, generator=g, device=dev, dtype=torch.float64)
    nr = nr / nr.norm(dim=2, keepdim=True)
    rows = torch.stack([torch.randperm(P, generator=g, device=dev) for _ in range(N)])
    R = torch.from_numpy(rotation([0.3, -0.5, 0.8], 0.01)).to(dev)
    T = torch.tensor([0.005, -0.005, 0.005], dtype=torch.float64, device=dev)
    X = (torch.gather(Y, 1, rows[..., None].expand(-1, -1, 3)) - T) @ R.T
    return X.float().contiguous(), Y.float().contiguous(), nr.float().contiguous(), R, T


def scene(N, P, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, device=dev, dtype=torch.float64) * 2 - 1  # noqa: E731
    surf = lambda x, y: 0.2 * torch.sin(3 * x) * torch.cos(2 * y)  # noqa: E731
    xy = u(N, P, 2)
    Y = torch.cat([xy, surf(xy[..., 0], xy[..., 1])[..., None]], 2)
    nr = torch.stack([-0.6 * torch.cos(3 * xy[..., 0]) * torch.cos(2 * xy[..., 1]),
                      0.4 * torch.sin(3 * xy[..., 0]) * torch.sin(2 * xy[..., 1]), torch.ones_like(xy[..., 0])], 2)
    nr = nr / nr.norm(dim=2, keepdim=True)
    over = P - P // 4
    rows = torch.stack([torch.randperm(P, generator=g, device=dev)[:over] for _ in range(N)])
    moved = torch.gather(Y, 1, rows[..., None].expand(-1, -1, 3))
    cxy = u(N, P - over, 2)
    clutter = torch.cat([cxy, surf(cxy[..., 0], cxy[..., 1])[..., None] + 1.5], 2)
    moved = torch.cat([moved, clutter], 1)
    moved = torch.gather(moved, 1, torch.stack([torch.randperm(P, generator=g, device=dev) for _ in range(N)])[
        ..., None].expand(-1, -1, 3))
    R = torch.from_numpy(rotation([0.3, -0.5, 0.8], 0.12)).to(dev)
    T = torch.tensor([0.02, -0.02, 0.02], dtype=torch.float64, device=dev)
    X = (moved - T) @ R.T
    return X.float().contiguous(), Y.float().contiguous(), nr.float().contiguous(), R, T


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def torch_step(Xt, Y, nr, lengths, r2):
    """One point-to-plane update composed from the package's search and torch: knn_points, knn_gather, mask, einsum
    normal equations in float64, torch.linalg.solve."""
    nn = knn_points(Xt, Y, lengths, lengths, K=1)
    q = knn_gather(Y, nn.idx, lengths)[:, :, 0].double()
    n = knn_gather(nr, nn.idx, lengths)[:, :, 0].double()
    w = (nn.dists[..., 0] < r2).double()
    x = Xt.double()
    p = x - x[:, :1]
    J = torch.cat([torch.cross(p, n, dim=2), n], 2) * w[..., None]
    rho = ((x - q) * n).sum(2)
    A = torch.einsum("npi,npj->nij", J, J)
    b = -torch.einsum("npi,np->ni", J, rho)
    return torch.linalg.solve(A, b)


SCENES = {"surface": scene, "uniform": uniform_scene}


def bench_shape(which, N, P, steps, rounds, dev):
    X, Y, nr, R, T = SCENES[which](N, P, 1000 + N, dev)
    lengths = torch.full((N,), P, dtype=torch.int64, device=dev)
    r2 = float(np.float32(R_MAX) * np.float32(R_MAX))
    total = steps * rounds + 8

    def new_state(estimation):
        s = _C_registration.RegistrationState(X, Y, nr, lengths, lengths, None, None, R_MAX, estimation, total, -1.0,
                                              -1.0)
        s.step()  # (untimed: builds the grid over the target)
        return s

    plane, point = new_state("point_to_plane"), new_state("point_to_point")
    old = _C.IcpState(X, X.clone(), Y, lengths, lengths, total, False, False, -1.0)
    old.step()
    Xt = plane.Xt.clone()
    variants = {"point_to_plane": plane.step, "point_to_point": point.step, "iterative_closest_point": old.step,
                "torch_composition": lambda: torch_step(Xt, Y, nr, lengths, r2)}
    for fn in variants.values():  # warm every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):  # in alternation: the variants share whatever else the machine is doing
        for k, fn in variants.items():
            times[k].append(timed(fn, steps))
    row = dict(scene=which, N=N, P1=P, P2=P, max_correspondence_distance=R_MAX, steps=steps, rounds=rounds,
               uses_grid=bool(plane.uses_grid))
    for k, v in times.items():
        row[f"step_ms_{k}"] = round(float(np.median(v)), 4)
        row[f"step_ms_min_{k}"] = round(float(np.min(v)), 4)
    for estimation, max_iterations in (("point_to_plane", 30), ("point_to_point", 100)):
        kw = dict(estimation=estimation, target_normals=nr, max_iterations=max_iterations)
        registration_icp(X, Y, R_MAX, **kw)  # (untimed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = registration_icp(X, Y, R_MAX, **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        err = float((r.R.double() - R).flatten(1).norm(dim=1).max())
        row[f"total_ms_{estimation}"] = round(ms, 3)
        row[f"updates_{estimation}"] = int(r.iterations.max())
        row[f"converged_{estimation}"] = int(r.converged.sum())
        row[f"pose_error_{estimation}"] = err
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = iterative_closest_point(X, Y, max_iterations=100)
    torch.cuda.synchronize()
    row["total_ms_iterative_closest_point"] = round((time.perf_counter() - t0) * 1e3, 3)
    row["iterations_iterative_closest_point"] = len(o.t_history)
    row["pose_error_iterative_closest_point"] = float((o.RTs.R.double() - R).flatten(1).norm(dim=1).max())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "registration_bench.jsonl"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--scenes", default="surface,uniform")
    ap.add_argument("--profile-only", action="store_true",
                    help="a few steps of both estimations at the first shape and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_registration needs a GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.profile_only:
        N, P = shapes[0]
        X, Y, nr, _, _ = SCENES[args.scenes.split(",")[0]](N, P, 1000 + N, dev)
        for estimation in ("point_to_plane", "point_to_point"):
            registration_icp(X, Y, R_MAX, estimation=estimation, target_normals=nr, max_iterations=10, check_every=0)
        torch.cuda.synchronize()
        return
    with open(args.out, "w") as f:
        for which, (N, P) in ((w, sh) for w in args.scenes.split(",") for sh in shapes):
            row = bench_shape(which, N, P, args.steps, args.rounds, dev)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
