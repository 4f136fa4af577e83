#!/usr/bin/env python3
"""registration_icp's step with search="exact" against search="bounded" on the MI355X, on the two scenes of
tools/bench_registration.py (the surface with a quarter of clutter rows, and uniform clouds): one JSON line per
(scene, shape, estimation) into profiles/registration_bounded_bench.jsonl (--out).

Step times are HIP-event times over `--steps` consecutive steps on one state (the search structure over the target is
built by an untimed first step), thresholds at -1 so that no cloud freezes and every step does all its work; the two
searches are timed in alternation, `--rounds` times, and the median is reported with the minimum and the maximum --
the run-to-run spread a "faster" or "not slower" has to clear.  Both states walk the same poses: their steps are
byte-equal."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_registration import R_MAX, SCENES, timed  # noqa: E402
from pytorch3d_pointops_amd import _C_registration  # noqa: E402

SHAPES = ((8, 65536), (16, 131072))


def bench_shape(which, N, P, estimation, steps, rounds, dev):
    X, Y, nr, _, _ = SCENES[which](N, P, 1000 + N, dev)
    lengths = torch.full((N,), P, dtype=torch.int64, device=dev)
    total = steps * rounds + 8

    def new_state(search):
        s = _C_registration.RegistrationState(X, Y, nr, lengths, lengths, None, None, R_MAX, estimation, total, -1.0,
                                              -1.0, search=search)
        s.step()  # (untimed: builds the search structure over the target)
        return s

    states = {"exact": new_state("exact"), "bounded": new_state("bounded")}
    for s in states.values():
        s.step()
    torch.cuda.synchronize()
    times = {k: [] for k in states}
    for _ in range(rounds):  # in alternation: the variants share whatever else the machine is doing
        for k, s in states.items():
            times[k].append(timed(s.step, steps))
    same = all(torch.equal(getattr(states["exact"], k), getattr(states["bounded"], k))
               for k in ("Xt", "state", "correspondences", "num_correspondences"))
    row = dict(scene=which, N=N, P1=P, P2=P, estimation=estimation, max_correspondence_distance=R_MAX, steps=steps,
               rounds=rounds, exact_uses_grid=bool(states["exact"].uses_grid), byte_equal=bool(same),
               inlier_fraction=round(float(states["exact"].num_correspondences.double().mean()) / P, 4))
    for k, v in times.items():
        row[f"step_ms_{k}"] = round(float(np.median(v)), 4)
        row[f"step_ms_min_{k}"] = round(float(np.min(v)), 4)
        row[f"step_ms_max_{k}"] = round(float(np.max(v)), 4)
    row["exact_over_bounded"] = round(row["step_ms_exact"] / row["step_ms_bounded"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "registration_bounded_bench.jsonl"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{n}x{p}" for n, p in SHAPES))
    ap.add_argument("--scenes", default="surface,uniform")
    ap.add_argument("--estimations", default="point_to_plane,point_to_point")
    ap.add_argument("--profile-only", action="store_true",
                    help="three bounded steps at the first shape and scene and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_registration_bounded needs a GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.profile_only:
        N, P = shapes[0]
        X, Y, nr, _, _ = SCENES[args.scenes.split(",")[0]](N, P, 1000 + N, dev)
        lengths = torch.full((N,), P, dtype=torch.int64, device=dev)
        s = _C_registration.RegistrationState(X, Y, nr, lengths, lengths, None, None, R_MAX, "point_to_plane", 3, -1.0,
                                              -1.0, search="bounded")
        for _ in range(3):
            s.step()
        torch.cuda.synchronize()
        return
    with open(args.out, "w") as f:
        for which in args.scenes.split(","):
            for N, P in shapes:
                for estimation in args.estimations.split(","):
                    line = json.dumps(bench_shape(which, N, P, estimation, args.steps, args.rounds, dev))
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
