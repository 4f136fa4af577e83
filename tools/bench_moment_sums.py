#!/usr/bin/env python3
"""The kernels behind point_covariances, local_frames, points_alignment, icp_iteration and registration_step, timed for
two builds of the library in alternation -- the comparison a refactor of these kernels owes its parent commit.

    python tools/bench_moment_sums.py --parent PATH/libpointops_amd.so [--change PATH] [--alternations 5] [--out FILE]

The driver never touches the GPU.  It starts one child process per build and alternation (a process loads one library:
POINTOPS_AMD_LIB), parent first, then the change, and so on; every child warms each row up, then times it in `--windows`
windows of `--reps` consecutive calls between two device events.  The table (profiles/moment_sums_once_bench.txt by
default) gives, per row and build, the median and the range of all windows, the parent's spread (its range over its
median), whether the change's median lies within the parent's range, and whether both builds wrote the same bytes.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P = 8, 65536


def rows(dev):
    """[(name, fn, outputs)]: fn enqueues one call; outputs() gives the tensors whose bytes the builds must share"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from pytorch3d_pointops_amd import _C, _C_registration, synth
    from pytorch3d_pointops_amd.functions import knn_points

    G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    pts = G(synth.uniform_f32(1, (N, P, 3)))
    lengths = torch.full((N,), P, dtype=torch.int64, device=dev)
    out = []

    def covariances(name, knn):
        grad = G(synth.uniform_f32(5, tuple(knn.shape[:2]) + (knn.shape[3],) * 2)) - 0.5
        keep = {}

        def fwd():
            keep["cov"] = _C.point_covariances(knn)

        def bwd():
            keep["grad"] = _C.point_covariances_backward(knn, grad)

        out.append((f"point_covariances forward {name}", fwd, lambda: [keep["cov"]]))
        out.append((f"point_covariances backward {name}", bwd, lambda: [keep["grad"]]))

    idx = {K: knn_points(pts, pts, lengths, lengths, K=K).idx for K in (16, 32, 80)}
    covariances("8x65536x16x3 (staged)", _C.gather_neighbors(pts, idx[16], lengths))
    covariances("8x65536x32x3 (direct)", _C.gather_neighbors(pts, idx[32], lengths))
    covariances("8x65536x8x4 (runtime D)", G(synth.uniform_f32(2, (N, P, 8, 4))))
    for K in (16, 80):
        keep = {}

        def frames(K=K, keep=keep):
            keep["out"] = _C.local_frames(pts, lengths, idx[K], True)

        out.append((f"local_frames 8x65536 K={K}", frames, lambda keep=keep: list(keep["out"])))

    NA = 32
    X = G(synth.uniform_f32(3, (NA, P, 3)))
    Y = G(synth.uniform_f32(4, (NA, P, 3)) * np.float32(0.05)) + X
    la = torch.full((NA,), P, dtype=torch.int64, device=dev)
    aidx = G(synth.randint(6, 0, P - 1, (NA, P)))
    w = G(synth.uniform_f32(7, (NA, P)))
    keep_a = {}

    def alignment():
        keep_a["out"] = _C.points_alignment(X, Y, aidx, la, w, True, False, 1e-9, want_moments=True)

    out.append(("points_alignment 32x65536x3 idx, weights", alignment, lambda: list(keep_a["out"])))

    icp = _C.IcpState(X, X.clone(), Y, la, la, 4, False, False, -1.0)
    icp.step()  # (builds the grid over Y; the timed calls align to this neighbour table)

    def icp_step():
        icp.steps = 1  # (the same history entry every time; Xt moves on, as in a run)
        icp.step()

    out.append(("icp_iteration 32x65536x3", icp_step, lambda: [icp.R[1], icp.T[1], icp.s[1], icp.Xt, icp.rmse]))
    normals = G(synth.unit_normals(8, (NA, P, 3)))
    for est in ("point_to_plane", "point_to_point"):
        st = _C_registration.RegistrationState(X, Y, normals, la, la, None, None, 0.04, est, 4, -1.0, -1.0,
                                               want_moments=True)
        st.step()

        def reg_step(st=st):
            st.steps = 1  # (the same history entry every time; the state moves on, as in a run)
            st.step()

        out.append((f"registration_step {est} 32x65536", reg_step,
                    lambda st=st: [st.moments, st.num_correspondences, st.status]))
    return out


def child(args):
    import torch

    dev = torch.device("cuda:0")
    result = {}
    for name, fn, outputs in rows(dev):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        digest = hashlib.blake2b(b"".join(t.detach().cpu().numpy().tobytes() for t in outputs()),
                                 digest_size=8).hexdigest()
        times = []
        for _ in range(args.windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / args.reps)
        result[name] = {"us": times, "digest": digest}
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's libpointops_amd.so")
    ap.add_argument("--change", default=os.path.join(ROOT, "pytorch3d_pointops_amd", "lib", "libpointops_amd.so"))
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moment_sums_once_bench.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent:
        raise SystemExit("--parent is required: speed is measured against the parent commit's build")
    import numpy as np

    samples = {"parent": {}, "change": {}}
    digests = {"parent": {}, "change": {}}
    for i in range(args.alternations):
        for side, lib in (("parent", args.parent), ("change", args.change)):
            env = dict(os.environ, POINTOPS_AMD_LIB=os.path.abspath(lib))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--windows", str(args.windows), "--reps",
                   str(args.reps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:  # nothing more is started on the GPU after a child that failed
                raise SystemExit(f"{side} child {i} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for name, v in res.items():
                samples[side].setdefault(name, []).extend(v["us"])
                digests[side].setdefault(name, set()).add(v["digest"])
            print(f"alternation {i} {side}: done", flush=True)
    lines = [
        "Moment and neighbourhood sums written once: time per call on the MI355X, parent commit against this change",
        "",
        f"python tools/bench_moment_sums.py --parent <parent build> --alternations {args.alternations} --windows "
        f"{args.windows} --reps {args.reps} --warmup {args.warmup}",
        f"One process per build and alternation, parent and change in turn; every process warms a row up with {args.warmup}"
        f" calls and times {args.windows} windows of {args.reps}",
        f"consecutive calls between two device events: {args.alternations * args.windows} windows per row and build.  "
        "Microseconds per call: median [min, max].",
        "spread = the parent's (max - min) / median, its own run-to-run noise.  within = the change's median lies in the "
        "parent's range.",
        "bytes = both builds wrote the same output bytes in every process (the ICP and registration rows step a state that",
        "moves on with every call, the same number of calls in every process).",
        "",
        "%-46s %28s %8s %28s %7s %6s %6s" % ("row", "parent us", "spread", "change us", "ratio", "within", "bytes"),
    ]
    for name in samples["parent"]:
        p, c = np.array(samples["parent"][name]), np.array(samples["change"][name])
        pm, cm = float(np.median(p)), float(np.median(c))
        same = len(digests["parent"][name] | digests["change"][name]) == 1
        lines.append("%-46s %28s %7.1f%% %28s %7.3f %6s %6s" % (
            name, "%.1f [%.1f, %.1f]" % (pm, p.min(), p.max()), 100.0 * (p.max() - p.min()) / pm,
            "%.1f [%.1f, %.1f]" % (cm, c.min(), c.max()), cm / pm, "yes" if p.min() <= cm <= p.max() else "NO",
            "same" if same else "DIFFER"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
