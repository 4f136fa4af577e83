"""The radius-filter cases of tests/test_filters_gpu.py, in a module of their own because two programs build them: the
test process, and the child processes it starts with POINTOPS_DEBUG=filter_grid=0 / =1 (`python tests/filters_cases.py
OUT.npz` runs every case through the boundary call and saves what it returned).  A case is (points (N, P, D) float32,
lengths (N,) int64, radius, min_neighbors); the builders are seeded, so both programs see the same bytes."""
import sys

import numpy as np

import filters_ref as ref

P = 700                      # above the 512 points from which a cloud gets a grid unasked
LENGTHS = (700, 513, 0)
RADIUS = 0.1
KINDS = {"uniform": ref.uniform_scene, "slab": ref.slab_scene, "outlier": ref.outlier_scene}
MIN_NEIGHBORS = (0, 1, 5, P)
KEYS = ("mask", "index", "num_kept", "counts")


def _batch(kind, D, P_, lengths):
    pts = np.stack([KINDS[kind](100 * D + n, P_, D, radius_=RADIUS) for n in range(len(lengths))])
    return np.ascontiguousarray(pts, np.float32), np.array(lengths, np.int64)


def radius_cases():
    """{name: (points, lengths, radius, min_neighbors)}"""
    cases = {}
    for D in (1, 2, 3):
        for kind in KINDS:
            for mn in MIN_NEIGHBORS:
                cases[f"{kind}-D{D}-mn{mn}"] = (*_batch(kind, D, P, LENGTHS), RADIUS, mn)
        for mn in (0, 1, 5):
            cases[f"short-D{D}-mn{mn}"] = (*_batch("outlier", D, 37, (1, 2, 37)), RADIUS, mn)
        # a pair at exactly the radius (0.25 - 0 = 0.25; 0.25 * 0.25 is exact) is no pair; one ulp more makes it one
        pair = np.zeros((1, 2, D), np.float32)
        pair[0, 1, 0] = 0.25
        cases[f"pair-at-radius-D{D}"] = (pair, np.array([2], np.int64), 0.25, 1)
        cases[f"pair-inside-D{D}"] = (pair, np.array([2], np.int64), float(np.nextafter(np.float32(0.25), np.float32(1))), 1)
    return cases


def run_case(dev, case, want_counts=True):
    """The boundary call -> {key: numpy} (counts only when asked for)."""
    import torch

    from pytorch3d_pointops_amd import _C_filters

    pts, lengths, radius, mn = case
    out = _C_filters.radius_outlier(torch.from_numpy(pts).to(dev), torch.from_numpy(lengths).to(dev), radius, mn,
                                    want_counts=want_counts)
    return {k: t.cpu().numpy() for k, t in zip(KEYS, out) if t is not None}


def main(out_path):
    import torch

    dev = torch.device("cuda:0")
    saved = {}
    for name, case in radius_cases().items():
        for k, a in run_case(dev, case).items():
            saved[f"{name}/{k}"] = a
        saved[f"{name}/mask-early"] = run_case(dev, case, want_counts=False)["mask"]
    torch.cuda.synchronize()
    np.savez(out_path, **saved)


if __name__ == "__main__":
    main(sys.argv[1])
