"""The cases of tests/test_knn_in_radius_cpu.py and tests/test_knn_in_radius_gpu.py, in a module of their own because two
programs build them: the test process, and the child processes it starts with POINTOPS_DEBUG=knn_in_radius_grid=0 / =1
(`python tests/knn_in_radius_cases.py OUT.npz` runs every case through the boundary call and saves what it returned).
The builders are seeded, so both programs see the same bytes.

A case is a Case(p1 (N,P1,D), p2 (N,P2,D) float32, lengths1, lengths2 (N,) int64, K, radius, finite, same): `finite` says
that no coordinate is a NaN or an infinity (the identity with knn_points holds), `same` that p1 is passed as THE tensor
p2, lengths included.  The kernel's list capacities are KC in (1, 4, 8, 16, 32, 64): EDGE_K holds both sides of each edge.
The clouds have 600 to 750 rows -- above the 512 target rows from which a call builds grids unasked -- unless the case
is about something smaller."""
import sys
from collections import namedtuple

import numpy as np

import registration_ref

Case = namedtuple("Case", "p1 p2 lengths1 lengths2 K radius finite same")
EDGE_K = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64)
KEYS = ("idx", "dists", "counts")
AUTO = "auto-1x20000"  # goes through the library's own grid-or-raw choice only (no forced path, no oracle on the CPU)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _i64(a):
    return np.asarray(a, np.int64)


def _uniform(seed, N, P, D):
    return _f32(np.random.default_rng(seed).uniform(0.0, 1.0, (N, P, D)))


def _radius_for(K, P, D):
    """The radius whose ball holds about K of P uniform points of the unit cube: rows with fewer and with more than K."""
    per = K / P
    return float(np.float32({1: per / 2, 2: np.sqrt(per / np.pi), 3: np.cbrt(per / (4.0 / 3.0 * np.pi))}[D]))


def _lattice(side, D):
    axes = np.meshgrid(*[np.arange(side)] * D, indexing="ij")
    return np.stack([a.ravel() for a in axes], 1).astype(np.float64)


def _case(p1, p2, l1, l2, K, radius, finite=True, same=False):
    p2 = _f32(p2)
    l2 = _i64(l2)
    return Case(p2 if same else _f32(p1), p2, l2 if same else _i64(l1), l2, int(K), float(radius), finite, same)


def build_cases():
    cases = {}
    L1, L2 = (650, 300, 0, 7), (700, 513, 5, 0)  # ragged, 0 on either side, len2 < K
    for D in (1, 2, 3):
        for K in (EDGE_K if D == 3 else (1, 4, 17, 64)):
            cases[f"uniform-D{D}-K{K}"] = _case(_uniform(10 * D, 4, 650, D), _uniform(10 * D + 1, 4, 700, D), L1, L2, K,
                                                _radius_for(K, 700, D))
    # one row on either side: inside, at the radius exactly (outside), outside
    one_q = np.zeros((3, 1, 3))
    one_p = np.array([[[0.125, 0, 0]], [[0.25, 0, 0]], [[0.5, 0, 0]]])
    for K in (1, 4):
        cases[f"one-row-K{K}"] = _case(one_q, one_p, (1, 1, 1), (1, 1, 1), K, 0.25)
    # an integer lattice, exact in fp32 at every scale and shift: d2 takes the values s^2 {0, 1, 2, 3, 4, ...} with many
    # exact ties, and for r in {1, 2} many pairs sit at d2 == r2 exactly -- outside.  r = 1: the query itself is the only
    # candidate; inside the lattice r = 1.5 has 19 and r = 2 has 27, which the K cut inside a group of equal distances.
    lat = _lattice(9, 3)
    for r, K in ((1.0, 2), (1.5, 17), (2.0, 9)):
        for e in (-10, 0, 10):
            s = 2.0 ** e
            pts = np.stack([lat * s + 1000.0, lat * s - 1000.0])
            assert np.array_equal(_f32(pts).astype(np.float64), pts)
            cases[f"lattice-r{r}-2^{e}"] = _case(pts.copy(), pts, (729, 729), (729, 729), K, r * s)
    lat2 = _lattice(27, 2)[None]
    cases["lattice-D2-r1.5"] = _case(lat2.copy(), lat2, (729,), (729,), 5, 1.5)
    # duplicated points: every target row three times (ties at every distance, d2 == 0 among them); one point 600 times
    base = _uniform(40, 2, 240, 3)
    cases["duplicates-K2"] = _case(base, np.tile(base, (1, 3, 1)), (240, 100), (720, 719), 2, 0.2)
    cases["duplicates-K5"] = _case(base, np.tile(base, (1, 3, 1)), (240, 100), (720, 719), 5, 0.2)
    same_pt = np.full((1, 600, 3), 0.5)
    q = np.concatenate([np.full((1, 10, 3), 0.5), _uniform(41, 1, 20, 3)], 1)
    cases["all-identical"] = _case(q, same_pt, (30,), (600,), 4, 0.1)
    # no neighbour at all; a radius whose fp32 square is 0 (not even the query itself); a radius beyond the extent (the
    # cube is the whole grid); a radius whose square is +inf (knn_points up to the padding)
    far = _uniform(50, 2, 650, 3)
    far[..., 0] += 5.0
    cases["no-neighbours"] = _case(far, _uniform(51, 2, 700, 3), (650, 650), (700, 700), 4, 0.1)
    cases["r2-underflows"] = _case(None, _uniform(52, 2, 600, 3), None, (600, 555), 1, 1e-30, same=True)
    cases["radius-beyond-extent"] = _case(_uniform(53, 2, 300, 3), _uniform(54, 2, 600, 3), (300, 299), (600, 520), 16, 3.0)
    cases["r2-is-inf"] = _case(_uniform(55, 2, 300, 3), _uniform(56, 2, 600, 3), (300, 299), (600, 520), 8, 2e19)
    # queries outside the target's box beyond one, two and three faces, on either side
    rng = np.random.default_rng(60)
    out = rng.uniform(0.0, 1.0, (2, 600, 3))
    for faces in (1, 2, 3):
        rows = slice(200 * (faces - 1), 200 * faces)
        beyond = rng.uniform(1.0, 1.3, (2, 200, faces))
        out[:, rows, :faces] = np.where(rng.random((2, 200, 1)) < 0.5, beyond, 1.0 - beyond)
    cases["outside-the-box"] = _case(out, _uniform(61, 2, 700, 3), (600, 600), (700, 650), 4, 0.25)
    # queries exactly on cell faces, and one ulp on either side.  The radius decides the cell size here (the density
    # floor of 2 points per cell asks for 0.142), so the grid's cell function is cell_d(x) = int((x - lo_d) * (1 / h))
    # with h = fl32(1.001 r) and lo_d the target's minimum: the faces are at lo_d + k h.
    tgt = _uniform(62, 1, 700, 3)
    h = np.float32(0.2) * np.float32(1.001)
    lo = tgt[0].min(0)
    faces = np.stack([lo + np.float32(k) * h for k in range(1, 5)])           # (4, 3) fp32
    faces = np.concatenate([np.nextafter(faces, np.float32(-9)), faces, np.nextafter(faces, np.float32(9))])  # (12, 3)
    onf = rng.uniform(0.0, 1.0, (1, 400, 3)).astype(np.float32)
    pick = rng.integers(0, 12, (400, 3))
    onf[0] = np.where(rng.random((400, 3)) < 0.6, faces[pick, np.arange(3)[None, :]], onf[0])
    onf[0, :12] = faces
    cases["on-cell-faces"] = _case(onf, tgt, (400,), (700,), 8, 0.2)
    # the surface-plus-clutter scene of registration_icp: a quarter of the queries have nothing within the radius
    scenes = [registration_ref.scene(70 + n, 800, 1000, clutter=True) for n in range(2)]
    for K in (1, 4):
        cases[f"surface-and-clutter-K{K}"] = _case(np.stack([s.X for s in scenes]), np.stack([s.Y for s in scenes]),
                                                   (800, 640), (1000, 900), K, 0.1)
    # p1 passed as the same tensor as p2, and as a clone of it
    self_pts = _uniform(80, 2, 700, 3)
    cases["self-same-tensor"] = _case(None, self_pts, None, (700, 600), 5, 0.15, same=True)
    cases["self-clone"] = _case(self_pts.copy(), self_pts, (700, 600), (700, 600), 5, 0.15)
    # a NaN row and an inf row in the targets of two clouds beside a healthy one (whose queries hold a NaN row): the
    # grid is refused for those two clouds
    bad_q, bad_p = _uniform(90, 3, 650, 3), _uniform(91, 3, 700, 3)
    bad_p[1, 17, 1] = np.nan
    bad_p[2, 5, 0] = np.inf
    bad_q[0, 3, 2] = np.nan
    cases["nan-and-inf-rows"] = _case(bad_q, bad_p, (650, 650, 650), (700, 700, 700), 4, 0.15, finite=False)
    cases[AUTO] = _case(_uniform(100, 1, 20000, 3), _uniform(101, 1, 20000, 3), (20000,), (20000,), 8,
                        1.6 * 20000.0 ** (-1.0 / 3.0))
    return cases


def run_case(dev, case):
    """The boundary call -> {key: numpy}"""
    import torch

    from pytorch3d_pointops_amd import _C_knn_in_radius

    p2, l2 = torch.from_numpy(case.p2).to(dev), torch.from_numpy(case.lengths2).to(dev)
    p1, l1 = (p2, l2) if case.same else (torch.from_numpy(case.p1).to(dev), torch.from_numpy(case.lengths1).to(dev))
    out = _C_knn_in_radius.knn_in_radius(p1, p2, l1, l2, case.K, case.radius)
    return {k: t.cpu().numpy() for k, t in zip(KEYS, out)}


def main(out_path):
    import torch

    dev = torch.device("cuda:0")
    saved = {}
    for name, case in build_cases().items():
        if name == AUTO:
            continue
        for k, a in run_case(dev, case).items():
            saved[f"{name}/{k}"] = a
    torch.cuda.synchronize()
    np.savez(out_path, **saved)


if __name__ == "__main__":
    main(sys.argv[1])
