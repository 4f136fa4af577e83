"""CPU suite of the FPFH feature: the numpy checker (tests/fpfh_ref.py) against a hand-computed pair and against its
own properties, the argument validation of functions/fpfh.py on CPU tensors, and the float32 checker against the
float64 one on the inputs of tests/test_fpfh_gpu.py -- the bounds that suite holds the device to are reachable."""
import math

import numpy as np
import pytest
import torch

import fpfh_ref as ref


def _pair(p0, n0, p1, n1, dtype=np.float64):
    """Features of the two-point cloud {0, 1}, each point's table holding the other: (2, 4)."""
    pts = np.array([[p0, p1]], np.float64)
    nrm = np.array([[n0, n1]], np.float64)
    idx = np.array([[[1], [0]]], np.int64)
    return ref.pair_features(pts, nrm, idx, None, dtype)["f"][0, :, 0, :]


def test_hand_computed_pair():
    """p_i = 0, n_i = e_z; p_j = (3,0,4), n_j = (0.6,0.8,0): d = 5, a1 = 0.8, a2 = 0.36, no swap, f3 = 0.8;
    v = dp x n_i / |.| = -e_y, w = n_i x v = e_x, f2 = v.n_j = -0.8, f1 = atan2(w.n_j, n_i.n_j) = atan2(0.6, 0) = pi/2.
    From j the roles swap (|a1| = 0.36 < |a2| = 0.8) and the features are the same.  Bins: floor(1.5 pi * 11 / (2 pi))
    = floor(8.25) = 8, floor(0.2 * 5.5) = 1, floor(1.8 * 5.5) = floor(9.9) = 9."""
    for dtype, tol in ((np.float64, 1e-15), (np.float32, 1e-6)):
        f = _pair((0, 0, 0), (0, 0, 1), (3, 0, 4), (0.6, 0.8, 0), dtype)
        want = np.array([math.pi / 2, -0.8, 0.8, 5.0])
        assert np.abs(f[0] - want).max() <= tol and np.abs(f[1] - want).max() <= tol, f
        assert ref.bins(f, dtype).tolist() == [[8, 1, 9], [8, 1, 9]]
    sp = ref.spfh_from_bins(ref.bins(f[None, :, None, :]), np.ones((1, 2, 1), bool))
    want = np.zeros(33, np.float32)
    want[[8, 11 + 1, 22 + 9]] = 100.0
    assert np.array_equal(sp[0, 0], want) and np.array_equal(sp[0, 1], want)


def test_dead_slots_and_uncounted_pairs():
    pts = np.array([[[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 2], [9, 9, 9]]], np.float32)
    nrm = np.array([[[0, 0, 1], [0, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]]], np.float32)
    # row 0: itself, a neighbour, -1 padding, a row past the length, a neighbour along its own normal (dp x ns = 0)
    idx = np.array([[[0, 1, -1, 4, 3], [2, 0, 1, 1, 1], [0] * 5, [0] * 5, [0] * 5]], np.int64)
    pf = ref.pair_features(pts, nrm, idx, np.array([4]), np.float32)
    assert pf["live"][0, 0].tolist() == [False, True, False, False, True]
    assert pf["counted"][0, 0].tolist() == [False, True, False, False, False]
    assert pf["live"][0, 1].tolist() == [False, True, False, False, False]  # the duplicate, the neighbour, itself
    assert not pf["live"][0, 4].any() and not pf["f"][0, 4].any()  # a row past the length
    assert not pf["f"][0, 0, [0, 2, 3, 4]].any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_spfh_groups_sum_to_100(dtype):
    pts, nrm = ref.cloud("heightfield", 2, 200)
    lengths = np.array([200, 90])
    idx = ref.knn_self(pts, lengths, 12)
    fp, sp, pf = ref.fpfh(pts, nrm, idx, lengths, dtype)
    assert sp.dtype == dtype and fp.dtype == dtype
    sums = sp.astype(np.float64).reshape(2, 200, 3, 11).sum(-1)
    m = pf["counted"].sum(2)
    assert (m[0] > 0).all() and (m[1, :90] > 0).all() and (m[1, 90:] == 0).all()
    assert np.abs(sums[m > 0] - 100.0).max() <= 1e-4 and not sums[m == 0].any()
    assert not fp[1, 90:].any() and fp.min() >= 0 and fp.max() <= 200 + 1e-3


def test_float64_fpfh_is_invariant_under_a_rigid_motion():
    pts, nrm = ref.cloud("heightfield", 1, 300)
    idx = ref.knn_self(pts, [300], 16)
    R, t = ref.rigid_motion()
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0
    a, _, _ = ref.fpfh(pts, nrm, idx)
    b, _, _ = ref.fpfh(pts.astype(np.float64) @ R.T + t, nrm.astype(np.float64) @ R.T, idx)
    assert np.abs(a - b).max() <= 1e-6


def test_swap_rule_is_symmetric():
    """Computed from either end, a pair has the same source: f1, f2 and f3 agree, so no sign can change."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        p0, p1, n0, n1 = rng.standard_normal((4, 3))
        n0, n1 = n0 / np.linalg.norm(n0), n1 / np.linalg.norm(n1)
        f = _pair(p0, n0, p1, n1)
        assert f[0, 3] > 0 and np.sign(f[0, 0]) == np.sign(f[1, 0]) and np.sign(f[0, 1]) == np.sign(f[1, 1])
        worst = max(worst, float(np.abs(f[0] - f[1]).max()))
    assert worst <= 1e-9


def test_exported_names():
    from pytorch3d_pointops_amd import functions

    assert {"fpfh_features", "point_pair_features", "mutual_nearest_neighbors"} <= set(functions.__all__)


def test_validation_errors():
    from pytorch3d_pointops_amd.functions import fpfh_features, mutual_nearest_neighbors, point_pair_features

    p, n = torch.rand(2, 20, 3), torch.rand(2, 20, 3)
    idx = torch.zeros(2, 20, 4, dtype=torch.int64)
    for bad in (torch.rand(20, 3), torch.rand(2, 20, 2)):
        with pytest.raises(ValueError, match=r"\(N, P, 3\)"):
            fpfh_features(bad, n, idx=idx)
        with pytest.raises(ValueError, match=r"\(N, P, 3\)"):
            point_pair_features(bad, n, idx)
    with pytest.raises(ValueError, match="float32"):
        fpfh_features(p.double(), n, idx=idx)
    with pytest.raises(ValueError, match="float32"):
        fpfh_features(p, n.double(), idx=idx)
    with pytest.raises(ValueError, match="float32"):
        point_pair_features(p, n.double(), idx)
    with pytest.raises(ValueError, match="shape of points"):
        fpfh_features(p, n[:, :19], idx=idx)
    for K in (0, 256, -3):
        with pytest.raises(ValueError, match=r"K must be in 1\.\.255"):
            fpfh_features(p, n, K=K)
    for bad in (idx.int(), idx[:, :19], idx[0], torch.zeros(2, 20, 256, dtype=torch.int64),
                torch.zeros(2, 20, 0, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"idx must be an int64 tensor of shape \(N, P, K\)|K must be in"):
            fpfh_features(p, n, idx=bad)
        with pytest.raises(ValueError, match=r"idx must be an int64 tensor of shape \(N, P, K\)|K must be in"):
            point_pair_features(p, n, bad)
    for bad in (torch.tensor([20, 20, 20]), torch.tensor([20, 20], dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"lengths must be an int64 tensor of shape \(N,\)"):
            fpfh_features(p, n, bad, idx=idx)
    with pytest.raises(ValueError, match="pass the normals"):
        fpfh_features(p, None, torch.tensor([20, 11]), K=4)
    with pytest.raises(ValueError, match=r"shape \(N, P, D\)"):
        mutual_nearest_neighbors(torch.rand(20, 33), torch.rand(2, 20, 33))
    with pytest.raises(ValueError, match="float32"):
        mutual_nearest_neighbors(torch.rand(2, 20, 33), torch.rand(2, 20, 33).double())
    with pytest.raises(ValueError, match="same batch and feature dimensions"):
        mutual_nearest_neighbors(torch.rand(2, 20, 33), torch.rand(2, 20, 32))
    with pytest.raises(ValueError, match="lengths2 must be an int64 tensor"):
        mutual_nearest_neighbors(torch.rand(2, 20, 33), torch.rand(2, 9, 33), None, torch.tensor([9]))


def test_no_cpu_fallback():
    from pytorch3d_pointops_amd.functions import fpfh_features, mutual_nearest_neighbors, point_pair_features

    p, n = torch.rand(2, 20, 3), torch.rand(2, 20, 3)
    idx = torch.zeros(2, 20, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        point_pair_features(p, n, idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fpfh_features(p, n, idx=idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fpfh_features(p, n, K=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fpfh_features(p, n, K=4, radius=0.3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mutual_nearest_neighbors(torch.rand(2, 20, 33), torch.rand(2, 9, 33))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mutual_nearest_neighbors(torch.rand(2, 0, 33), torch.rand(2, 9, 33))


@pytest.mark.parametrize("name", ref.CLOUDS)
@pytest.mark.parametrize("K", ref.KS)
def test_float32_checker_stays_within_the_device_bounds(name, K):
    """The staged bounds of the GPU suite, with the float32 checker in the device's place and a float64 brute-force
    table in knn_points' layout: pair features within T over their conditioning, at most 1 % of the live slots left
    out, the same slots counted, and the FPFH of the float32 SPFH within 16 * 200 * 2^-24."""
    N, P = ref.shape_for(K)
    pts, nrm = ref.cloud(name, N, P)
    lengths = ref.lengths_for(P, K)
    idx = ref.knn_self(pts, lengths, K)
    f64 = ref.pair_features(pts, nrm, idx, lengths, np.float64)
    f32 = ref.pair_features(pts, nrm, idx, lengths, np.float32)
    rep = ref.pair_feature_report(f32["f"], f64)
    print(name, K, "ratios (f1, f2, f3, d):", rep["ratio"], "excluded:", rep["excluded"])
    assert rep["excluded"] <= 0.01
    assert max(rep["ratio"]) <= 1.0, rep["ratio"]
    assert np.array_equal(f32["counted"][rep["kept"]], f64["counted"][rep["kept"]])
    assert not f32["f"][~f64["live"]].any()
    sp32 = ref.spfh_from_bins(ref.bins(f32["f"]), f32["counted"])
    got = ref.fpfh_from_spfh(sp32, idx, f32["live"], f32["d2"], np.float32)
    want = ref.fpfh_from_spfh(sp32, idx, f64["live"], f64["d2"], np.float64)
    err = float(np.abs(got - want).max())
    print(name, K, "fpfh float32 error over 200 * 2^-24:", err / (200 * ref.EPS))
    assert err <= ref.T_FPFH
    valid = np.arange(P)[None, :] < lengths[:, None]
    assert not got[~valid].any() and not sp32[~valid].any()
