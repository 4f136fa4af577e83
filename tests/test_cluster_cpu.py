"""cluster_dbscan without a GPU: the numpy checker of tests/cluster_ref.py against scikit-learn's brute-force DBSCAN,
the constructed border scene, the checker's two component routines against each other, and the argument checks of
functions/cluster.py (which come before any launch)."""
import numpy as np
import pytest
import torch

import cluster_ref


def test_checker_equals_sklearn_on_random_scenes():
    cluster = pytest.importorskip("sklearn.cluster")
    kept = 0
    for p, eps, min_points in cluster_ref.random_scenes(40):
        p32 = p.astype(np.float32)
        p = p32.astype(np.float64)  # scikit-learn sees float64 copies of the float32 inputs
        d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
        if (np.abs(d - eps) / eps < 1e-5).any():
            continue  # a pair at eps: scikit-learn compares <= in float64, the definition < in float32
        kept += 1
        sk = cluster.DBSCAN(eps=eps, min_samples=min_points, algorithm="brute").fit(p)
        labels, core, num = cluster_ref.dbscan_cloud(p32, eps, min_points)
        sk_core = np.zeros(len(p), bool)
        sk_core[sk.core_sample_indices_] = True
        assert np.array_equal(core, sk_core)
        assert np.array_equal(labels, sk.labels_.astype(np.int64))
        assert num == (sk.labels_.max() + 1 if len(p) else 0)
    assert kept >= 30, kept


def test_checker_component_routines_agree():
    for p, eps, min_points in cluster_ref.random_scenes(12):
        a = cluster_ref.dbscan_cloud(p.astype(np.float32), eps, min_points, use_scipy=True)
        b = cluster_ref.dbscan_cloud(p.astype(np.float32), eps, min_points, use_scipy=False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    p, pos = cluster_ref.chain_scene(512, 0.01, "shuffled", cut=200)
    labels, core, num = cluster_ref.dbscan_cloud(p, 0.01, 2, use_scipy=False)
    assert num == 2 and core.all()
    side = (pos >= 200) != (pos[0] >= 200)  # False on the side that holds row 0
    assert np.array_equal(labels, side.astype(np.int64))


def test_checker_border_point_takes_the_smallest_label():
    p, eps, min_points = cluster_ref.bridge_scene()
    labels, core, num = cluster_ref.dbscan_cloud(p, eps, min_points)
    assert num == 2
    assert core[:40].all() and not core[40]
    assert (labels[:20] == 0).all() and (labels[20:40] == 1).all()
    assert labels[40] == 0
    adj = cluster_ref.neighbours(p, eps)
    assert adj[40].sum() == 3 and adj[40, 0] and adj[40, 20]  # within eps of a core point of each blob
    # the same scene with the blobs in the other index order: the bridge still takes label 0, now the other blob's
    q = np.concatenate([p[20:40], p[:20], p[40:]])
    labels, core, num = cluster_ref.dbscan_cloud(q, eps, min_points)
    assert num == 2 and labels[40] == 0 and (labels[:20] == 0).all() and (labels[20:40] == 1).all()


def test_checker_padding_and_empty_clouds():
    p = cluster_ref.blobs_scene(1, 64)[None].repeat(3, 0)
    labels, num, core = cluster_ref.dbscan(p, [0, 1, 64], 0.08, 1)
    assert (labels[0] == -1).all() and num[0] == 0 and not core[0].any()
    assert labels[1, 0] == 0 and (labels[1, 1:] == -1).all() and num[1] == 1 and core[1].sum() == 1
    assert (labels[2] >= 0).all() and num[2] == labels[2].max() + 1


def test_exports():
    from pytorch3d_pointops_amd import _C, functions
    from pytorch3d_pointops_amd.structures import Pointclouds

    assert callable(functions.cluster_dbscan) and callable(functions.euclidean_clusters)
    assert functions.DBSCANClusters._fields == ("labels", "num_clusters", "core_mask")
    assert callable(Pointclouds.cluster_dbscan)
    assert {"pointops_cluster_dbscan", "pointops_cluster_workspace_bytes"} <= set(_C.exported_symbols())
    # an empty batch needs no scratch; the sizer refuses what the entry refuses
    assert _C._lib.pointops_cluster_workspace_bytes(0, 100) == 0
    assert _C._lib.pointops_cluster_workspace_bytes(65536, 100) == 0
    assert _C._lib.pointops_cluster_workspace_bytes(3, 100) > 0


def test_validation_errors_come_before_any_launch():
    from pytorch3d_pointops_amd.functions import cluster_dbscan, euclidean_clusters

    p = torch.zeros(2, 8, 3)
    for eps in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60):
        with pytest.raises(ValueError, match="eps"):
            cluster_dbscan(p, eps, 3)
    for mp in (0, -2, 2.5):
        with pytest.raises(ValueError, match="min_points"):
            cluster_dbscan(p, 0.1, mp)
    with pytest.raises(ValueError, match="shape"):
        cluster_dbscan(torch.zeros(8, 3), 0.1, 3)
    with pytest.raises(ValueError, match="shape"):
        cluster_dbscan(torch.zeros(2, 8, 4), 0.1, 3)
    with pytest.raises(ValueError, match="float32"):
        cluster_dbscan(p.double(), 0.1, 3)
    with pytest.raises(ValueError, match="lengths"):
        cluster_dbscan(p, 0.1, 3, lengths=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="lengths"):
        cluster_dbscan(p, 0.1, 3, lengths=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="eps"):
        euclidean_clusters(p, 0.0)


def test_cpu_tensors_raise():
    from pytorch3d_pointops_amd.functions import cluster_dbscan, euclidean_clusters
    from pytorch3d_pointops_amd.structures import Pointclouds

    p = torch.rand(2, 8, 3)
    with pytest.raises(RuntimeError, match="GPU-only"):
        cluster_dbscan(p, 0.1, 3)
    with pytest.raises(RuntimeError, match="GPU-only"):
        euclidean_clusters(p, 0.1, lengths=torch.tensor([8, 3]))
    with pytest.raises(RuntimeError, match="GPU-only"):
        Pointclouds([p[0], p[1, :5]]).cluster_dbscan(0.1, 3)
