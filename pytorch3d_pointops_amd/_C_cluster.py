"""Operator boundary of the density clustering (csrc/cluster.hip; C ABI: pointops_cluster_dbscan in
include/pointops_amd.h).

Beside `_C.py`, not in it, as `_C_ransac.py` is: an eager-only building block of functions/cluster.py, not a registered
operator.  Everything it uses is `_C`'s -- the argument normalisers, the native-call namespace and the output seam --
looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees this call too.  There is no CPU
implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C


def cluster_dbscan(points, lengths, eps: float, min_points: int):
    """points (N,P,D) fp32, D in 1..3; lengths (N,) int64 or None ->
    (labels (N,P) int64, num_clusters (N,) int64, core_mask (N,P) bool)."""
    dev = _C._require_gpu(points, lengths)
    points, lengths = _C._f32c(points, "points"), _C._i64c(lengths, "lengths")
    if points.dim() != 3 or not 1 <= points.shape[2] <= 3:
        raise RuntimeError("cluster_dbscan: need points (N,P,D) with D in 1..3")
    N, P, D = points.shape
    if lengths is not None and lengths.shape != (N,):
        raise RuntimeError("cluster_dbscan: need lengths (N,)")
    labels = _C._out((N, P), dtype=torch.int64, device=dev)
    num_clusters = _C._out((N,), dtype=torch.int64, device=dev)
    core_mask = _C._out((N, P), dtype=torch.bool, device=dev)
    sizer = _C._lib.pointops_cluster_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.cluster_dbscan("cluster_dbscan", dev, r(points), r(lengths), n, P, D, float(eps), int(min_points),
                                r(labels), r(num_clusters), r(core_mask), workspace, sizer(n, P))
    return labels, num_clusters, core_mask
