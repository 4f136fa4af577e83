"""Operator boundary of the outlier filters (csrc/filters.hip; C ABI: pointops_radius_outlier,
pointops_statistical_outlier and pointops_mask_compact in include/pointops_amd.h).

Beside `_C.py`, not in it, as `_C_iss.py` is: eager-only building blocks of functions/filters.py, not registered
operators.  Everything they use is `_C`'s -- the argument normalisers, the native-call namespace and the output seam --
looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees these calls too.  There is no CPU
implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

STAT_MAX_K1 = 128  # knn_points' longest list: nb_neighbors + 1


def _mask_u8(mask, name):
    """One byte per row, contiguous: a bool or uint8 tensor as the kernels read it."""
    if mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"{name} must be bool or uint8")
    return mask.contiguous()


def mask_compact(mask):
    """mask (N,P) bool or uint8 -> (index (N,P) int64: the kept rows of every cloud in ascending order, then -1;
    num_kept (N,) int64)."""
    dev = _C._require_gpu(mask)
    if mask.dim() != 2:
        raise RuntimeError("mask_compact: need mask (N,P)")
    mask = _mask_u8(mask, "mask")
    N, P = mask.shape
    index = _C._out((N, P), dtype=torch.int64, device=dev)
    num_kept = _C._out((N,), dtype=torch.int64, device=dev)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        _C._call.mask_compact("mask_compact", dev, r(mask), n, P, r(index), r(num_kept))
    return index, num_kept


def radius_outlier(points, lengths, radius: float, min_neighbors: int, want_counts: bool = False):
    """points (N,P,D) fp32, D in 1..3; lengths (N,) int64 or None ->
    (mask (N,P) bool, index (N,P) int64, num_kept (N,) int64, counts (N,P) int32 or None)."""
    dev = _C._require_gpu(points, lengths)
    points, lengths = _C._f32c(points, "points"), _C._i64c(lengths, "lengths")
    if points.dim() != 3 or not 1 <= points.shape[2] <= 3:
        raise RuntimeError("radius_outlier: need points (N,P,D) with D in 1..3")
    N, P, D = points.shape
    if lengths is not None and lengths.shape != (N,):
        raise RuntimeError("radius_outlier: need lengths (N,)")
    mask = _C._out((N, P), dtype=torch.bool, device=dev)
    counts = _C._out((N, P), dtype=torch.int32, device=dev) if want_counts else None
    index = _C._out((N, P), dtype=torch.int64, device=dev)
    num_kept = _C._out((N,), dtype=torch.int64, device=dev)
    sizer = _C._lib.pointops_radius_outlier_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.radius_outlier("radius_outlier", dev, r(points), r(lengths), n, P, D, float(radius),
                                int(min_neighbors), r(mask), r(counts), r(index), r(num_kept), workspace, sizer(n, P))
    return mask, index, num_kept, counts


def statistical_outlier(dists, lengths, std_ratio: float):
    """dists (N,P,K1) fp32: the squared distances of knn_points of the cloud against itself, K1 = nb_neighbors + 1;
    lengths (N,) int64 or None -> (mask (N,P) bool, index (N,P) int64, num_kept (N,) int64, mean_distance (N,P) fp32,
    threshold (N,) fp32, stats (N,3) fp64 = (mean, std, n_f))."""
    dev = _C._require_gpu(dists, lengths)
    dists, lengths = _C._f32c(dists, "dists"), _C._i64c(lengths, "lengths")
    if dists.dim() != 3 or not 2 <= dists.shape[2] <= STAT_MAX_K1:
        raise RuntimeError(f"statistical_outlier: need dists (N,P,K1) with 2 <= K1 <= {STAT_MAX_K1}")
    N, P, K1 = dists.shape
    if lengths is not None and lengths.shape != (N,):
        raise RuntimeError("statistical_outlier: need lengths (N,)")
    mean_distance = _C._out((N, P), dtype=torch.float32, device=dev)
    stats = _C._out((N, 3), dtype=torch.float64, device=dev)
    threshold = _C._out((N,), dtype=torch.float32, device=dev)
    mask = _C._out((N, P), dtype=torch.bool, device=dev)
    index = _C._out((N, P), dtype=torch.int64, device=dev)
    num_kept = _C._out((N,), dtype=torch.int64, device=dev)
    sizer = _C._lib.pointops_statistical_outlier_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        _C._call.statistical_outlier("statistical_outlier", dev, r(dists), r(lengths), n, P, K1, float(std_ratio),
                                     r(mean_distance), r(stats), r(threshold), r(mask), r(index), r(num_kept),
                                     workspace, sizer(n, P))
    return mask, index, num_kept, mean_distance, threshold, stats
