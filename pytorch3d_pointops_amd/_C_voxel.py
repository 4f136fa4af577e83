"""Operator boundary of the voxel-grid pooling (csrc/voxel.hip; C ABI: pointops_voxel_downsample in
include/pointops_amd.h).

Beside `_C.py`, not in it, as `_C_iss.py` is: an eager-only building block of functions/voxel.py, not a registered
operator.  Everything it uses is `_C`'s -- the argument normalisers, the native-call namespace and the output seam --
looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees this call too.  There is no CPU
implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

VOXEL_MAX_CHANNELS = 1024


def voxel_downsample(points, lengths, voxel_size: float, features=None, origin=None, want_coords: bool = True):
    """points (N,P,3) fp32; lengths (N,) int64 or None; features (N,P,C) fp32 or None; origin (3,) or (N,3) fp32 or None
    -> (num_voxels (N,) int64, status (N,) int32, inverse (N,P) int64, counts (N,P) int64, first_index (N,P) int64,
    coords (N,P,3) int64 or None, centroids (N,P,3) fp32, pooled (N,P,C) fp32 or None)."""
    dev = _C._require_gpu(points, lengths, features, origin)
    points, lengths = _C._f32c(points, "points"), _C._i64c(lengths, "lengths")
    features, origin = _C._f32c(features, "features"), _C._f32c(origin, "origin")
    if points.dim() != 3 or points.shape[2] != 3:
        raise RuntimeError("voxel_downsample: need points (N,P,3)")
    N, P, _ = points.shape
    if lengths is not None and lengths.shape != (N,):
        raise RuntimeError("voxel_downsample: need lengths (N,)")
    if features is not None and (features.dim() != 3 or features.shape[:2] != (N, P)):
        raise RuntimeError("voxel_downsample: need features (N,P,C)")
    C = 0 if features is None else features.shape[2]
    if C > VOXEL_MAX_CHANNELS:
        raise RuntimeError(f"voxel_downsample: at most {VOXEL_MAX_CHANNELS} feature channels, got {C}")
    if origin is not None and origin.shape not in ((3,), (N, 3)):
        raise RuntimeError("voxel_downsample: need origin (3,) or (N,3)")
    per_cloud = origin is not None and origin.dim() == 2
    num_voxels = _C._out((N,), dtype=torch.int64, device=dev)
    status = _C._out((N,), dtype=torch.int32, device=dev)
    inverse = _C._out((N, P), dtype=torch.int64, device=dev)
    counts = _C._out((N, P), dtype=torch.int64, device=dev)
    first_index = _C._out((N, P), dtype=torch.int64, device=dev)
    coords = _C._out((N, P, 3), dtype=torch.int64, device=dev) if want_coords else None
    centroids = _C._out((N, P, 3), dtype=torch.float32, device=dev)
    pooled = _C._out((N, P, C), dtype=torch.float32, device=dev) if features is not None else None
    sizer = _C._lib.pointops_voxel_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P, C)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.voxel_downsample("voxel_downsample", dev, r(points), r(lengths), r(features) if C else None,
                                  r(origin) if per_cloud else origin, per_cloud, n, P, C, float(voxel_size),
                                  r(num_voxels), r(status), r(inverse), r(counts), r(first_index), r(coords),
                                  r(centroids), r(pooled) if C else None, workspace, sizer(n, P, C))
    return num_voxels, status, inverse, counts, first_index, coords, centroids, pooled
