"""Operator boundary of the moving-least-squares smoothing (csrc/mls.hip; C ABI: pointops_mls_smooth in
include/pointops_amd.h).

Beside `_C.py`, not in it, as `_C_iss.py` is: an eager-only building block of functions/mls.py, not a registered
operator.  Everything it uses is `_C`'s -- the argument normalisers, the native-call namespace and the output seam --
looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees this call too.  There is no CPU
implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

MLS_MOMENTS = 10  # W, M1[3], M2[6] (xx, xy, xz, yy, yz, zz)


def mls_smooth(points, lengths, radius: float, min_neighbors: int, iterations: int = 1, want_moments: bool = False):
    """points (N,P,3) fp32; lengths (N,) int64 or None ->
    (points (N,P,3) fp32, normals (N,P,3) fp32, curvature (N,P) fp32, num_neighbors (N,P) int64, status (N,P) uint8,
    moments (N,P,10) int64 or None) -- all of the last of `iterations` passes."""
    dev = _C._require_gpu(points, lengths)
    points, lengths = _C._f32c(points, "points"), _C._i64c(lengths, "lengths")
    if points.dim() != 3 or points.shape[2] != 3:
        raise RuntimeError("mls_smooth: need points (N,P,3)")
    N, P, _ = points.shape
    if lengths is not None and lengths.shape != (N,):
        raise RuntimeError("mls_smooth: need lengths (N,)")
    smoothed = _C._out((N, P, 3), dtype=torch.float32, device=dev)
    normals = _C._out((N, P, 3), dtype=torch.float32, device=dev)
    curvature = _C._out((N, P), dtype=torch.float32, device=dev)
    num_neighbors = _C._out((N, P), dtype=torch.int64, device=dev)
    status = _C._out((N, P), dtype=torch.uint8, device=dev)
    moments = _C._out((N, P, MLS_MOMENTS), dtype=torch.int64, device=dev) if want_moments else None
    sizer = _C._lib.pointops_mls_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P, int(iterations))
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.mls_smooth("mls_smooth", dev, r(points), r(lengths), n, P, float(radius), int(min_neighbors),
                            int(iterations), r(smoothed), r(normals), r(curvature), r(num_neighbors), r(status),
                            r(moments), workspace, sizer(n, P, int(iterations)))
    return smoothed, normals, curvature, num_neighbors, status, moments
