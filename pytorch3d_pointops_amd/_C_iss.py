"""Operator boundary of the ISS keypoint detector (csrc/iss.hip; C ABI: pointops_iss_keypoints in
include/pointops_amd.h).

Beside `_C.py`, not in it, as `_C_cluster.py` is: an eager-only building block of functions/iss.py, not a registered
operator.  Everything it uses is `_C`'s -- the argument normalisers, the native-call namespace and the output seam --
looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees this call too.  There is no CPU
implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

ISS_MOMENTS = 10  # n, M1[3], M2[6] (xx, xy, xz, yy, yz, zz)


def iss_keypoints(points, lengths, salient_radius: float, non_max_radius: float, gamma_21: float, gamma_32: float,
                  min_neighbors: int, want_moments: bool = False):
    """points (N,P,3) fp32; lengths (N,) int64 or None ->
    (mask (N,P) bool, saliency (N,P) fp32, eigenvalues (N,P,3) fp32, moments (N,P,10) int64 or None)."""
    dev = _C._require_gpu(points, lengths)
    points, lengths = _C._f32c(points, "points"), _C._i64c(lengths, "lengths")
    if points.dim() != 3 or points.shape[2] != 3:
        raise RuntimeError("iss_keypoints: need points (N,P,3)")
    N, P, _ = points.shape
    if lengths is not None and lengths.shape != (N,):
        raise RuntimeError("iss_keypoints: need lengths (N,)")
    eigenvalues = _C._out((N, P, 3), dtype=torch.float32, device=dev)
    saliency = _C._out((N, P), dtype=torch.float32, device=dev)
    mask = _C._out((N, P), dtype=torch.bool, device=dev)
    moments = _C._out((N, P, ISS_MOMENTS), dtype=torch.int64, device=dev) if want_moments else None
    sizer = _C._lib.pointops_iss_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.iss_keypoints("iss_keypoints", dev, r(points), r(lengths), n, P, float(salient_radius),
                               float(non_max_radius), float(gamma_21), float(gamma_32), int(min_neighbors),
                               r(eigenvalues), r(saliency), r(mask), r(moments), workspace, sizer(n, P))
    return mask, saliency, eigenvalues, moments
