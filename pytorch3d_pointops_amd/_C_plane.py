"""Operator boundary of the plane extraction (csrc/plane.hip; C ABI: pointops_segment_plane in
include/pointops_amd.h).

Beside `_C.py`, not in it, as `_C_ransac.py` is: an eager-only building block of functions/plane.py, not a registered
operator.  Everything it uses is `_C`'s -- the argument normalisers, the native-call namespace and the output seam --
looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees this call too.  There is no CPU
implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

# records one scoring workgroup walks: a cloud's valid rows are scored in chunks of this many
PLANE_CHUNK = int(_C._lib.pointops_plane_chunk())
PLANE_MAX_HYPOTHESES = 1 << 24


def segment_plane(points, lengths, mask, samples, H: int, seed: int, distance_threshold: float, axis, cos_max_angle,
                  refine_steps: int, want_hypotheses: bool = False):
    """points (N,P,3) fp32; lengths (N,) int64 or None; mask (N,P) bool or None; samples (N,H,3) int64 or None (drawn);
    axis: three floats of unit length with cos_max_angle in [0,1], or None ->
    (planes (N,4), mask (N,P) bool, num_inliers (N,) int64, rmse (N,), best (N,) int64, counts (N,H) int32,
    hyp_planes (N,H,4), samples (N,H,3) int64); the last three are None without `want_hypotheses`."""
    dev = _C._require_gpu(points, lengths, mask, samples)
    points = _C._f32c(points, "points")
    lengths, samples = _C._i64c(lengths, "lengths"), _C._i64c(samples, "samples")
    if mask is not None:
        if mask.dtype != torch.bool:
            raise RuntimeError("mask must be bool")
        mask = mask.contiguous()
    H = int(H)
    if points.dim() != 3 or points.shape[2] != 3:
        raise RuntimeError("segment_plane: need points (N,P,3)")
    N, P = points.shape[0], points.shape[1]
    if ((lengths is not None and lengths.shape != (N,)) or (mask is not None and mask.shape != (N, P))
            or (samples is not None and samples.shape != (N, H, 3)) or not 1 <= H <= PLANE_MAX_HYPOTHESES):
        raise RuntimeError("segment_plane: need lengths (N,), mask (N,P), samples (N,H,3) and "
                           f"1 <= H <= {PLANE_MAX_HYPOTHESES}")
    use_axis = axis is not None
    ax, ay, az = (float(a) for a in axis) if use_axis else (0.0, 0.0, 0.0)
    cosm = float(cos_max_angle) if use_axis else 0.0
    planes = _C._out((N, 4), dtype=torch.float32, device=dev)
    inliers = _C._out((N, P), dtype=torch.bool, device=dev)
    num_inliers = _C._out((N,), dtype=torch.int64, device=dev)
    rmse = _C._out((N,), dtype=torch.float32, device=dev)
    best = _C._out((N,), dtype=torch.int64, device=dev)
    counts = hyp_planes = samples_out = None
    if want_hypotheses:
        counts = _C._out((N, H), dtype=torch.int32, device=dev)
        hyp_planes = _C._out((N, H, 4), dtype=torch.float32, device=dev)
        samples_out = _C._out((N, H, 3), dtype=torch.int64, device=dev)
    scratch = _C._scratch(dev, _C._lib.pointops_plane_workspace_bytes, min(N, _C.ALIGNMENT_MAX_CLOUDS), P, H)
    first = 0
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        _C._call.segment_plane("segment_plane", dev, r(points), r(lengths), r(mask), r(samples), n, P, H, int(seed),
                               first, float(distance_threshold), use_axis, ax, ay, az, cosm, int(refine_steps),
                               r(planes), r(inliers), r(num_inliers), r(rmse), r(best), r(counts), r(hyp_planes),
                               r(samples_out), *scratch)
        first += n
    return planes, inliers, num_inliers, rmse, best, counts, hyp_planes, samples_out
