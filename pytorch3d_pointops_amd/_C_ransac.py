"""Operator boundary of the robust registration (csrc/ransac.hip; C ABI: pointops_ransac_alignment in
include/pointops_amd.h).

The wrapper lives beside `_C.py`, not in it, as `_C_descriptors.py` does: an eager-only building block of
functions/ransac.py, not a registered operator.  Everything it uses is `_C`'s -- the argument normalisers, the
native-call namespace and the output seam -- looked up on the module at call time, so whatever patches `_C._out` or
`_C._call` sees this call too.  There is no CPU implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

# records one scoring workgroup walks: a cloud's valid pairs are scored in chunks of this many
RANSAC_CHUNK = int(_C._lib.pointops_ransac_chunk())
RANSAC_MAX_HYPOTHESES = 1 << 24


def ransac_alignment(X, Y, corr, lengths1, lengths2, samples, H: int, seed: int, inlier_threshold: float,
                     edge_length_ratio: float, estimate_scale: bool, refine_steps: int, want_hypotheses: bool = False):
    """X (N,P1,3), Y (N,P2,3) fp32; corr (N,P1) int64 or None (row i <-> row i); lengths1, lengths2 (N,) or None;
    samples (N,H,3) int64 or None (drawn) ->
    (R (N,3,3), T (N,3), s (N,), mask (N,P1) bool, num_inliers (N,) int64, rmse (N,), best (N,) int64, counts (N,H)
    int32, hyp_R (N,H,3,3), hyp_T (N,H,3), hyp_s (N,H), samples (N,H,3) int64); the last five are None without
    `want_hypotheses`."""
    dev = _C._require_gpu(X, Y, corr, lengths1, lengths2, samples)
    X, Y = _C._f32c(X, "X"), _C._f32c(Y, "Y")
    corr, samples = _C._i64c(corr, "corr"), _C._i64c(samples, "samples")
    lengths1, lengths2 = _C._i64c(lengths1, "lengths1"), _C._i64c(lengths2, "lengths2")
    H = int(H)
    if X.dim() != 3 or Y.dim() != 3 or X.shape[2] != 3 or Y.shape[2] != 3 or Y.shape[0] != X.shape[0]:
        raise RuntimeError("ransac_alignment: need X (N,P1,3) and Y (N,P2,3)")
    N, P1, P2 = X.shape[0], X.shape[1], Y.shape[1]
    if ((corr is None and P2 != P1) or (corr is not None and corr.shape != (N, P1))
            or (lengths1 is not None and lengths1.shape != (N,)) or (lengths2 is not None and lengths2.shape != (N,))
            or (samples is not None and samples.shape != (N, H, 3)) or not 1 <= H <= RANSAC_MAX_HYPOTHESES):
        raise RuntimeError("ransac_alignment: need corr (N,P1) (or P2 == P1), lengths (N,), samples (N,H,3) and "
                           f"1 <= H <= {RANSAC_MAX_HYPOTHESES}")
    R = _C._out((N, 3, 3), dtype=torch.float32, device=dev)
    T = _C._out((N, 3), dtype=torch.float32, device=dev)
    s = _C._out((N,), dtype=torch.float32, device=dev)
    mask = _C._out((N, P1), dtype=torch.bool, device=dev)
    num_inliers = _C._out((N,), dtype=torch.int64, device=dev)
    rmse = _C._out((N,), dtype=torch.float32, device=dev)
    best = _C._out((N,), dtype=torch.int64, device=dev)
    counts = hyp_R = hyp_T = hyp_s = samples_out = None
    if want_hypotheses:
        counts = _C._out((N, H), dtype=torch.int32, device=dev)
        hyp_R = _C._out((N, H, 3, 3), dtype=torch.float32, device=dev)
        hyp_T = _C._out((N, H, 3), dtype=torch.float32, device=dev)
        hyp_s = _C._out((N, H), dtype=torch.float32, device=dev)
        samples_out = _C._out((N, H, 3), dtype=torch.int64, device=dev)
    scratch = _C._scratch(dev, _C._lib.pointops_ransac_workspace_bytes, min(N, _C.ALIGNMENT_MAX_CLOUDS), P1, H)
    first = 0
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        _C._call.ransac_alignment("ransac_alignment", dev, r(X), r(Y), r(corr), r(lengths1), r(lengths2), r(samples),
                                  n, P1, P2, H, int(seed), first, float(inlier_threshold), float(edge_length_ratio),
                                  bool(estimate_scale), int(refine_steps), r(R), r(T), r(s), r(mask), r(num_inliers),
                                  r(rmse), r(best), r(counts), r(hyp_R), r(hyp_T), r(hyp_s), r(samples_out), *scratch)
        first += n
    return R, T, s, mask, num_inliers, rmse, best, counts, hyp_R, hyp_T, hyp_s, samples_out
