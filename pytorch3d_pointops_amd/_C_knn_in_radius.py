"""Operator boundary of knn_in_radius (csrc/knn_in_radius.hip; C ABI: pointops_knn_in_radius and
pointops_knn_in_radius_workspace_bytes in include/pointops_amd.h, whose KNN IN RADIUS block is the definition).

Beside `_C.py`, not in it, as `_C_filters.py` is: an eager-only building block of functions/knn_in_radius.py, not a
registered operator.  Everything it uses is `_C`'s -- the argument normalisers, the native-call namespace and the output
seam -- looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees these calls too.  There is
no CPU implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

MAX_K = 64  # the fused path's longest list
MAX_D = 3


def knn_in_radius(p1, p2, lengths1, lengths2, K: int, radius: float, workspace=None, reuse: bool = False):
    """p1 (N,P1,D), p2 (N,P2,D) fp32, D in 1..3; lengths (N,) int64 or None; 1 <= K <= 64 ->
    (idx (N,P1,K) int64 padded with -1, dists (N,P1,K) fp32 padded with 0, counts (N,P1) int32, workspace).

    `workspace`: the uint8 tensor an earlier call of the same shape returned, or None for a fresh one.  `reuse=True`:
    the caller vouches that p2, lengths2 and the shape are those of the previous call into `workspace`; only the query
    side of the search structure is rebuilt.  Batches above 65535 clouds go in slices that share one workspace, so
    they cannot reuse."""
    dev = _C._require_gpu(p1, p2, lengths1, lengths2)
    same = p1 is p2
    p1 = _C._f32c(p1, "p1")
    p2 = p1 if same else _C._f32c(p2, "p2")
    lengths1, lengths2 = _C._i64c(lengths1, "lengths1"), _C._i64c(lengths2, "lengths2")
    if p1.dim() != 3 or p2.dim() != 3:
        raise RuntimeError("knn_in_radius: p1 and p2 must be 3-dimensional")
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    if p2.shape[0] != N or p2.shape[2] != D or not 1 <= D <= MAX_D:
        raise RuntimeError(f"knn_in_radius: need p1 (N,P1,D) and p2 (N,P2,D) with D in 1..{MAX_D}")
    if any(l is not None and l.shape != (N,) for l in (lengths1, lengths2)):
        raise RuntimeError("knn_in_radius: need lengths (N,)")
    K = int(K)
    if not 1 <= K <= MAX_K:
        raise RuntimeError(f"knn_in_radius: need 1 <= K <= {MAX_K}")
    idx = _C._out((N, P1, K), dtype=torch.int64, device=dev)
    dists = _C._out((N, P1, K), dtype=torch.float32, device=dev)
    counts = _C._out((N, P1), dtype=torch.int32, device=dev)
    sizer = _C._lib.pointops_knn_in_radius_workspace_bytes
    slices = list(_C._cloud_slices(N))
    if reuse and (workspace is None or len(slices) > 1):
        raise RuntimeError("knn_in_radius: reuse needs the workspace of the previous call, and a batch of one slice")
    need = sizer(min(N, _C.ALIGNMENT_MAX_CLOUDS), P1, P2, D, K)
    if workspace is None:
        workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P1, P2, D, K)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or workspace.numel() < need:
        raise RuntimeError(f"knn_in_radius: workspace must be a uint8 tensor of at least {need} bytes on the inputs' "
                           "device")
    for sl, n in slices:
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.knn_in_radius("knn_in_radius", dev, r(p1), r(p2), r(lengths1), r(lengths2), n, P1, P2, D, K,
                               float(radius), r(idx), r(dists), r(counts), workspace, sizer(n, P1, P2, D, K),
                               1 if reuse else 0)
    return idx, dists, counts, workspace
