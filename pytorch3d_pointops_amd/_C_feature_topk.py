"""Operator boundary of knn_features (csrc/feature_topk.hip; C ABI: pointops_feature_topk and
pointops_feature_topk_workspace_bytes in include/pointops_amd.h, whose FEATURE TOP-K block is the definition).

Beside `_C.py`, not in it, as `_C_match.py` is, and with the same seams: the argument normalisers, the native-call
namespace and the output seam are `_C`'s, looked up on the module at call time, so whatever patches `_C._out` or
`_C._call` sees these calls too.  There is no CPU implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C
from ._C_match import _pair

SCREEN_MAX_D = 128
SCREEN_MAX_K = 32


def feature_topk(p1, p2, lengths1, lengths2, K: int):
    """p1 (N,P1,D), p2 (N,P2,D) fp32, any D; lengths (N,) int64; K >= 1 ->
    (idx (N,P1,K) int64, dists (N,P1,K) fp32, stats (N,4) int32): `_C.knn_points_idx(..., norm=2, K)` byte for byte, and
    per cloud whether the screen ran, the rows it certified, the rows it sent to the exact kernel and the key lists per
    query (2 S; 0 when not screened)."""
    dev, p1, p2, lengths1, lengths2, N, P1, P2, D = _pair("feature_topk", p1, p2, lengths1, lengths2)
    K = int(K)
    if K < 1:
        raise RuntimeError("feature_topk: need K >= 1")
    idx = _C._out((N, P1, K), dtype=torch.int64, device=dev)
    dists = _C._out((N, P1, K), dtype=torch.float32, device=dev)
    stats = _C._out((N, 4), dtype=torch.int32, device=dev)
    sizer = _C._lib.pointops_feature_topk_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P1, P2, D, K)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.feature_topk("feature_topk", dev, r(p1), r(p2), r(lengths1), r(lengths2), n, P1, P2, D, K, r(idx),
                              r(dists), r(stats), workspace, sizer(n, P1, P2, D, K))
    return idx, dists, stats
