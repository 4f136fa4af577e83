"""Operator boundary of match_features (csrc/feature_match.hip; C ABI: pointops_feature_knn,
pointops_feature_knn_workspace_bytes and pointops_feature_screen_values in include/pointops_amd.h, whose FEATURE
MATCHING block is the definition).

Beside `_C.py`, not in it, as `_C_knn_in_radius.py` is: an eager-only building block of functions/match.py, not a
registered operator.  Everything it uses is `_C`'s -- the argument normalisers, the native-call namespace and the output
seam -- looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees these calls too.  There is
no CPU implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

MAX_K = 2
SCREEN_VALUES_MAX_POINTS = 1024
SCREEN_VALUES_MAX_D = 128


def _pair(what, p1, p2, lengths1, lengths2):
    dev = _C._require_gpu(p1, p2, lengths1, lengths2)
    same = p1 is p2
    p1 = _C._f32c(p1, "p1")
    p2 = p1 if same else _C._f32c(p2, "p2")
    lengths1, lengths2 = _C._i64c(lengths1, "lengths1"), _C._i64c(lengths2, "lengths2")
    if p1.dim() != 3 or p2.dim() != 3:
        raise RuntimeError(f"{what}: p1 and p2 must be 3-dimensional")
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    if p2.shape[0] != N or p2.shape[2] != D or D < 1:
        raise RuntimeError(f"{what}: need p1 (N,P1,D) and p2 (N,P2,D) with D >= 1")
    if lengths1 is None or lengths2 is None or lengths1.shape != (N,) or lengths2.shape != (N,):
        raise RuntimeError(f"{what}: need lengths (N,)")
    return dev, p1, p2, lengths1, lengths2, N, P1, P2, D


def feature_knn(p1, p2, lengths1, lengths2, K: int):
    """p1 (N,P1,D), p2 (N,P2,D) fp32, any D; lengths (N,) int64; K in {1, 2} ->
    (idx (N,P1,K) int64, dists (N,P1,K) fp32, stats (N,4) int32): `_C.knn_points_idx(..., norm=2, K)` byte for byte, and
    per cloud whether the screen ran, the rows it certified, the rows it sent to the exact kernel and a reserved 0."""
    dev, p1, p2, lengths1, lengths2, N, P1, P2, D = _pair("feature_knn", p1, p2, lengths1, lengths2)
    K = int(K)
    if not 1 <= K <= MAX_K:
        raise RuntimeError(f"feature_knn: need 1 <= K <= {MAX_K}")
    idx = _C._out((N, P1, K), dtype=torch.int64, device=dev)
    dists = _C._out((N, P1, K), dtype=torch.float32, device=dev)
    stats = _C._out((N, 4), dtype=torch.int32, device=dev)
    sizer = _C._lib.pointops_feature_knn_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), P1, P2, D, K)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.feature_knn("feature_knn", dev, r(p1), r(p2), r(lengths1), r(lengths2), n, P1, P2, D, K, r(idx),
                             r(dists), r(stats), workspace, sizer(n, P1, P2, D, K))
    return idx, dists, stats


def feature_screen_values(p1, p2, lengths1, lengths2):
    """Test support: (s (N,P1,P2), n1 (N,P1), n2 (N,P2), n2max (N,), E (N,P1)) fp32 as the screen of feature_knn computes
    them, from the same tile code; P1, P2 in 1..1024, D <= 128, N < 65536."""
    dev, p1, p2, lengths1, lengths2, N, P1, P2, D = _pair("feature_screen_values", p1, p2, lengths1, lengths2)
    if not (1 <= P1 <= SCREEN_VALUES_MAX_POINTS and 1 <= P2 <= SCREEN_VALUES_MAX_POINTS and D <= SCREEN_VALUES_MAX_D
            and N <= _C.ALIGNMENT_MAX_CLOUDS):
        raise RuntimeError("feature_screen_values: need 1 <= P1, P2 <= 1024, D <= 128 and N < 65536")
    out = [_C._out(shape, dtype=torch.float32, device=dev) for shape in ((N, P1, P2), (N, P1), (N, P2), (N,), (N, P1))]
    _C._call.feature_screen_values("feature_screen_values", dev, p1, p2, lengths1, lengths2, N, P1, P2, D, *out)
    return tuple(out)
