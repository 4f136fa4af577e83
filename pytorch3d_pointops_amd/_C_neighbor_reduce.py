"""Operator boundary of neighbor_reduce (csrc/neighbor_reduce.hip; C ABI: pointops_neighbor_reduce,
pointops_neighbor_reduce_backward and its workspace sizer in include/pointops_amd.h, whose NEIGHBOUR REDUCE block is the
definition).

Beside `_C.py`, not in it, as `_C_feature_topk.py` is, and with the same seams: the argument normalisers, the native-call
namespace and the output seam are `_C`'s, looked up on the module at call time, so whatever patches `_C._out` or
`_C._call` sees these calls too.  There is no CPU implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

REDUCE = {"sum": 0, "mean": 1, "max": 2}
MAX_K = 255  # `max`: the winning slot is a byte, 255 = none


def _rows16(t, name):
    """fp32 + contiguous + 16-byte aligned: the kernels move rows of C % 4 == 0 channels 16 bytes at a time (a view at an
    odd storage offset is copied)."""
    t = _C._f32c(t, name)
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def _args(what, x, idx, lengths, weights, reduce):
    dev = _C._require_gpu(x, idx, lengths, weights)
    x, weights = _rows16(x, "x"), _C._f32c(weights, "weights")
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    if reduce not in REDUCE:
        raise RuntimeError(f"{what}: reduce must be one of {sorted(REDUCE)}")
    if x.dim() != 3 or idx.dim() != 3 or idx.shape[0] != x.shape[0] or x.shape[2] < 1:
        raise RuntimeError(f"{what}: need x (N,M,C) with C >= 1 and idx (N,L,K)")
    N, M, C = x.shape
    _, L, K = idx.shape
    if (lengths is not None and lengths.shape != (N,)) or (weights is not None and weights.shape != idx.shape):
        raise RuntimeError(f"{what}: need lengths (N,) and weights (N,L,K)")
    if weights is not None and reduce != "sum":
        raise RuntimeError(f"{what}: weights go with reduce='sum' only")
    if reduce == "max" and K > MAX_K:
        raise RuntimeError(f"{what}: reduce='max' takes K <= {MAX_K}")
    return dev, x, idx, lengths, weights, N, M, C, L, K


def neighbor_reduce(x, idx, lengths=None, weights=None, reduce: str = "max"):
    """x (N,M,C) fp32, idx (N,L,K) int64, lengths (N,) int64 or None, weights (N,L,K) fp32 or None (sum only) ->
    (out (N,L,C) fp32, arg (N,L,C) uint8 for max, else None)."""
    dev, x, idx, lengths, weights, N, M, C, L, K = _args("neighbor_reduce", x, idx, lengths, weights, reduce)
    out = _C._out((N, L, C), dtype=torch.float32, device=dev)
    arg = _C._out((N, L, C), dtype=torch.uint8, device=dev) if reduce == "max" else None
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        _C._call.neighbor_reduce("neighbor_reduce", dev, r(x), r(idx), r(lengths), r(weights), n, M, C, L, K,
                                 REDUCE[reduce], r(out), r(arg))
    return out, arg


def neighbor_reduce_backward(grad_out, x, idx, lengths, weights, arg, reduce: str, need_x: bool = True,
                             need_w: bool = False):
    """grad_out (N,L,C) -> (grad_x (N,M,C) or None, grad_w (N,L,K) or None): the pull backward, one path, no atomics."""
    dev, x, idx, lengths, weights, N, M, C, L, K = _args("neighbor_reduce_backward", x, idx, lengths, weights, reduce)
    _C._require_gpu(grad_out, arg)
    grad_out = _rows16(grad_out, "grad_out")
    if grad_out.shape != (N, L, C) or (reduce == "max") != (arg is not None) or (need_w and weights is None):
        raise RuntimeError("neighbor_reduce_backward: need grad_out (N,L,C), arg for max only, weights for grad_w")
    if arg is not None and (arg.dtype != torch.uint8 or arg.shape != (N, L, C)):
        raise RuntimeError("neighbor_reduce_backward: arg must be the forward's (N,L,C) uint8")
    arg = _C._contig(arg, "arg") if arg is not None else None
    grad_x = _C._out((N, M, C), dtype=torch.float32, device=dev) if need_x else None
    grad_w = _C._out((N, L, K), dtype=torch.float32, device=dev) if need_w else None
    sizer = _C._lib.pointops_neighbor_reduce_backward_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), L, K, M)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.neighbor_reduce_backward("neighbor_reduce_backward", dev, r(grad_out), r(x), r(idx), r(lengths),
                                          r(weights), r(arg), n, M, C, L, K, REDUCE[reduce], r(grad_x), r(grad_w),
                                          workspace, sizer(n, L, K, M))
    return grad_x, grad_w
