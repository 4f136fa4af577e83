"""Operator boundary of neighbor_attention (csrc/neighbor_attention.hip; C ABI: pointops_neighbor_attention,
pointops_neighbor_attention_backward and its workspace sizer in include/pointops_amd.h, whose NEIGHBOUR ATTENTION block is
the definition).

Beside `_C.py`, not in it, as `_C_neighbor_reduce.py` is, and with the same seams: the argument normalisers, the
native-call namespace and the output seam are `_C`'s, looked up on the module at call time, so whatever patches `_C._out`
or `_C._call` sees these calls too.  There is no CPU implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

HEAD_DIMS = (4, 8, 16, 32, 64, 128, 256)  # a head is D / 4 lanes, at most a wave
MAX_C = 1 << 16


def supported(N, L, M, K, heads, D):
    """The sizes the native entries take (na_sizes_ok of csrc/neighbor_attention.hip)."""
    return D in HEAD_DIMS and heads * D <= MAX_C and N * L * K * heads < 2 ** 31 and N * M < 2 ** 31 - 1


def _rows16(t, name):
    """fp32 + contiguous + 16-byte aligned: the kernels move rows 16 bytes at a time (a view at an odd storage offset
    is copied)."""
    t = _C._f32c(t, name)
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def _args(what, q, k, v, idx, lengths, bias, heads):
    dev = _C._require_gpu(q, k, v, idx, lengths, bias)
    q, k, v, bias = _rows16(q, "q"), _rows16(k, "k"), _rows16(v, "v"), _C._f32c(bias, "bias")
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    heads = int(heads)
    if q.dim() != 3 or k.dim() != 3 or idx.dim() != 3 or v.shape != k.shape or k.shape[0] != q.shape[0] \
            or k.shape[2] != q.shape[2] or idx.shape[:2] != q.shape[:2]:
        raise RuntimeError(f"{what}: need q (N,L,C), k and v (N,M,C) and idx (N,L,K)")
    N, L, C = q.shape
    M, K = k.shape[1], idx.shape[2]
    if heads < 1 or C % heads or C // heads not in HEAD_DIMS or C > MAX_C:
        raise RuntimeError(f"{what}: need C = heads * D with D in {HEAD_DIMS} and C <= {MAX_C}")
    if (lengths is not None and lengths.shape != (N,)) or (bias is not None and bias.shape != (N, L, K, heads)):
        raise RuntimeError(f"{what}: need lengths (N,) and bias (N,L,K,heads)")
    return dev, q, k, v, idx, lengths, bias, N, L, M, K, heads, C // heads


def neighbor_attention(q, k, v, idx, lengths=None, bias=None, heads: int = 1, scale: float = 1.0):
    """q (N,L,C), k and v (N,M,C) fp32, idx (N,L,K) int64, lengths (N,) int64 or None, bias (N,L,K,heads) fp32 or None
    -> (out (N,L,C) fp32, lse (N,L,heads) fp32)."""
    dev, q, k, v, idx, lengths, bias, N, L, M, K, heads, D = _args("neighbor_attention", q, k, v, idx, lengths, bias,
                                                                   heads)
    out = _C._out((N, L, heads * D), dtype=torch.float32, device=dev)
    lse = _C._out((N, L, heads), dtype=torch.float32, device=dev)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        _C._call.neighbor_attention("neighbor_attention", dev, r(q), r(k), r(v), r(idx), r(lengths), r(bias), n, L, M, K,
                                    heads, D, float(scale), r(out), r(lse))
    return out, lse


def neighbor_attention_backward(grad_out, q, k, v, out, lse, idx, lengths, bias, heads: int, scale: float,
                                need=(True, True, True, False)):
    """grad_out (N,L,C) and the forward's out, lse -> (grad_q, grad_k, grad_v, grad_bias), None where `need` is False:
    one path, no atomics."""
    dev, q, k, v, idx, lengths, bias, N, L, M, K, heads, D = _args("neighbor_attention_backward", q, k, v, idx, lengths,
                                                                   bias, heads)
    _C._require_gpu(grad_out, out, lse)
    grad_out, out, lse = _rows16(grad_out, "grad_out"), _rows16(out, "out"), _C._f32c(lse, "lse")
    if grad_out.shape != q.shape or out.shape != q.shape or lse.shape != (N, L, heads) or (need[3] and bias is None):
        raise RuntimeError("neighbor_attention_backward: need grad_out and out (N,L,C), lse (N,L,heads), bias for its "
                           "gradient")
    shapes = (q.shape, k.shape, v.shape, (N, L, K, heads))
    grads = [_C._out(tuple(s), dtype=torch.float32, device=dev) if w else None for s, w in zip(shapes, need)]
    sizer = _C._lib.pointops_neighbor_attention_backward_workspace_bytes
    workspace, _ = _C._scratch(dev, sizer, min(N, _C.ALIGNMENT_MAX_CLOUDS), L, K, M, heads)
    for sl, n in _C._cloud_slices(N):
        r = lambda t: _C._rows(t, sl)  # noqa: E731
        # (a slice is told the bytes IT needs of the one workspace, sized for the largest slice)
        _C._call.neighbor_attention_backward("neighbor_attention_backward", dev, r(grad_out), r(q), r(k), r(v), r(out),
                                             r(lse), r(idx), r(lengths), r(bias), n, L, M, K, heads, D, float(scale),
                                             *[r(t) for t in grads], workspace, sizer(n, L, K, M, heads))
    return tuple(grads)
