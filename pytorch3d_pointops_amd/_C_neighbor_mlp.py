"""Operator boundary of neighbor_mlp_max (csrc/neighbor_mlp.hip; C ABI: pointops_neighbor_mlp_max,
pointops_neighbor_mlp_max_backward and its workspace sizer in include/pointops_amd.h, whose NEIGHBOUR MLP-MAX block is the
definition) and of its bfloat16 / float16 form (csrc/neighbor_mlp16.hip; pointops_neighbor_mlp_max16,
pointops_neighbor_mlp_max16_backward and their workspace sizers), and of the 16-bit form with a second hidden layer
(csrc/neighbor_mlp2_16.hip; pointops_neighbor_mlp2_max16, pointops_neighbor_mlp2_max16_backward and their sizers).

Beside `_C.py`, not in it, as `_C_neighbor_conv.py` is, and with the same seams: the argument normalisers, the
native-call namespace and the output seam are `_C`'s, looked up on the module at call time, so whatever patches `_C._out`
or `_C._call` sees these calls too.  There is no CPU implementation: CPU tensors raise RuntimeError.
"""
import os

import torch

from . import _C
from ._C_neighbor_attention import _rows16
from ._C_neighbor_conv import DTYPES16, _t16c

MAX_C, MAX_K = 128, 255
MAX_C16 = 256


def supported(N, L, M, K, C1, C2):
    """The sizes the native entries take (nm_sizes_ok of csrc/neighbor_mlp.hip)."""
    return (all(4 <= c <= MAX_C and c % 4 == 0 for c in (C1, C2)) and 1 <= K <= MAX_K
            and N * L * K < 2 ** 31 and N * M < 2 ** 31 - 1)


def forced():
    """POINTOPS_DEBUG=neighbor_mlp=0|1 (csrc/debug.h's switchboard): False = the torch route, True = the HIP path
    whenever the tensors are float32 GPU tensors, or GPU tensors whose x is bfloat16 or float16 (sizes it does not take
    are then an error), None = by `supported` / `supported16` / `supported2_16`."""
    for item in os.environ.get("POINTOPS_DEBUG", "").split(","):
        key, _, value = item.partition("=")
        if key.strip() == "neighbor_mlp" and value.strip() in ("0", "1"):
            return value.strip() == "1"
    return None


def _args(what, x, idx, weight, bias, center, lengths):
    dev = _C._require_gpu(x, idx, weight, bias, center, lengths)
    x, center = _rows16(x, "x"), _rows16(center, "center")
    weight, bias = _C._f32c(weight, "weight"), _C._f32c(bias, "bias")
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    if x.dim() != 3 or idx.dim() != 3 or weight.dim() != 2 or idx.shape[0] != x.shape[0] \
            or weight.shape[0] != x.shape[2]:
        raise RuntimeError(f"{what}: need x (N,M,C1), idx (N,L,K) and weight (C1,C2)")
    (N, M, C1), (_, L, K), C2 = x.shape, idx.shape, weight.shape[1]
    if (lengths is not None and lengths.shape != (N,)) or (bias is not None and bias.shape != (C2,)) \
            or (center is not None and center.shape != (N, L, C1)):
        raise RuntimeError(f"{what}: need lengths (N,), bias (C2,) and center (N,L,C1)")
    if not supported(N, L, M, K, C1, C2):
        raise RuntimeError(f"{what}: need C1 and C2 multiples of 4 in [4, {MAX_C}] and 1 <= K <= {MAX_K}")
    return dev, x, idx, weight, bias, center, lengths, N, L, M, K, C1, C2


def neighbor_mlp_max(x, idx, weight, bias=None, center=None, lengths=None, relu_out=True):
    """x (N,M,C1) fp32, idx (N,L,K) int64, weight (C1,C2) fp32, bias (C2,), center (N,L,C1) fp32 or None, lengths (N,)
    int64 or None -> (out (N,L,C2) fp32, arg (N,L,C2) uint8)."""
    dev, x, idx, weight, bias, center, lengths, N, L, M, K, C1, C2 = _args("neighbor_mlp_max", x, idx, weight, bias,
                                                                          center, lengths)
    out = _C._out((N, L, C2), dtype=torch.float32, device=dev)
    arg = _C._out((N, L, C2), dtype=torch.uint8, device=dev)
    _C._call.neighbor_mlp_max("neighbor_mlp_max", dev, x, idx, lengths, center, weight, bias, N, L, M, K, C1, C2,
                              bool(relu_out), out, arg)
    return out, arg


def neighbor_mlp_max_backward(grad_out, x, idx, weight, center, lengths, out, arg, relu_out=True,
                              need=(True, True, True, True)):
    """grad_out (N,L,C2) and the forward's out, arg -> (grad_x, grad_center, grad_weight, grad_bias), None where `need`
    is False: one path, no atomics."""
    dev, x, idx, weight, _, center, lengths, N, L, M, K, C1, C2 = _args("neighbor_mlp_max_backward", x, idx, weight, None,
                                                                        center, lengths)
    _C._require_gpu(grad_out, out, arg)
    grad_out, out = _rows16(grad_out, "grad_out"), _rows16(out, "out")
    if grad_out.shape != (N, L, C2) or out.shape != (N, L, C2) or (need[1] and center is None):
        raise RuntimeError("neighbor_mlp_max_backward: need grad_out and out (N,L,C2), center for its gradient")
    if arg.dtype != torch.uint8 or arg.shape != (N, L, C2):
        raise RuntimeError("neighbor_mlp_max_backward: arg must be the forward's (N,L,C2) uint8")
    arg = _C._contig(arg, "arg")
    shapes = (x.shape, (N, L, C1), weight.shape, (C2,))
    grads = [_C._out(tuple(s), dtype=torch.float32, device=dev) if w else None for s, w in zip(shapes, need)]
    _C._call.neighbor_mlp_max_backward(
        "neighbor_mlp_max_backward", dev, grad_out, x, idx, lengths, center, weight, out, arg, N, L, M, K, C1, C2,
        bool(relu_out), *grads,
        *_C._scratch(dev, _C._lib.pointops_neighbor_mlp_max_backward_workspace_bytes, N, L, K, M, C1, C2))
    return tuple(grads)


def supported16(N, L, M, K, C1, C2):
    """The sizes the 16-bit entries take (nm16_sizes_ok of csrc/neighbor_mlp16.hip)."""
    return (all(8 <= c <= MAX_C16 and c % 8 == 0 for c in (C1, C2)) and 1 <= K <= MAX_K
            and N * L * K < 2 ** 31 and N * M < 2 ** 31 - 1)


def _args16(what, x, idx, weight, bias, center, lengths):
    dev = _C._require_gpu(x, idx, weight, bias, center, lengths)
    if x.dtype not in DTYPES16:
        raise RuntimeError(f"{what}: x must be bfloat16 or float16")
    dt = x.dtype
    x, center = _t16c(x, "x", dt, rows=True), _t16c(center, "center", dt, rows=True)
    weight, bias = _t16c(weight, "weight", dt), _t16c(bias, "bias", dt)
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    if x.dim() != 3 or idx.dim() != 3 or weight.dim() != 2 or idx.shape[0] != x.shape[0] \
            or weight.shape[0] != x.shape[2]:
        raise RuntimeError(f"{what}: need x (N,M,C1), idx (N,L,K) and weight (C1,C2)")
    (N, M, C1), (_, L, K), C2 = x.shape, idx.shape, weight.shape[1]
    if (lengths is not None and lengths.shape != (N,)) or (bias is not None and bias.shape != (C2,)) \
            or (center is not None and center.shape != (N, L, C1)):
        raise RuntimeError(f"{what}: need lengths (N,), bias (C2,) and center (N,L,C1)")
    if not supported16(N, L, M, K, C1, C2):
        raise RuntimeError(f"{what}: need C1 and C2 multiples of 8 in [8, {MAX_C16}] and 1 <= K <= {MAX_K}")
    return dev, dt, x, idx, weight, bias, center, lengths, N, L, M, K, C1, C2


def neighbor_mlp_max16(x, idx, weight, bias=None, center=None, lengths=None, relu_out=True):
    """neighbor_mlp_max for T = bfloat16 or float16: x (N,M,C1), weight (C1,C2), bias (C2,) and center (N,L,C1) or None
    of T -> (out (N,L,C2) of T, arg (N,L,C2) uint8), accumulated in fp32 on the 16-deep matrix instructions."""
    dev, dt, x, idx, weight, bias, center, lengths, N, L, M, K, C1, C2 = _args16("neighbor_mlp_max16", x, idx, weight,
                                                                                bias, center, lengths)
    out = _C._out((N, L, C2), dtype=dt, device=dev)
    arg = _C._out((N, L, C2), dtype=torch.uint8, device=dev)
    _C._call.neighbor_mlp_max16(
        "neighbor_mlp_max16", dev, x, idx, lengths, center, weight, bias, DTYPES16[dt], N, L, M, K, C1, C2,
        bool(relu_out), out, arg,
        *_C._scratch(dev, _C._lib.pointops_neighbor_mlp_max16_workspace_bytes, N, L, K, M, C1, C2))
    return out, arg


def neighbor_mlp_max16_backward(grad_out, x, idx, weight, center, lengths, out, arg, relu_out=True,
                                need=(True, True, True, True)):
    """grad_out (N,L,C2) of x's dtype and the forward's out, arg -> (grad_x, grad_center, grad_weight, grad_bias) of that
    dtype, None where `need` is False: one path, no atomics."""
    dev, dt, x, idx, weight, _, center, lengths, N, L, M, K, C1, C2 = _args16("neighbor_mlp_max16_backward", x, idx,
                                                                             weight, None, center, lengths)
    _C._require_gpu(grad_out, out, arg)
    grad_out, out = _t16c(grad_out, "grad_out", dt, rows=True), _t16c(out, "out", dt, rows=True)
    if grad_out.shape != (N, L, C2) or out.shape != (N, L, C2) or (need[1] and center is None):
        raise RuntimeError("neighbor_mlp_max16_backward: need grad_out and out (N,L,C2), center for its gradient")
    if arg.dtype != torch.uint8 or arg.shape != (N, L, C2):
        raise RuntimeError("neighbor_mlp_max16_backward: arg must be the forward's (N,L,C2) uint8")
    arg = _C._contig(arg, "arg")
    shapes = (x.shape, (N, L, C1), weight.shape, (C2,))
    grads = [_C._out(tuple(s), dtype=dt, device=dev) if w else None for s, w in zip(shapes, need)]
    _C._call.neighbor_mlp_max16_backward(
        "neighbor_mlp_max16_backward", dev, grad_out, x, idx, lengths, center, weight, out, arg, DTYPES16[dt], N, L, M, K,
        C1, C2, bool(relu_out), *grads,
        *_C._scratch(dev, _C._lib.pointops_neighbor_mlp_max16_backward_workspace_bytes, N, L, K, M, C1, C2))
    return tuple(grads)


MAX_C2L, MAX_C3 = 128, 256


def supported2_16(N, L, M, K, C1, C2, C3):
    """The sizes the two-layer 16-bit entries take (nm2_sizes_ok of csrc/neighbor_mlp2_16.hip)."""
    return (all(8 <= c <= MAX_C2L and c % 8 == 0 for c in (C1, C2)) and 8 <= C3 <= MAX_C3 and C3 % 8 == 0
            and 1 <= K <= MAX_K and N * L * K < 2 ** 31 and N * M < 2 ** 31 - 1)


def _args2_16(what, x, idx, weight, bias, weight2, bias2, center, lengths):
    dev = _C._require_gpu(x, idx, weight, bias, weight2, bias2, center, lengths)
    if x.dtype not in DTYPES16:
        raise RuntimeError(f"{what}: x must be bfloat16 or float16")
    dt = x.dtype
    x, center = _t16c(x, "x", dt, rows=True), _t16c(center, "center", dt, rows=True)
    weight, bias = _t16c(weight, "weight", dt), _t16c(bias, "bias", dt)
    weight2, bias2 = _t16c(weight2, "weight2", dt), _t16c(bias2, "bias2", dt)
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    if x.dim() != 3 or idx.dim() != 3 or weight.dim() != 2 or weight2.dim() != 2 or idx.shape[0] != x.shape[0] \
            or weight.shape[0] != x.shape[2] or weight2.shape[0] != weight.shape[1]:
        raise RuntimeError(f"{what}: need x (N,M,C1), idx (N,L,K), weight (C1,C2) and weight2 (C2,C3)")
    (N, M, C1), (_, L, K), (C2, C3) = x.shape, idx.shape, weight2.shape
    if (lengths is not None and lengths.shape != (N,)) or (bias is not None and bias.shape != (C2,)) \
            or (bias2 is not None and bias2.shape != (C3,)) or (center is not None and center.shape != (N, L, C1)):
        raise RuntimeError(f"{what}: need lengths (N,), bias (C2,), bias2 (C3,) and center (N,L,C1)")
    if not supported2_16(N, L, M, K, C1, C2, C3):
        raise RuntimeError(f"{what}: need C1 and C2 multiples of 8 in [8, {MAX_C2L}], C3 a multiple of 8 in "
                           f"[8, {MAX_C3}] and 1 <= K <= {MAX_K}")
    return dev, dt, x, idx, weight, bias, weight2, bias2, center, lengths, N, L, M, K, C1, C2, C3


def neighbor_mlp2_max16(x, idx, weight, bias, weight2, bias2=None, center=None, lengths=None, relu_out=True):
    """neighbor_mlp_max16 with a second hidden layer: x (N,M,C1), weight (C1,C2), bias (C2,) or None, weight2 (C2,C3),
    bias2 (C3,) or None and center (N,L,C1) or None of T -> (out (N,L,C3) of T, arg (N,L,C3) uint8)."""
    dev, dt, x, idx, weight, bias, weight2, bias2, center, lengths, N, L, M, K, C1, C2, C3 = _args2_16(
        "neighbor_mlp2_max16", x, idx, weight, bias, weight2, bias2, center, lengths)
    out = _C._out((N, L, C3), dtype=dt, device=dev)
    arg = _C._out((N, L, C3), dtype=torch.uint8, device=dev)
    _C._call.neighbor_mlp2_max16(
        "neighbor_mlp2_max16", dev, x, idx, lengths, center, weight, bias, weight2, bias2, DTYPES16[dt], N, L, M, K, C1,
        C2, C3, bool(relu_out), out, arg,
        *_C._scratch(dev, _C._lib.pointops_neighbor_mlp2_max16_workspace_bytes, N, L, K, M, C1, C2, C3))
    return out, arg


def neighbor_mlp2_max16_backward(grad_out, x, idx, weight, bias, weight2, center, lengths, out, arg, relu_out=True,
                                 need=(True,) * 6):
    """grad_out (N,L,C3) of x's dtype and the forward's out, arg -> (grad_x, grad_center, grad_weight, grad_bias,
    grad_weight2, grad_bias2) of that dtype, None where `need` is False: one path, no atomics.  The workspace holds e1
    (N,L,K,C1) of T for the duration of the call."""
    dev, dt, x, idx, weight, bias, weight2, _, center, lengths, N, L, M, K, C1, C2, C3 = _args2_16(
        "neighbor_mlp2_max16_backward", x, idx, weight, bias, weight2, None, center, lengths)
    _C._require_gpu(grad_out, out, arg)
    grad_out, out = _t16c(grad_out, "grad_out", dt, rows=True), _t16c(out, "out", dt, rows=True)
    if grad_out.shape != (N, L, C3) or out.shape != (N, L, C3) or (need[1] and center is None):
        raise RuntimeError("neighbor_mlp2_max16_backward: need grad_out and out (N,L,C3), center for its gradient")
    if arg.dtype != torch.uint8 or arg.shape != (N, L, C3):
        raise RuntimeError("neighbor_mlp2_max16_backward: arg must be the forward's (N,L,C3) uint8")
    arg = _C._contig(arg, "arg")
    shapes = (x.shape, (N, L, C1), weight.shape, (C2,), weight2.shape, (C3,))
    grads = [_C._out(tuple(s), dtype=dt, device=dev) if w else None for s, w in zip(shapes, need)]
    _C._call.neighbor_mlp2_max16_backward(
        "neighbor_mlp2_max16_backward", dev, grad_out, x, idx, lengths, center, weight, bias, weight2, out, arg,
        DTYPES16[dt], N, L, M, K, C1, C2, C3, bool(relu_out), *grads,
        *_C._scratch(dev, _C._lib.pointops_neighbor_mlp2_max16_backward_workspace_bytes, N, L, K, M, C1, C2, C3))
    return tuple(grads)
