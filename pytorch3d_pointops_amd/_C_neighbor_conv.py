"""Operator boundary of neighbor_conv (csrc/neighbor_conv.hip; C ABI: pointops_neighbor_conv,
pointops_neighbor_conv_backward and its workspace sizer in include/pointops_amd.h, whose NEIGHBOUR CONVOLUTION block is the
definition) and of its bfloat16 / float16 form (csrc/neighbor_conv16.hip; pointops_neighbor_conv16,
pointops_neighbor_conv16_backward and their workspace sizers).

Beside `_C.py`, not in it, as `_C_neighbor_attention.py` is, and with the same seams: the argument normalisers, the
native-call namespace and the output seam are `_C`'s, looked up on the module at call time, so whatever patches `_C._out`
or `_C._call` sees these calls too.  There is no CPU implementation: CPU tensors raise RuntimeError.
"""
import os

import torch

from . import _C
from ._C_neighbor_attention import _rows16

MAX_C, MAX_P, MAX_K = 128, 32, 255
MAX_C16 = 256
DTYPES16 = {torch.bfloat16: 0, torch.float16: 1}  # POINTOPS_DTYPE_BF16, POINTOPS_DTYPE_F16


def supported(N, L, M, K, P, Cin, Cout):
    """The sizes the native entries take (nc_sizes_ok of csrc/neighbor_conv.hip)."""
    return (all(4 <= c <= MAX_C and c % 4 == 0 for c in (Cin, Cout)) and 1 <= P <= MAX_P and 1 <= K <= MAX_K
            and N * L * K < 2 ** 31 and N * M < 2 ** 31 - 1)


def supported16(N, L, M, K, P, Cin, Cout):
    """The sizes the 16-bit entries take (nc16_sizes_ok of csrc/neighbor_conv16.hip)."""
    return (all(8 <= c <= MAX_C16 and c % 8 == 0 for c in (Cin, Cout)) and 1 <= P <= MAX_P and 1 <= K <= MAX_K
            and N * L * K < 2 ** 31 and N * M < 2 ** 31 - 1)


def forced():
    """POINTOPS_DEBUG=neighbor_conv=0|1 (csrc/debug.h's switchboard): False = the torch route, True = the HIP path
    whenever the tensors are float32 (or all bfloat16, or all float16) GPU tensors (sizes it does not take are then an error), None = by `supported`."""
    for item in os.environ.get("POINTOPS_DEBUG", "").split(","):
        key, _, value = item.partition("=")
        if key.strip() == "neighbor_conv" and value.strip() in ("0", "1"):
            return value.strip() == "1"
    return None


def _args(what, x, idx, lengths, coeff, weight):
    dev = _C._require_gpu(x, idx, lengths, coeff, weight)
    x, coeff, weight = _rows16(x, "x"), _C._f32c(coeff, "coeff"), _C._f32c(weight, "weight")
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    if x.dim() != 3 or idx.dim() != 3 or weight.dim() != 3 or idx.shape[0] != x.shape[0] \
            or weight.shape[1] != x.shape[2]:
        raise RuntimeError(f"{what}: need x (N,M,Cin), idx (N,L,K) and weight (P,Cin,Cout)")
    (N, M, Cin), (_, L, K), (P, _, Cout) = x.shape, idx.shape, weight.shape
    if (lengths is not None and lengths.shape != (N,)) or (coeff is not None and coeff.shape != (N, L, K, P)) \
            or (coeff is None and P != K):
        raise RuntimeError(f"{what}: need lengths (N,) and coeff (N,L,K,P), or P == K without coeff")
    if not supported(N, L, M, K, P, Cin, Cout):
        raise RuntimeError(f"{what}: need Cin and Cout multiples of 4 in [4, {MAX_C}], P <= {MAX_P}, 1 <= K <= {MAX_K}")
    return dev, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout


def neighbor_conv(x, idx, weight, lengths=None, coeff=None):
    """x (N,M,Cin) fp32, idx (N,L,K) int64, weight (P,Cin,Cout) fp32, lengths (N,) int64 or None, coeff (N,L,K,P) fp32 or
    None (P == K) -> out (N,L,Cout) fp32."""
    dev, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout = _args("neighbor_conv", x, idx, lengths, coeff, weight)
    out = _C._out((N, L, Cout), dtype=torch.float32, device=dev)
    _C._call.neighbor_conv("neighbor_conv", dev, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout, out)
    return out


def neighbor_conv_backward(grad_out, x, idx, weight, lengths, coeff, need=(True, True, True)):
    """grad_out (N,L,Cout) -> (grad_x, grad_weight, grad_coeff), None where `need` is False: one path, no atomics."""
    dev, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout = _args("neighbor_conv_backward", x, idx, lengths,
                                                                          coeff, weight)
    _C._require_gpu(grad_out)
    grad_out = _rows16(grad_out, "grad_out")
    if grad_out.shape != (N, L, Cout) or (need[2] and coeff is None):
        raise RuntimeError("neighbor_conv_backward: need grad_out (N,L,Cout), coeff for its gradient")
    shapes = (x.shape, weight.shape, (N, L, K, P))
    grads = [_C._out(tuple(s), dtype=torch.float32, device=dev) if w else None for s, w in zip(shapes, need)]
    _C._call.neighbor_conv_backward(
        "neighbor_conv_backward", dev, grad_out, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout, *grads,
        *_C._scratch(dev, _C._lib.pointops_neighbor_conv_backward_workspace_bytes, N, L, K, M, P, Cin, Cout))
    return tuple(grads)


def _t16c(t, name, dtype, rows=False):
    """`dtype` (bfloat16 or float16) + contiguous, and for `rows` 16-byte aligned: the 16-bit kernels move rows 16 bytes
    at a time (a view at an odd storage offset is copied)."""
    if t is None:
        return None
    if t.dtype != dtype:
        raise RuntimeError(f"expected scalar type {str(dtype).replace('torch.', '')} for {name}")
    t = t.contiguous()
    return t.clone() if rows and t.data_ptr() % 16 else t


def _args16(what, x, idx, lengths, coeff, weight):
    dev = _C._require_gpu(x, idx, lengths, coeff, weight)
    if x.dtype not in DTYPES16:
        raise RuntimeError(f"{what}: x must be bfloat16 or float16")
    dt = x.dtype
    x, coeff, weight = _t16c(x, "x", dt, rows=True), _t16c(coeff, "coeff", dt), _t16c(weight, "weight", dt)
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    if x.dim() != 3 or idx.dim() != 3 or weight.dim() != 3 or idx.shape[0] != x.shape[0] \
            or weight.shape[1] != x.shape[2]:
        raise RuntimeError(f"{what}: need x (N,M,Cin), idx (N,L,K) and weight (P,Cin,Cout)")
    (N, M, Cin), (_, L, K), (P, _, Cout) = x.shape, idx.shape, weight.shape
    if (lengths is not None and lengths.shape != (N,)) or (coeff is not None and coeff.shape != (N, L, K, P)) \
            or (coeff is None and P != K):
        raise RuntimeError(f"{what}: need lengths (N,) and coeff (N,L,K,P), or P == K without coeff")
    if not supported16(N, L, M, K, P, Cin, Cout):
        raise RuntimeError(f"{what}: need Cin and Cout multiples of 8 in [8, {MAX_C16}], P <= {MAX_P}, "
                           f"1 <= K <= {MAX_K}")
    return dev, dt, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout


def neighbor_conv16(x, idx, weight, lengths=None, coeff=None):
    """neighbor_conv for T = bfloat16 or float16: x (N,M,Cin), weight (P,Cin,Cout) and coeff (N,L,K,P) or None of T
    -> out (N,L,Cout) of T, accumulated in fp32 on the 16-deep matrix instructions."""
    dev, dt, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout = _args16("neighbor_conv16", x, idx, lengths, coeff,
                                                                                weight)
    out = _C._out((N, L, Cout), dtype=dt, device=dev)
    _C._call.neighbor_conv16("neighbor_conv16", dev, x, idx, lengths, coeff, weight, DTYPES16[dt], N, L, M, K, P, Cin,
                             Cout, out,
                             *_C._scratch(dev, _C._lib.pointops_neighbor_conv16_workspace_bytes, N, L, K, M, P, Cin, Cout))
    return out


def neighbor_conv16_backward(grad_out, x, idx, weight, lengths, coeff, need=(True, True, True)):
    """grad_out (N,L,Cout) of x's dtype -> (grad_x, grad_weight, grad_coeff) of that dtype, None where `need` is False:
    one path, no atomics."""
    dev, dt, x, idx, lengths, coeff, weight, N, L, M, K, P, Cin, Cout = _args16("neighbor_conv16_backward", x, idx,
                                                                                lengths, coeff, weight)
    _C._require_gpu(grad_out)
    grad_out = _t16c(grad_out, "grad_out", dt, rows=True)
    if grad_out.shape != (N, L, Cout) or (need[2] and coeff is None):
        raise RuntimeError("neighbor_conv16_backward: need grad_out (N,L,Cout), coeff for its gradient")
    shapes = (x.shape, weight.shape, (N, L, K, P))
    grads = [_C._out(tuple(s), dtype=dt, device=dev) if w else None for s, w in zip(shapes, need)]
    _C._call.neighbor_conv16_backward(
        "neighbor_conv16_backward", dev, grad_out, x, idx, lengths, coeff, weight, DTYPES16[dt], N, L, M, K, P, Cin, Cout,
        *grads, *_C._scratch(dev, _C._lib.pointops_neighbor_conv16_backward_workspace_bytes, N, L, K, M, P, Cin, Cout))
    return tuple(grads)
