"""Operator boundary of neighbor_conv (csrc/neighbor_conv.hip; C ABI: pointops_neighbor_conv,
pointops_neighbor_conv_backward and its workspace sizer in include/pointops_amd.h, whose NEIGHBOUR CONVOLUTION block is the
definition).

Beside `_C.py`, not in it, as `_C_neighbor_attention.py` is, and with the same seams: the argument normalisers, the
native-call namespace and the output seam are `_C`'s, looked up on the module at call time, so whatever patches `_C._out`
or `_C._call` sees these calls too.  There is no CPU implementation: CPU tensors raise RuntimeError.
"""
import os

import torch

from . import _C
from ._C_neighbor_attention import _rows16

MAX_C, MAX_P, MAX_K = 128, 32, 255


def supported(N, L, M, K, P, Cin, Cout):
    """The sizes the native entries take (nc_sizes_ok of csrc/neighbor_conv.hip)."""
    return (all(4 <= c <= MAX_C and c % 4 == 0 for c in (Cin, Cout)) and 1 <= P <= MAX_P and 1 <= K <= MAX_K
            and N * L * K < 2 ** 31 and N * M < 2 ** 31 - 1)


def forced():
    """POINTOPS_DEBUG=neighbor_conv=0|1 (csrc/debug.h's switchboard): False = the torch route, True = the HIP path
    whenever the tensors are float32 GPU tensors (sizes it does not take are then an error), None = by `supported`."""
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
