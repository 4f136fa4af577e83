"""neighbor_conv / voxel_neighbors -- convolution over a neighbour table, without the (N, L, K, Cin) and (N, L, P, Cin)
tensors of knn_gather + einsum + matmul.

    out[n,l,:] = sum_p ( sum_k coeff[n,l,k,p] * x[n, idx[n,l,k], :] ) @ weight[p]          weight: (P, Cin, Cout)

One form for KPConv (`coeff` the linear correlation max(0, 1 - |y_k - x~_p| / sigma) with P kernel points), PointConv and
continuous convolutions (`coeff` from a weight net on relative positions), interpolated kernels, and -- with `coeff=None`,
where slot k uses weight[k] -- the submanifold sparse convolution over the table `voxel_neighbors` builds from
`voxel_downsample(...).coords`.

One autograd node: forward and backward are `_C_neighbor_conv`'s (csrc/neighbor_conv.hip: a 32-row tile per workgroup,
the rows gathered 16 bytes per lane into per-p registers, the product with weight[p] on v_mfma_f32_32x32x2_f32 with one
accumulator carried across all p; grad_x is the same kernel over the inverted table).  No float atomics, so there is one
backward and it is the one torch.use_deterministic_algorithms(True) gets.  The definition is the NEIGHBOUR CONVOLUTION
block of include/pointops_amd.h.  bfloat16 and float16 features take csrc/neighbor_conv16.hip: weight repacked once per call
in matrix-fragment order, all planes of a chunk through one LDS tile, the product on v_mfma_f32_32x32x16_bf16 / _f16 with
fp32 accumulation, every result rounded once.
"""
from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C_neighbor_conv
from ._common import as_f32
from .neighbor_reduce import _valid_slots


class _NeighborConv16Fn(Function):
    """The node of the bfloat16 / float16 path: every tensor is of x's dtype."""

    @staticmethod
    def forward(ctx, x, idx, weight, lengths, coeff):
        ctx.save_for_backward(x, idx, weight, lengths, coeff)
        return _C_neighbor_conv.neighbor_conv16(x, idx, weight, lengths, coeff)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, idx, weight, lengths, coeff = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gw, gc = _C_neighbor_conv.neighbor_conv16_backward(
            grad_out.to(x.dtype).contiguous(), x, idx, weight, lengths, coeff,
            need=(need[0], need[2], coeff is not None and need[4]))
        return gx, None, gw, None, gc


class _NeighborConvFn(Function):
    @staticmethod
    def forward(ctx, x, idx, weight, lengths, coeff):
        ctx.save_for_backward(x, idx, weight, lengths, coeff)
        return _C_neighbor_conv.neighbor_conv(x, idx, weight, lengths, coeff)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, idx, weight, lengths, coeff = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gw, gc = _C_neighbor_conv.neighbor_conv_backward(
            as_f32(grad_out).contiguous(), x, idx, weight, lengths, coeff,
            need=(need[0], need[2], coeff is not None and need[4]))
        return gx, None, gw, None, gc


def _neighbor_conv_torch(x, idx, weight, lengths, coeff):
    """The same definition through torch ops (CPU tensors, other dtypes, other sizes): the masked gather of
    `_neighbor_attention_torch`, the sums over the slots in ascending k, then one matmul."""
    N, M, Cin = x.shape
    L, K, P = idx.shape[1], idx.shape[2], weight.shape[0]
    valid = _valid_slots(idx, lengths, M)
    src = torch.where(valid, idx, torch.full_like(idx, M)).reshape(N, L * K, 1).expand(-1, -1, Cin)
    rows = torch.nn.functional.pad(x, (0, 0, 0, 1)).gather(1, src).reshape(N, L, K, Cin)
    if coeff is None:
        A = rows  # (N, L, P = K, Cin): the row at slot p, 0 where it is invalid
    else:
        cf = coeff.to(x.dtype)
        cf = torch.where(valid[..., None], cf, torch.full_like(cf, 0.0))
        A = (cf[:, :, :0, :, None] * rows[:, :, :0, None, :]).sum(2)  # (N, L, P, Cin) zeros that follow graph and dtype
        for k in range(K):
            A = A + cf[:, :, k, :, None] * rows[:, :, k, None, :]
    return A.reshape(N, L, P * Cin) @ weight.to(x.dtype).reshape(P * Cin, -1)


@torch.compiler.disable
def neighbor_conv(
    x: torch.Tensor,
    idx: torch.Tensor,
    weight: torch.Tensor,
    lengths: Optional[torch.Tensor] = None,
    coeff: Optional[torch.Tensor] = None,
):
    """Convolution of `x` (N, M, Cin) over the neighbour table `idx` (N, L, K) int64 with `weight` (P, Cin, Cout) and
    `coeff` (N, L, K, P) -> (N, L, Cout):

        out[n,l,:] = sum_p ( sum_k coeff[n,l,k,p] * x[n, idx[n,l,k], :] ) @ weight[p]

    `coeff=None` requires P == K and means "slot k uses weight[k]" (a sparse convolution whose table says which voxel
    sits at each kernel offset: `voxel_neighbors`).  A slot counts when `0 <= idx < M` and (`lengths` is None or
    `k < lengths[n]`), as for `neighbor_reduce`; a row with no such slot gives 0.  There is no bias: add one outside.

    Differentiable in `x`, `weight` and `coeff`, with one backward that uses no float atomics: two calls give the same
    bytes, also under torch.use_deterministic_algorithms(True).  float32 GPU tensors with Cin and Cout multiples of 4 in
    [4, 128], P <= 32 and 1 <= K <= 255 take the HIP kernels, and so do GPU tensors whose `x` is bfloat16 or float16 with
    Cin and Cout multiples of 8 in [8, 256] (`weight` and `coeff` are cast to `x.dtype`; products accumulate in fp32 and
    every result is rounded once to `x.dtype`); CPU tensors, other dtypes and other sizes take the same definition through
    torch ops (POINTOPS_DEBUG=neighbor_conv=0 forces that route, =1 the kernels).  Under torch.compile the call is a
    graph break."""
    if not all(torch.is_tensor(t) for t in (x, idx, weight)) or x.dim() != 3 or idx.dim() != 3 or weight.dim() != 3:
        raise ValueError("x must be of shape (N, M, Cin), idx of shape (N, L, K) and weight of shape (P, Cin, Cout).")
    if idx.shape[0] != x.shape[0] or weight.shape[1] != x.shape[2]:
        raise ValueError("idx must have x's batch dimension and weight x's channel dimension.")
    if idx.dtype != torch.int64:
        raise ValueError("idx must be int64.")
    if lengths is not None and lengths.shape != (x.shape[0],):
        raise ValueError("lengths must be of shape (N,).")
    if coeff is None and weight.shape[0] != idx.shape[2]:
        raise ValueError("without coeff, weight must hold one matrix per slot: P == K.")
    if coeff is not None and coeff.shape != (*idx.shape, weight.shape[0]):
        raise ValueError("coeff must be of shape (N, L, K, P).")
    (N, M, Cin), (_, L, K), (P, _, Cout) = x.shape, idx.shape, weight.shape
    tensors = [t for t in (x, weight, coeff) if t is not None]
    forced = _C_neighbor_conv.forced()
    native = all(t.is_cuda and t.dtype == torch.float32 for t in tensors) and forced is not False and (
        forced or _C_neighbor_conv.supported(N, L, M, K, P, Cin, Cout))
    if forced is not False and x.dtype in _C_neighbor_conv.DTYPES16 and all(t.is_cuda for t in tensors) and (
            forced or _C_neighbor_conv.supported16(N, L, M, K, P, Cin, Cout)):
        weight, coeff = weight.to(x.dtype), None if coeff is None else coeff.to(x.dtype)  # as _neighbor_conv_torch
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return _NeighborConv16Fn.apply(x, idx, weight, lengths, coeff)
        return _C_neighbor_conv.neighbor_conv16(x, idx, weight, lengths, coeff)  # no node
    if not native:
        return _neighbor_conv_torch(x, idx, weight, lengths, coeff)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _NeighborConvFn.apply(x, idx, weight, lengths, coeff)
    return _C_neighbor_conv.neighbor_conv(x, idx, weight, lengths, coeff)  # no node


def voxel_neighbors(coords: torch.Tensor, num_voxels: torch.Tensor, kernel_size: int = 3) -> torch.Tensor:
    """The table of a submanifold sparse convolution: for `coords` (N, P, 3) int64 and `num_voxels` (N,) int64 of
    `voxel_downsample`, `idx` (N, P, kernel_size^3) int64 with the voxel row at each kernel offset, -1 where there is
    none; offsets in ascending (dz, dy, dx) order, so slot kernel_size^3 // 2 is the voxel itself.  Rows at or past
    num_voxels are -1 everywhere.

    The voxels of a cloud come in ascending (z, y, x) cell order, so this is one key pack and one `torch.searchsorted`
    over the batch; nothing synchronises.  The padded extents of a cloud must multiply to less than 2^63."""
    if not torch.is_tensor(coords) or coords.dim() != 3 or coords.shape[2] != 3 or coords.dtype != torch.int64:
        raise ValueError("coords must be an int64 tensor of shape (N, P, 3).")
    N, P, _ = coords.shape
    if not torch.is_tensor(num_voxels) or num_voxels.dtype != torch.int64 or num_voxels.shape != (N,):
        raise ValueError("num_voxels must be an int64 tensor of shape (N,).")
    kernel_size = int(kernel_size)
    if kernel_size < 1 or kernel_size % 2 == 0:
        raise ValueError("kernel_size must be odd and positive.")
    r = kernel_size // 2
    live = torch.arange(P, device=coords.device)[None, :] < num_voxels[:, None]  # (N, P)
    big = torch.iinfo(torch.int64).max
    lo = torch.where(live[..., None], coords, torch.full_like(coords, big)).amin(1, keepdim=True) if P else coords
    hi = torch.where(live[..., None], coords, torch.full_like(coords, -big)).amax(1, keepdim=True) if P else coords
    lo, hi = torch.where(lo > hi, torch.full_like(lo, 0), lo), torch.where(lo > hi, torch.full_like(hi, 0), hi)  # empty cloud
    rel = coords - lo + r  # (N, P, 3) in [r, extent - r)
    extent = hi - lo + 1 + 2 * r  # (N, 1, 3)

    def pack(c, e):  # (z, y, x) order
        return (c[..., 2] * e[..., 1] + c[..., 1]) * e[..., 0] + c[..., 0]

    keys = torch.where(live, pack(rel, extent), torch.full((), big, dtype=torch.int64, device=coords.device))
    d = torch.arange(-r, r + 1, device=coords.device)
    offsets = torch.stack(torch.meshgrid(d, d, d, indexing="ij"), -1).reshape(-1, 3).flip(-1)  # rows (dx, dy, dz)
    want = pack(rel[:, :, None, :] + offsets, extent[:, :, None, :])  # (N, P, k^3): inside the padded extent
    pos = torch.searchsorted(keys, want.reshape(N, -1)).clamp(max=max(P - 1, 0))
    hit = (keys.gather(1, pos) == want.reshape(N, -1)) if P else pos.bool()
    idx = torch.where(hit, pos, torch.full_like(pos, -1)).reshape(N, P, -1)
    return torch.where(live[..., None], idx, torch.full_like(idx, -1))
