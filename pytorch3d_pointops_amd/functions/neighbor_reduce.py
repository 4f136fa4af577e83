"""neighbor_reduce / knn_interpolate -- what the neighbour tables are for, without the (N, L, K, C) tensor of knn_gather.

`neighbor_reduce` is the aggregation of EdgeConv / PointNet++ set abstraction (max, sum, mean over the K neighbours of a
row) and, with weights, the sum of PointNet++ feature propagation; `knn_interpolate` is that propagation (three_nn +
three_interpolate; PyG's knn_interpolate) over `knn_points`.

One autograd node: forward is `_C_neighbor_reduce.neighbor_reduce` (csrc/neighbor_reduce.hip: a group of lanes per
query row gathers 16 bytes per lane and slot and adds in ascending k), backward is its pull form over the inverted table
(every row of x sums its addends in table order; the weights' gradient is a dot per slot): no float atomics, so there is
one backward and it is the one torch.use_deterministic_algorithms(True) gets.  The definition is the NEIGHBOUR REDUCE
block of include/pointops_amd.h.
"""
from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C_neighbor_reduce
from ._common import as_f32
from .knn import knn_points

_REDUCTIONS = ("sum", "mean", "max")


class _NeighborReduceFn(Function):
    @staticmethod
    def forward(ctx, x, idx, lengths, weights, reduce):
        out, arg = _C_neighbor_reduce.neighbor_reduce(x, idx, lengths, weights, reduce)
        ctx.save_for_backward(x, idx, lengths, weights, arg)
        ctx.reduce = reduce
        if arg is not None:
            ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_arg):
        x, idx, lengths, weights, arg = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], weights is not None and ctx.needs_input_grad[3]
        grad_x, grad_w = _C_neighbor_reduce.neighbor_reduce_backward(
            as_f32(grad_out).contiguous(), x, idx, lengths, weights, arg, ctx.reduce, need_x=need_x, need_w=need_w)
        return grad_x, None, None, grad_w, None


def _valid_slots(idx, lengths, M):
    valid = (idx >= 0) & (idx < M)
    if lengths is not None:
        valid = valid & (torch.arange(idx.shape[2], device=idx.device)[None, None, :] < lengths[:, None, None])
    return valid


def _neighbor_reduce_torch(x, idx, lengths, weights, reduce):
    """The same definition through torch ops (CPU tensors, other dtypes, max with K > 255): the masked gather of
    knn_gather, then the reduction slot by slot in ascending k.  arg is uint8 (255 = none) for K <= 255, else int64
    (-1 = none)."""
    N, M, C = x.shape
    _, L, K = idx.shape
    valid = _valid_slots(idx, lengths, M)
    padded = torch.nn.functional.pad(x, (0, 0, 0, 1))  # row M: zeros, the source of every masked slot
    src = torch.where(valid, idx, torch.full_like(idx, M))
    rows = padded.gather(1, src.reshape(N, L * K, 1).expand(-1, -1, C)).reshape(N, L, K, C)
    if reduce == "max":
        none = 255 if K <= 255 else -1
        best = rows.sum(2) * 0  # (N, L, C) zeros that follow x's graph and dtype
        arg = torch.full((N, L, C), none, dtype=torch.int64, device=x.device)
        has = torch.full((N, L, 1), False, dtype=torch.bool, device=x.device)
        for k in range(K):
            ok = valid[:, :, k, None]
            take = ok & (~has | (rows[:, :, k] > best))
            best, arg, has = torch.where(take, rows[:, :, k], best), arg.masked_fill(take, k), has | ok
        return best, (arg.to(torch.uint8) if K <= 255 else arg)
    if weights is not None:
        rows = rows * torch.where(valid, weights, torch.full_like(weights, 0.0))[..., None].to(rows.dtype)
    out = rows.sum(2) * 0
    for k in range(K):
        out = out + rows[:, :, k]
    if reduce == "mean":
        out = out / valid.sum(2, keepdim=True).clamp(min=1).to(out.dtype)
    return out, None


@torch.compiler.disable
def neighbor_reduce(
    x: torch.Tensor,
    idx: torch.Tensor,
    lengths: Optional[torch.Tensor] = None,
    reduce: str = "max",
    weights: Optional[torch.Tensor] = None,
    return_arg: bool = False,
):
    """Reduce the neighbours of every row: `x` (N, M, C), `idx` (N, L, K) int64 from any search of the library ->
    (N, L, C), equal to `knn_gather(x, idx, lengths)` reduced over K with the padding left out, but never holding
    the (N, L, K, C) tensor.

    A slot counts when `0 <= idx < M` and (`lengths` is None or `k < lengths[n]`): `knn_points` / `knn_features` tables
    go with their `lengths2`, `ball_query` / `knn_in_radius` tables as they are (-1 is padding).
      "sum"   the sum of the counted rows in ascending k, each multiplied by `weights` (N, L, K) first when given;
      "mean"  the unweighted sum divided by the number of counted slots (at least 1);
      "max"   the maximum per channel, a tie going to the lowest k; 0 for a row without a counted slot.
    `weights` go with "sum" only.  With `return_arg` the result is (out, arg): for "max" arg (N, L, C) uint8 is the
    winning slot, 255 = none; for the other reductions it is None.

    Differentiable in `x` and `weights`, with one backward that uses no float atomics: two calls give the same bytes,
    also under torch.use_deterministic_algorithms(True).  float32 GPU tensors take the HIP kernels; CPU tensors, other
    dtypes and "max" with K > 255 take the same definition through torch ops.  Under torch.compile the call is a graph
    break."""
    if not (torch.is_tensor(x) and torch.is_tensor(idx)) or x.dim() != 3 or idx.dim() != 3:
        raise ValueError("x must be of shape (N, M, C) and idx of shape (N, L, K).")
    if x.shape[0] != idx.shape[0]:
        raise ValueError("x and idx must have same batch dimension.")
    if reduce not in _REDUCTIONS:
        raise ValueError(f"reduce must be one of {_REDUCTIONS}.")
    if weights is not None and reduce != "sum":
        raise ValueError('weights go with reduce="sum" only.')
    if weights is not None and weights.shape != idx.shape:
        raise ValueError("weights must be of idx's shape (N, L, K).")
    if lengths is not None and lengths.shape != (x.shape[0],):
        raise ValueError("lengths must be of shape (N,).")
    if idx.dtype != torch.int64:
        raise ValueError("idx must be int64.")
    native = (x.is_cuda and x.dtype == torch.float32 and x.shape[2] >= 1
              and (weights is None or weights.dtype == torch.float32)
              and not (reduce == "max" and idx.shape[2] > _C_neighbor_reduce.MAX_K))
    if not native:
        out, arg = _neighbor_reduce_torch(x, idx, lengths, weights, reduce)
    elif torch.is_grad_enabled() and (x.requires_grad or (weights is not None and weights.requires_grad)):
        out, arg = _NeighborReduceFn.apply(x, idx, lengths, weights, reduce)
    else:
        out, arg = _C_neighbor_reduce.neighbor_reduce(x, idx, lengths, weights, reduce)  # no node
    return (out, arg) if return_arg else out


@torch.compiler.disable
def knn_interpolate(
    x: torch.Tensor,
    pos_x: torch.Tensor,
    pos_y: torch.Tensor,
    lengths_x: Optional[torch.Tensor] = None,
    lengths_y: Optional[torch.Tensor] = None,
    K: int = 3,
):
    """Feature propagation of PointNet++ (three_nn + three_interpolate; PyG's knn_interpolate): the features `x`
    (N, M, C) at the points `pos_x` (N, M, D) interpolated to the points `pos_y` (N, L, D) -> (N, L, C):

        out[n,l] = sum_k w_k x[n, idx_k] / sum_k w_k,   w_k = 1 / clamp(d2_k, min=1e-16)

    over the `K` nearest points of `pos_x` (`knn_points(pos_y, pos_x, lengths_y, lengths_x, K=K)`, squared distances).
    Slots beyond `lengths_x[n]` and rows beyond `lengths_y[n]` have weight 0 (such rows are 0).  The weights are
    normalised with torch ops on the (N, L, K) tensors and the sum is `neighbor_reduce(..., "sum", weights)`.
    Differentiable in `x`, and in both position tensors through the KNN backward."""
    if x.dim() != 3 or pos_x.dim() != 3 or pos_y.dim() != 3 or x.shape[:2] != pos_x.shape[:2]:
        raise ValueError("x must be of shape (N, M, C), pos_x of (N, M, D) and pos_y of (N, L, D).")
    K = int(K)
    if K < 1:
        raise ValueError("K has to be >= 1.")
    nn = knn_points(pos_y, pos_x, lengths_y, lengths_x, K=K)
    L, M = pos_y.shape[1], pos_x.shape[1]
    valid = nn.idx >= 0
    if lengths_x is not None:
        valid = valid & (torch.arange(K, device=x.device)[None, None, :] < lengths_x[:, None, None])
    else:
        valid = valid & (torch.arange(K, device=x.device)[None, None, :] < M)
    if lengths_y is not None:
        valid = valid & (torch.arange(L, device=x.device)[None, :, None] < lengths_y[:, None, None])
    w = valid.to(nn.dists.dtype) / nn.dists.clamp(min=1e-16)
    w = w / w.sum(2, keepdim=True).clamp(min=torch.finfo(w.dtype).tiny)
    return neighbor_reduce(x, nn.idx, lengths_x, "sum", w.to(x.dtype))
