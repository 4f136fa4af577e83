"""neighbor_mlp_max / edge_mlp_max -- the per-edge MLP of PointNet++ set abstraction and multi-layer EdgeConv, fused with
the maximum over the K neighbours, without the two (N, L, K, C) tensors of knn_gather + add + relu + matmul + amax.

    out[i] = max_k act( W2 . relu( W1 . [f_j, p_j - p_i] + b1 ) + b2 ),   j = idx[i, k]

The first layer needs no edge-sized work: W1 . [f_j, p_j - p_i] + b1 = u[j] + c[i] with u per target and c per query, two
ordinary matmuls (`edge_mlp_max`).  `neighbor_mlp_max` starts from u and c.

One autograd node: forward and backward are `_C_neighbor_mlp`'s (csrc/neighbor_mlp.hip: 32 query rows at the same slot k
are the M side of a v_mfma_f32_32x32x2_f32 block, weight stays resident in registers as B-fragments, the running maximum
and its slot are updated elementwise in the accumulator's layout; the backward recomputes the selection from `arg`, so
nothing edge-sized is saved or written; grad_x is pulled over the inverted table).  No float atomics, so there is one
backward and it is the one torch.use_deterministic_algorithms(True) gets.  The definition is the NEIGHBOUR MLP-MAX block
of include/pointops_amd.h.  bfloat16 and float16 features take csrc/neighbor_mlp16.hip: weight transposed and zero-padded
once per call, several slots of a row tile through one LDS tile per barrier pair, the product on
v_mfma_f32_32x32x16_bf16 / _f16 with fp32 accumulation, every result rounded once.  With `weight2` they take
csrc/neighbor_mlp2_16.hip: a second matrix stage fed from a second LDS tile that the first stage writes in its
accumulator layout (bias, ReLU, one rounding), and a query-order backward that recomputes both hidden layers, runs the
two transposed products and the two weight gradients on the matrix cores and hands e1 to a pull over the inverted table.
"""
from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C_neighbor_mlp
from ._common import as_f32
from .neighbor_reduce import _valid_slots


class _NeighborMlpMaxFn(Function):
    @staticmethod
    def forward(ctx, x, idx, weight, bias, center, lengths, relu_out):
        out, arg = _C_neighbor_mlp.neighbor_mlp_max(x, idx, weight, bias, center, lengths, relu_out)
        ctx.save_for_backward(x, center, idx, lengths, weight, out, arg)
        ctx.relu_out = relu_out
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_arg):
        x, center, idx, lengths, weight, out, arg = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gc, gw, gb = _C_neighbor_mlp.neighbor_mlp_max_backward(
            as_f32(grad_out).contiguous(), x, idx, weight, center, lengths, out, arg, ctx.relu_out,
            need=(need[0], center is not None and need[4], need[2], need[3]))
        return gx, None, gw, gb, gc, None, None


class _NeighborMlpMax16Fn(Function):
    """The node of the bfloat16 / float16 path: every tensor is of x's dtype."""

    @staticmethod
    def forward(ctx, x, idx, weight, bias, center, lengths, relu_out):
        out, arg = _C_neighbor_mlp.neighbor_mlp_max16(x, idx, weight, bias, center, lengths, relu_out)
        ctx.save_for_backward(x, center, idx, lengths, weight, out, arg)
        ctx.relu_out = relu_out
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_arg):
        x, center, idx, lengths, weight, out, arg = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gc, gw, gb = _C_neighbor_mlp.neighbor_mlp_max16_backward(
            grad_out.to(x.dtype).contiguous(), x, idx, weight, center, lengths, out, arg, ctx.relu_out,
            need=(need[0], center is not None and need[4], need[2], need[3]))
        return gx, None, gw, gb, gc, None, None


class _NeighborMlp2Max16Fn(Function):
    """The node of the two-layer bfloat16 / float16 path: every tensor is of x's dtype; nothing edge-sized is saved."""

    @staticmethod
    def forward(ctx, x, idx, weight, bias, weight2, bias2, center, lengths, relu_out):
        out, arg = _C_neighbor_mlp.neighbor_mlp2_max16(x, idx, weight, bias, weight2, bias2, center, lengths, relu_out)
        ctx.save_for_backward(x, center, idx, lengths, weight, bias, weight2, out, arg)
        ctx.relu_out = relu_out
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_arg):
        x, center, idx, lengths, weight, bias, weight2, out, arg = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gc, gw, gb, gw2, gb2 = _C_neighbor_mlp.neighbor_mlp2_max16_backward(
            grad_out.to(x.dtype).contiguous(), x, idx, weight, bias, weight2, center, lengths, out, arg, ctx.relu_out,
            need=(need[0], center is not None and need[6], need[2], need[3], need[4], need[5]))
        return gx, None, gw, gb, gw2, gb2, gc, None, None


def _neighbor_mlp_max_torch(x, idx, weight, bias, center, lengths, relu_out, weight2=None, bias2=None):
    """The same definition through torch ops (CPU tensors, other dtypes, other sizes) -- the composition the fused
    kernels replace: the masked gather of knn_gather, add, relu, matmul (with `weight2`: relu and a second matmul), and
    the maximum over the valid slots with its gradient sent to the lowest winning k.  arg is uint8 (255 = none) for
    K <= 255, else int64 (-1 = none)."""
    N, M, C1 = x.shape
    _, L, K = idx.shape
    valid = _valid_slots(idx, lengths, M)
    src = torch.where(valid, idx, torch.full_like(idx, M)).reshape(N, L * K, 1).expand(-1, -1, C1)
    a = torch.nn.functional.pad(x, (0, 0, 0, 1)).gather(1, src).reshape(N, L, K, C1)
    if center is not None:
        a = a + center.to(x.dtype)[:, :, None, :]
    y = torch.relu(a) @ weight.to(x.dtype)  # (N, L, K, C2)
    if bias is not None:
        y = y + bias.to(x.dtype)
    if weight2 is not None:
        y = torch.relu(y) @ weight2.to(x.dtype)  # (N, L, K, C3)
        if bias2 is not None:
            y = y + bias2.to(x.dtype)
    masked = y.detach().masked_fill(~valid[..., None], float("-inf"))
    slots = torch.arange(K, device=x.device)[None, None, :, None]
    arg = torch.where(masked == masked.amax(2, keepdim=True), slots, torch.full_like(slots, K)).amin(2)  # (N, L, C2)
    none = ~valid.any(2)[..., None] | (arg >= K)
    best = y.gather(2, arg.clamp(max=max(K - 1, 0))[:, :, None, :]).squeeze(2)
    best = best.masked_fill(none, 0.0)
    if relu_out:
        best = torch.relu(best)
    arg = torch.where(none, torch.full_like(arg, 255 if K <= 255 else -1), arg)
    return best, (arg.to(torch.uint8) if K <= 255 else arg)


@torch.compiler.disable
def neighbor_mlp_max(
    x: torch.Tensor,
    idx: torch.Tensor,
    weight: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    center: Optional[torch.Tensor] = None,
    lengths: Optional[torch.Tensor] = None,
    relu_out: bool = True,
    return_arg: bool = False,
    weight2: Optional[torch.Tensor] = None,
    bias2: Optional[torch.Tensor] = None,
):
    """ReLU, one linear layer and the maximum over the neighbours of every row: `x` (N, M, C1) per-target
    pre-activations, `idx` (N, L, K) int64, `weight` (C1, C2), `bias` (C2,), `center` (N, L, C1) the per-query term
    added before the inner ReLU -> (N, L, C2):

        out[n,l,:] = act( max_k  relu(x[n, idx[n,l,k], :] + center[n,l,:]) @ weight + bias )

    with act = relu for `relu_out`, else the identity.  A slot counts when `0 <= idx < M` and (`lengths` is None or
    `k < lengths[n]`), as for `neighbor_reduce`; a tie goes to the lowest k; a row with no such slot gives 0.  With
    `return_arg` the result is (out, arg): arg (N, L, C2) uint8 is the winning slot, 255 = none.

    Differentiable in `x`, `weight`, `bias` and `center`, with one backward that uses no float atomics and holds no
    (N, L, K, .) tensor: two calls give the same bytes, also under torch.use_deterministic_algorithms(True).  float32 GPU
    tensors with C1 and C2 multiples of 4 in [4, 128] and 1 <= K <= 255 take the HIP kernels, and so do GPU tensors whose
    `x` is bfloat16 or float16 with C1 and C2 multiples of 8 in [8, 256] (`weight`, `bias` and `center` are cast to
    `x.dtype`; the hidden value is rounded to `x.dtype` as a torch add and relu would, products accumulate in fp32 and
    every result is rounded once); CPU tensors, other dtypes and other sizes take the same definition through torch ops
    (POINTOPS_DEBUG=neighbor_mlp=0 forces that route, =1 the kernels).  Under torch.compile the call is a graph break.

    With `weight2` (C2, C3) and `bias2` (C3,) one more hidden layer sits between the inner ReLU and the pooled layer,

        out[n,l,:] = act( max_k  relu( relu(x[n, idx[n,l,k], :] + center[n,l,:]) @ weight + bias ) @ weight2 + bias2 )

    and out and arg are (N, L, C3): the three-layer block of PointNet++ or a two-layer EdgeConv after `edge_mlp_max`'s
    split.  GPU tensors whose `x` is bfloat16 or float16, with C1 and C2 multiples of 8 in [8, 128], C3 a multiple of 8
    in [8, 256] and 1 <= K <= 255, take csrc/neighbor_mlp2_16.hip (`weight2` and `bias2` are cast to `x.dtype` too; the
    hidden value is rounded to `x.dtype` once): the same promises, gradients also for `weight2` and `bias2`, nothing
    edge-sized saved between forward and backward; the backward holds e1 (N, L, K, C1) of `x.dtype` in its workspace
    for the duration of the call.  Everything else, float32 included, takes the torch route."""
    if not all(torch.is_tensor(t) for t in (x, idx, weight)) or x.dim() != 3 or idx.dim() != 3 or weight.dim() != 2:
        raise ValueError("x must be of shape (N, M, C1), idx of shape (N, L, K) and weight of shape (C1, C2).")
    if idx.shape[0] != x.shape[0] or weight.shape[0] != x.shape[2]:
        raise ValueError("idx must have x's batch dimension and weight x's channel dimension.")
    if idx.dtype != torch.int64:
        raise ValueError("idx must be int64.")
    if lengths is not None and lengths.shape != (x.shape[0],):
        raise ValueError("lengths must be of shape (N,).")
    if bias is not None and bias.shape != (weight.shape[1],):
        raise ValueError("bias must be of shape (C2,).")
    if center is not None and center.shape != (x.shape[0], idx.shape[1], x.shape[2]):
        raise ValueError("center must be of shape (N, L, C1).")
    (N, M, C1), (_, L, K), C2 = x.shape, idx.shape, weight.shape[1]
    relu_out = bool(relu_out)
    forced = _C_neighbor_mlp.forced()
    if weight2 is None:
        if bias2 is not None:
            raise ValueError("bias2 needs weight2.")
    else:
        if not torch.is_tensor(weight2) or weight2.dim() != 2 or weight2.shape[0] != C2:
            raise ValueError("weight2 must be of shape (C2, C3).")
        if bias2 is not None and bias2.shape != (weight2.shape[1],):
            raise ValueError("bias2 must be of shape (C3,).")
        tensors = [t for t in (x, weight, bias, weight2, bias2, center) if t is not None]
        if forced is not False and x.dtype in _C_neighbor_mlp.DTYPES16 and all(t.is_cuda for t in tensors) and (
                forced or _C_neighbor_mlp.supported2_16(N, L, M, K, C1, C2, weight2.shape[1])):
            weight, bias, weight2, bias2, center = (None if t is None else t.to(x.dtype)
                                                    for t in (weight, bias, weight2, bias2, center))
            if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
                out, arg = _NeighborMlp2Max16Fn.apply(x, idx, weight, bias, weight2, bias2, center, lengths, relu_out)
            else:
                out, arg = _C_neighbor_mlp.neighbor_mlp2_max16(x, idx, weight, bias, weight2, bias2, center, lengths,
                                                               relu_out)  # no node
        else:
            out, arg = _neighbor_mlp_max_torch(x, idx, weight, bias, center, lengths, relu_out, weight2, bias2)
        return (out, arg) if return_arg else out
    tensors = [t for t in (x, weight, bias, center) if t is not None]
    native = all(t.is_cuda and t.dtype == torch.float32 for t in tensors) and forced is not False and (
        forced or _C_neighbor_mlp.supported(N, L, M, K, C1, C2))
    if forced is not False and x.dtype in _C_neighbor_mlp.DTYPES16 and all(t.is_cuda for t in tensors) and (
            forced or _C_neighbor_mlp.supported16(N, L, M, K, C1, C2)):
        weight, bias, center = (None if t is None else t.to(x.dtype) for t in (weight, bias, center))  # as the torch route
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            out, arg = _NeighborMlpMax16Fn.apply(x, idx, weight, bias, center, lengths, relu_out)
        else:
            out, arg = _C_neighbor_mlp.neighbor_mlp_max16(x, idx, weight, bias, center, lengths, relu_out)  # no node
    elif not native:
        out, arg = _neighbor_mlp_max_torch(x, idx, weight, bias, center, lengths, relu_out)
    elif torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        out, arg = _NeighborMlpMaxFn.apply(x, idx, weight, bias, center, lengths, relu_out)
    else:
        out, arg = _C_neighbor_mlp.neighbor_mlp_max(x, idx, weight, bias, center, lengths, relu_out)  # no node
    return (out, arg) if return_arg else out


def edge_mlp_max(feat_t, feat_q, idx, w_target, w_query, b1, w2, b2, lengths=None, w3=None, b3=None):
    """A two-layer edge MLP with max pooling, its first layer split so that no edge-sized tensor exists:

        u = feat_t @ w_target + b1        (N, M, C1), per target
        c = feat_q @ w_query              (N, L, C1), per query
        out = neighbor_mlp_max(u, idx, w2, b2, center=c, lengths=lengths)      = relu(max_k relu(u[j] + c[i]) @ w2 + b2)

    For a first layer W1 (rows: input channels) on the concatenated edge feature:
      EdgeConv on [x_i, x_j - x_i], W1 = [W1a; W1b]:  feat_t = feat_q = x, w_target = W1b, w_query = W1a - W1b.
      PointNet++ on [p_j - p_i, f_j], W1 = [W1p; W1f]:  feat_t = [p, f] with w_target = W1, feat_q = the query positions
      with w_query = -W1p.
    With `w3` (and `b3`) the block has three layers: out = relu(max_k relu(relu(u[j] + c[i]) @ w2 + b2) @ w3 + b3)."""
    u = feat_t @ w_target + b1
    c = feat_q @ w_query
    return neighbor_mlp_max(u, idx, w2, b2, center=c, lengths=lengths, weight2=w3, bias2=b3)
