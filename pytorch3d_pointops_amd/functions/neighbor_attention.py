"""neighbor_attention -- softmax attention over a neighbour table, without the (N, L, K, C) tensors of knn_gather.

The aggregation of point and graph transformers: every query row attends, per head, to the K rows its table names
(PyG's TransformerConv on a knn_graph, the local self-attention of Point-BERT and Stratified Transformer).  As
knn_gather(k), knn_gather(v), einsum, softmax, einsum it writes two (N, L, K, C) tensors and keeps them for a scatter
backward with float atomics.

One autograd node: forward is `_C_neighbor_attention.neighbor_attention` (csrc/neighbor_attention.hip: a group of lanes
per query row, a head on D / 4 consecutive lanes, the k row and the v row of a slot gathered 16 bytes per lane, one pass
with a running maximum), backward is one pass per query row for grad_q and grad_bias and a pull over the inverted table
for grad_k and grad_v: no float atomics, so there is one backward and it is the one
torch.use_deterministic_algorithms(True) gets.  The definition is the NEIGHBOUR ATTENTION block of
include/pointops_amd.h.
"""
import math
import struct
from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C_neighbor_attention
from ._common import as_f32
from .neighbor_reduce import _valid_slots


class _NeighborAttentionFn(Function):
    @staticmethod
    def forward(ctx, q, k, v, idx, lengths, bias, heads, scale):
        out, lse = _C_neighbor_attention.neighbor_attention(q, k, v, idx, lengths, bias, heads, scale)
        ctx.save_for_backward(q, k, v, out, lse, idx, lengths, bias)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v, out, lse, idx, lengths, bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        need = (need[0], need[1], need[2], bias is not None and need[5])
        gq, gk, gv, gb = _C_neighbor_attention.neighbor_attention_backward(
            as_f32(grad_out).contiguous(), q, k, v, out, lse, idx, lengths, bias, ctx.heads, ctx.scale, need=need)
        return gq, gk, gv, None, None, gb, None, None


def _neighbor_attention_torch(q, k, v, idx, lengths, heads, bias, scale):
    """The same definition through torch ops (CPU tensors, other dtypes, other head sizes): the masked gather of
    knn_gather for k and v, then the sums over the slots in ascending k.  A slot that does not count never reaches a
    quotient or an exponential whose gradient could be NaN."""
    N, L, C = q.shape
    M, K, D = k.shape[1], idx.shape[2], C // heads
    valid = _valid_slots(idx, lengths, M)
    src = torch.where(valid, idx, torch.full_like(idx, M)).reshape(N, L * K, 1).expand(-1, -1, C)
    rows = [torch.nn.functional.pad(x, (0, 0, 0, 1)).gather(1, src).reshape(N, L, K, heads, D) for x in (k, v)]
    s = (q.reshape(N, L, 1, heads, D) * rows[0]).sum(-1) * scale  # (N, L, K, heads)
    if bias is not None:
        s = s + bias.to(s.dtype)
    counted = valid[..., None] & (s > -math.inf)
    top = torch.where(counted, s, torch.full_like(s, -math.inf)).amax(2, keepdim=True).detach() if K else s.detach()
    top = torch.where(top > -math.inf, top, torch.full_like(top, 0.0))
    e = torch.where(counted, torch.exp(torch.where(counted, s, top) - top), torch.full_like(s, 0.0))
    den = e.sum(2) * 0
    for j in range(K):
        den = den + e[:, :, j]
    den = torch.where(den > 0, den, torch.full_like(den, 1.0))
    out = rows[1].sum(2) * 0  # (N, L, heads, D) zeros that follow the graph and dtype
    for j in range(K):
        out = out + (e[:, :, j] / den)[..., None] * rows[1][:, :, j]
    return out.reshape(N, L, C)


@torch.compiler.disable
def neighbor_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    idx: torch.Tensor,
    lengths: Optional[torch.Tensor] = None,
    heads: int = 1,
    bias: Optional[torch.Tensor] = None,
    scale: Optional[float] = None,
):
    """Attention of every query row over its neighbours: `q` (N, L, C), `k` and `v` (N, M, C), C = `heads` * D, `idx`
    (N, L, K) int64 from any search of the library -> (N, L, C).  For row (n, l) and head h, over the counted slots:

        s_k = scale * sum_d q[n,l,h,d] k[n,idx_k,h,d] + bias[n,l,k,h]
        w_k = exp(s_k - max_j s_j) / sum_j exp(s_j - max_j s_j)        out[n,l,h,:] = sum_k w_k v[n,idx_k,h,:]

    A slot counts when `0 <= idx < M` and (`lengths` is None or `k < lengths[n]`), as for `neighbor_reduce`.  `bias`
    (N, L, K, heads) is the relative-position term or an additive mask; `-inf` means weight 0.  `scale` defaults to
    1 / sqrt(D); its float32 value is used.  A row and head without a counted slot, or whose every logit is `-inf`,
    gives 0, and every gradient that belongs to it is 0.

    Differentiable in `q`, `k`, `v` and `bias`, with one backward that uses no float atomics: two calls give the same
    bytes, also under torch.use_deterministic_algorithms(True).  float32 GPU tensors with D in {4, 8, ..., 256} take the
    HIP kernels; CPU tensors, other dtypes and other D take the same definition through torch ops.  Under torch.compile
    the call is a graph break."""
    if not all(torch.is_tensor(t) for t in (q, k, v, idx)) or q.dim() != 3 or k.dim() != 3 or idx.dim() != 3:
        raise ValueError("q must be of shape (N, L, C), k and v of shape (N, M, C) and idx of shape (N, L, K).")
    if v.shape != k.shape or k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2]:
        raise ValueError("k and v must be of one shape (N, M, C), with q's batch and channel dimensions.")
    if idx.shape[:2] != q.shape[:2]:
        raise ValueError("idx must be of shape (N, L, K), with q's batch and row dimensions.")
    if idx.dtype != torch.int64:
        raise ValueError("idx must be int64.")
    heads = int(heads)
    if heads < 1 or q.shape[2] < 1 or q.shape[2] % heads:
        raise ValueError("heads must divide the channels C.")
    if lengths is not None and lengths.shape != (q.shape[0],):
        raise ValueError("lengths must be of shape (N,).")
    if bias is not None and bias.shape != (*idx.shape, heads):
        raise ValueError("bias must be of shape (N, L, K, heads).")
    (N, L, C), M, K = q.shape, k.shape[1], idx.shape[2]
    D = C // heads
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    scale = struct.unpack("f", struct.pack("f", scale))[0]  # the float32 value
    tensors = [t for t in (q, k, v, bias) if t is not None]
    native = (all(t.is_cuda and t.dtype == torch.float32 for t in tensors)
              and _C_neighbor_attention.supported(N, L, M, K, heads, D))
    if not native:
        return _neighbor_attention_torch(q, k, v, idx, lengths, heads, bias, scale)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _NeighborAttentionFn.apply(q, k, v, idx, lengths, bias, heads, scale)
    return _C_neighbor_attention.neighbor_attention(q, k, v, idx, lengths, bias, heads, scale)[0]  # no node
