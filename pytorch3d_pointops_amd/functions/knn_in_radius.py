"""knn_in_radius -- the K nearest points among those closer than a radius, sorted by distance: Open3D's
search_hybrid_vector_3d, PCL's radiusSearch with max_nn on sorted results.  It sits between the library's two other
searches: `knn_points` returns the K nearest however far away they are, `ball_query` the first K in INDEX order inside
the radius.

One autograd node: forward is `_C_knn_in_radius.knn_in_radius` (csrc/knn_in_radius.hip: one lane per query walks the
3x3x3 cube of a grid whose cells are at least as wide as the radius), backward is the KNN backward with the squared-L2
norm over the same neighbour table (the -1 padding is skipped inside the kernel), exactly as `ball_query`'s.  The
definition is the KNN IN RADIUS block of include/pointops_amd.h.
"""
import math
import struct
from collections import namedtuple
from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C_knn_in_radius
from ._common import neighbor_backward, point_pair
from .knn import knn_points
from .utils import masked_gather

KNNInRadius = namedtuple("KNNInRadius", "dists idx knn counts")


def _fl32(value: float) -> float:
    try:
        return struct.unpack("f", struct.pack("f", float(value)))[0]
    except OverflowError:
        return math.copysign(math.inf, float(value))
    except (TypeError, ValueError):
        return math.nan


def _radius(value) -> float:
    r = _fl32(value)
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError(f"radius must be finite and > 0 in float32, got {value}")
    return r


class _KnnInRadiusFn(Function):
    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K, radius):
        idx, dists, counts, _ = _C_knn_in_radius.knn_in_radius(p1, p2, lengths1, lengths2, K, radius)
        ctx.mark_non_differentiable(idx, counts)
        ctx.save_for_backward(p1, p2, lengths1, lengths2, idx)
        return dists, idx, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dists, _grad_idx, _grad_counts):
        grad_p1, grad_p2 = neighbor_backward(ctx.saved_tensors, 2, grad_dists, "knn_in_radius backward")
        return grad_p1, grad_p2, None, None, None, None


def _composed(p1, p2, lengths1, lengths2, K, radius):
    """The same definition from `knn_points`: its K nearest, with every slot whose distance is not below r2, whose
    position is at or past lengths2, or whose row is at or past lengths1 turned into padding."""
    nn = knn_points(p1, p2, lengths1, lengths2, K=K)
    r2 = _fl32(radius * radius)  # (the fp64 product of two fp32 values, rounded once: the fp32 product)
    slot = torch.arange(K, device=p1.device)
    row = torch.arange(p1.shape[1], device=p1.device)
    keep = (nn.dists < r2) & (slot[None, None, :] < lengths2[:, None, None]) & \
        (row[None, :, None] < lengths1[:, None, None])
    idx = torch.where(keep, nn.idx, -1)
    dists = torch.where(keep, nn.dists, 0.0)
    return dists, idx, keep.sum(dim=2).to(torch.int32)


@torch.compiler.disable
def knn_in_radius(
    p1: torch.Tensor,
    p2: torch.Tensor,
    lengths1: Optional[torch.Tensor] = None,
    lengths2: Optional[torch.Tensor] = None,
    K: int = 1,
    radius: float = 0.2,
    return_nn: bool = False,
) -> KNNInRadius:
    """For every point of `p1` (N, P1, D): the `K` nearest points of `p2` (N, P2, D) among those closer than `radius`
    (squared distance in float32 below fl32(radius * radius), `ball_query`'s rule), in ascending order of distance, a
    tie going to the lower index.

    Returns KNNInRadius(dists, idx, knn, counts) in `ball_query`'s conventions: squared distances (N, P1, K) padded with
    0, indices (N, P1, K) padded with -1, the gathered neighbours (N, P1, K, D) padded with 0 when `return_nn` (else
    None), and counts (N, P1) int32, the number of valid slots of every row.  `lengths1` / `lengths2` (N,) give the
    valid points per cloud.  On finite inputs the result is `knn_points(K)` with every slot at or beyond the radius
    turned into padding.

    Inputs are float32.  `dists` is differentiable in `p1` and `p2`.  The fused path covers D <= 3 and K <= 64; anything
    else is composed from `knn_points`.  Under torch.compile the call is a graph break."""
    if not (torch.is_tensor(p1) and torch.is_tensor(p2)) or p1.dim() != 3 or p2.dim() != 3:
        raise ValueError("p1 and p2 must be padded tensors of shape (N, P, D).")
    if p1.dtype != torch.float32 or p2.dtype != torch.float32:
        raise ValueError("p1 and p2 must be float32.")
    K = int(K)
    if K < 1:
        raise ValueError("K has to be >= 1.")
    radius = _radius(radius)
    p1, p2, lengths1, lengths2 = point_pair(p1, p2, lengths1, lengths2)
    if lengths1.shape != (p1.shape[0],) or lengths2.shape != (p1.shape[0],):
        raise ValueError("lengths1 and lengths2 must be of shape (N,).")
    if p1.shape[2] > _C_knn_in_radius.MAX_D or K > _C_knn_in_radius.MAX_K:
        dists, idx, counts = _composed(p1, p2, lengths1, lengths2, K, radius)
    elif not (torch.is_grad_enabled() and (p1.requires_grad or p2.requires_grad)):
        # nothing to differentiate: no autograd node
        idx, dists, counts, _ = _C_knn_in_radius.knn_in_radius(p1, p2, lengths1, lengths2, K, radius)
    else:
        dists, idx, counts = _KnnInRadiusFn.apply(p1, p2, lengths1, lengths2, K, radius)
    return KNNInRadius(dists=dists, idx=idx, knn=masked_gather(p2, idx) if return_nn else None, counts=counts)
