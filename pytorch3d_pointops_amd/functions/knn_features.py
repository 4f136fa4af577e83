"""knn_features -- the K nearest rows of a feature table for every row of another: the dynamic graph of DGCNN / EdgeConv,
Point-Transformer-style feature neighbourhoods, candidate lists for learned descriptors.  `knn_points`' results, field
by field and byte for byte, from a search built for wide rows.

One autograd node: forward is `_C_feature_topk.feature_topk` (csrc/feature_topk.hip: for D <= 128 and K <= 32 the
targets are ordered on the matrix cores, a certificate per row proves that the collected ones hold the K nearest, and the
rest go through the exact all-pairs kernel), backward is the KNN backward with the squared-L2 norm over the same
neighbour table, as `knn_points`' own.  The definition is the FEATURE TOP-K block of include/pointops_amd.h.
"""
from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C_feature_topk
from ._common import neighbor_backward, point_pair
from .knn import _KNN, knn_gather, knn_points

MIN_D = 9  # D <= 8: knn_points has its register scan and its grid


class _KnnFeaturesFn(Function):
    @staticmethod
    def forward(ctx, f1, f2, lengths1, lengths2, K):
        idx, dists, _ = _C_feature_topk.feature_topk(f1, f2, lengths1, lengths2, K)
        ctx.mark_non_differentiable(idx)
        ctx.save_for_backward(f1, f2, lengths1, lengths2, idx)
        return dists, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dists, _grad_idx):
        grad_f1, grad_f2 = neighbor_backward(ctx.saved_tensors, 2, grad_dists, "knn_features backward")
        return grad_f1, grad_f2, None, None, None


@torch.compiler.disable
def knn_features(
    f1: torch.Tensor,
    f2: torch.Tensor,
    lengths1: Optional[torch.Tensor] = None,
    lengths2: Optional[torch.Tensor] = None,
    K: int = 1,
    return_nn: bool = False,
) -> _KNN:
    """For every row of `f1` (N, P1, D): the `K` rows of `f2` (N, P2, D) at the smallest squared L2 distance, in
    ascending order of distance, a tie going to the lower index.

    Returns `knn_points`' KNN(dists, idx, knn) and equals `knn_points(f1, f2, lengths1, lengths2, K=K,
    return_nn=return_nn)` field by field: dists / idx (N, P1, K) are zero for rows >= lengths1[n] and slots >=
    lengths2[n]; knn (N, P1, K, D) when `return_nn`, else None.  `dists` is differentiable in `f1` and `f2`, also
    under torch.use_deterministic_algorithms(True).

    float32 GPU inputs with D > 8 take the feature search; CPU tensors, other dtypes and D <= 8 go to `knn_points`.
    Under torch.compile the call is a graph break."""
    if not (torch.is_tensor(f1) and torch.is_tensor(f2)) or f1.dim() != 3 or f2.dim() != 3:
        raise ValueError("f1 and f2 must be padded tensors of shape (N, P, D).")
    K = int(K)
    if K < 1:
        raise ValueError("K has to be >= 1.")
    if not (f1.is_cuda and f2.is_cuda and f1.dtype == torch.float32 and f2.dtype == torch.float32
            and f1.shape[2] >= MIN_D):
        return knn_points(f1, f2, lengths1, lengths2, K=K, return_nn=return_nn)
    f1, f2, lengths1, lengths2 = point_pair(f1, f2, lengths1, lengths2)
    if lengths1.shape != (f1.shape[0],) or lengths2.shape != (f1.shape[0],):
        raise ValueError("lengths1 and lengths2 must be of shape (N,).")
    if not (torch.is_grad_enabled() and (f1.requires_grad or f2.requires_grad)):
        idx, dists, _ = _C_feature_topk.feature_topk(f1, f2, lengths1, lengths2, K)  # nothing to differentiate: no node
    else:
        dists, idx = _KnnFeaturesFn.apply(f1, f2, lengths1, lengths2, K)
    return _KNN(dists=dists, idx=idx, knn=knn_gather(f2, idx, lengths2) if return_nn else None)
