"""estimate_pointcloud_normals / estimate_pointcloud_local_coord_frames -- the API of PyTorch3D's
ops/points_normals.py, the consumer that `get_point_covariances` exists for (the reference's own example,
examples/utils_on_pointclouds.py:90-108, follows it with torch.linalg.eigh).

After the neighbour search everything per point is a 3x3 problem over K rows, so it runs as ONE HIP kernel
(csrc/local_frames.hip): it reads the knn indices once, gathers each neighbour once, forms the covariance in
`covariance.hip`'s order, solves the symmetric eigenproblem with an fp64 Jacobi and disambiguates the signs, writing
48 bytes per point -- no (N,P,K,3) neighbourhood tensor, no batched eigensolver, no host synchronisation.
"""
from typing import Tuple, Union

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C
from ..structures.pointclouds import Pointclouds
from ._common import deterministic_requested, full_lengths
from .knn import knn_points


def centre_clouds(points: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """Each cloud of `points` (N,P,3) minus the mean of its `lengths[n]` valid rows; padded rows become 0.
    (Upstream centres for numerical stability before the covariance; it is differentiable through torch.)"""
    valid = torch.arange(points.shape[1], device=points.device)[None, :] < lengths[:, None]
    mask = valid[..., None].to(points.dtype)
    mean = (points * mask).sum(1) / lengths.clamp(min=1)[:, None].to(points.dtype)
    return (points - mean[:, None, :]) * mask


def _points_and_lengths(pointclouds, neighborhood_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Validated padded points (N,P,3) float32 and lengths (N,) of a Pointclouds or a padded tensor."""
    if isinstance(pointclouds, Pointclouds):
        points, lengths = pointclouds.points_padded(), pointclouds.num_points_per_cloud()
    elif torch.is_tensor(pointclouds):
        points, lengths = pointclouds, None
    else:
        raise ValueError("pointclouds must be a Pointclouds object or a padded (N, P, 3) tensor")
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("The pointclouds argument has to be of shape (minibatch, N, 3)")
    if points.dtype != torch.float32:
        raise ValueError(f"estimate_pointcloud_normals supports float32 points only, got {points.dtype}")
    if neighborhood_size < 1:
        raise ValueError("neighborhood_size has to be >= 1")
    N, P = points.shape[:2]
    if lengths is None:
        if N > 0 and P <= neighborhood_size:
            raise ValueError("The neighborhood_size argument has to be < size of each of the point clouds.")
        lengths = torch.full((N,), P, dtype=torch.int64, device=points.device) if torch.compiler.is_compiling() \
            else full_lengths(N, P, points.device)
    elif N > 0 and not (torch.compiler.is_compiling()
                        or (lengths.is_cuda and torch.cuda.is_current_stream_capturing())):
        # a device-to-host read: skipped while a graph is traced or captured (the kernel stays in bounds for any
        # length; a cloud with lengths[n] <= K then averages over zero rows past its end)
        if int(lengths.min()) <= neighborhood_size:
            raise ValueError("The neighborhood_size argument has to be < size of each of the point clouds.")
    return points, lengths


class _local_frames(Function):
    """Fused forward (csrc/local_frames.hip); backward = grad_C from the eigenpairs, then the existing covariance
    chain: gather -> point_covariances_backward -> gather backward (the inverted-table form when determinism is
    requested)."""

    @staticmethod
    def forward(ctx, points, lengths, idx, disambiguate):
        curvatures, frames = _C.local_frames(points, lengths, idx, disambiguate)
        ctx.save_for_backward(points, lengths, idx, curvatures, frames)
        ctx.disambiguate = disambiguate
        return curvatures, frames

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_curvatures, grad_frames):
        points, lengths, idx, curvatures, frames = ctx.saved_tensors
        grad_cov = _C.local_frames_backward(curvatures, frames, grad_curvatures.float().contiguous(),
                                            grad_frames.float().contiguous(), lengths, ctx.disambiguate)
        knn = _C.gather_neighbors(points, idx, lengths)
        grad_knn = _C.point_covariances_backward(knn, grad_cov)
        grad_points = _C.gather_neighbors_backward(grad_knn, idx, lengths, points.shape[1],
                                                   deterministic=deterministic_requested())
        return grad_points, None, None, None


def estimate_pointcloud_local_coord_frames(
    pointclouds: Union[torch.Tensor, Pointclouds],
    neighborhood_size: int = 50,
    disambiguate_directions: bool = True,
    *,
    use_symeig_workaround: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Principal curvatures (N,P,3, ascending) and local frames (N,P,3,3; column j = unit principal direction j) of
    each point's `neighborhood_size` nearest neighbours in its centred cloud.

    `pointclouds` is a Pointclouds or a padded (N,P,3) float32 tensor (every cloud of length P).  Each cloud must have
    more than `neighborhood_size` points; that check reads the lengths back from the device and is skipped while a
    stream is being captured or a graph traced.  With `disambiguate_directions` the normal n (column 0) and the main
    direction z (column 2) are flipped to face the majority of their neighbourhood and column 1 is n x z; otherwise
    the eigenvector signs are implementation-defined.  Rows past a cloud's length are zero.

    `use_symeig_workaround` is accepted so that code written for PyTorch3D runs unchanged: both values use the same
    fp64 Jacobi solver, which matches a float64 `eigh` of the fp32 covariance to fp32 rounding.
    Differentiable w.r.t. the points (the flips carry no gradient; coincident eigenvalues give inf / nan gradients,
    as `torch.linalg.eigh` does).
    """
    points, lengths = _points_and_lengths(pointclouds, neighborhood_size)
    centred = centre_clouds(points, lengths)
    fixed = centred.detach()
    idx = knn_points(fixed, fixed, lengths, lengths, K=neighborhood_size).idx
    disambiguate = bool(disambiguate_directions)
    if torch.compiler.is_compiling():
        return torch.ops.pointops_amd.local_frames(centred, lengths, idx, disambiguate)
    if not (torch.is_grad_enabled() and centred.requires_grad):
        return _C.local_frames(centred, lengths, idx, disambiguate)  # nothing to differentiate: no autograd node
    return _local_frames.apply(centred, lengths, idx, disambiguate)


def estimate_pointcloud_normals(
    pointclouds: Union[torch.Tensor, Pointclouds],
    neighborhood_size: int = 50,
    disambiguate_directions: bool = True,
    *,
    use_symeig_workaround: bool = True,
) -> torch.Tensor:
    """Unit normals (N,P,3): column 0 of `estimate_pointcloud_local_coord_frames` (same arguments), i.e. the
    principal direction of least variance of each point's neighbourhood."""
    _, frames = estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size, disambiguate_directions,
                                                       use_symeig_workaround=use_symeig_workaround)
    return frames[..., :, 0]
