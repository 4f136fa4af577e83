"""voxel_downsample -- the step in front of every scan pipeline: one point per occupied voxel.

Open3D's voxel_down_sample and PCL's VoxelGrid put it before plane extraction, clustering, normals, keypoints,
descriptors and registration, so that those run at the density the task needs and their radii are chosen per voxel size
instead of per sensor; the same operation is the grid pooling of point networks, and its integer cell coordinates are
what sparse convolutions consume.  Composed in torch it is a floor, a `torch.unique(dim=..., return_inverse=True)`, an
`index_add_` and a divide: an output whose shape depends on the data (a host synchronisation, no graph capture) and
atomic sums whose last bit changes from run to run.  Here it is one native call (csrc/voxel.hip): keys, one stable
radix sort, one scan, and sums in an order the sorted position alone fixes -- static shapes padded to P voxel rows,
nothing read back, two calls byte-equal, capturable.  The definition is the comment block of pointops_voxel_downsample
in include/pointops_amd.h.  Differentiable in the points and the features, with the voxel assignment held constant.
"""
import math
import struct
from collections import namedtuple
from typing import Dict, Optional, Union

import torch

from .. import _C_voxel
from ..structures.pointclouds import Pointclouds

VoxelDownsample = namedtuple("VoxelDownsample", "points features num_voxels inverse counts first_index coords status")


def _voxel_size(value):
    """`value` as the kernels receive it: rounded to float32; finite and > 0 or ValueError."""
    try:
        v = struct.unpack("f", struct.pack("f", float(value)))[0]
    except (OverflowError, TypeError, ValueError):
        v = math.nan
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"voxel_size must be finite and > 0 in float32, got {value}")
    return v


def _member_mean_grad(grad_out, inverse, counts):
    """grad_in[n, i] = grad_out[n, inverse[n, i]] / counts[n, inverse[n, i]] on the rows of a voxel, 0 elsewhere."""
    member = inverse >= 0
    idx = inverse.clamp(min=0)
    g = torch.gather(grad_out, 1, idx[..., None].expand(-1, -1, grad_out.shape[2]))
    c = torch.gather(counts, 1, idx).clamp(min=1).to(grad_out.dtype)
    return torch.where(member[..., None], g / c[..., None], torch.full((), 0.0, dtype=grad_out.dtype,
                                                                       device=grad_out.device))


class _VoxelDownsampleFn(torch.autograd.Function):
    """The native call; the backward is plain torch (a gather and a divide: deterministic, no kernel of its own)."""

    @staticmethod
    def forward(ctx, points, lengths, voxel_size, features, origin):
        num, status, inverse, counts, first, coords, centroids, pooled = _C_voxel.voxel_downsample(
            points.detach(), lengths, voxel_size, None if features is None else features.detach(), origin)
        ctx.save_for_backward(inverse, counts)
        ctx.has_features = features is not None
        ctx.mark_non_differentiable(num, status, inverse, counts, first, coords)
        if pooled is None:
            return centroids, num, status, inverse, counts, first, coords
        return centroids, num, status, inverse, counts, first, coords, pooled

    @staticmethod
    def backward(ctx, grad_centroids, *grads):
        inverse, counts = ctx.saved_tensors
        grad_points = grad_features = None
        if ctx.needs_input_grad[0] and grad_centroids is not None:
            grad_points = _member_mean_grad(grad_centroids, inverse, counts)
        if ctx.has_features and ctx.needs_input_grad[3] and grads[-1] is not None:
            grad_features = _member_mean_grad(grads[-1], inverse, counts)
        return grad_points, None, None, grad_features, None


def _check_features(features, N, P):
    """features as (one (N, P, C) tensor or None, the dict's (name, width) list or None)."""
    if features is None:
        return None, None
    named = None
    if isinstance(features, dict):
        if not features:
            return None, []
        named = [(k, t) for k, t in features.items()]
        tensors = [t for _, t in named]
    else:
        tensors = [features]
    for t in tensors:
        if not torch.is_tensor(t) or t.dim() != 3 or tuple(t.shape[:2]) != (N, P):
            raise ValueError("features must be a tensor of shape (N, P, C), or a dict of such tensors")
        if t.dtype != torch.float32:
            raise ValueError(f"features must be float32, got {t.dtype}")
    if named is None:
        both = tensors[0]
    else:
        both = tensors[0] if len(tensors) == 1 else torch.cat(tensors, dim=2)
    if both.shape[2] > _C_voxel.VOXEL_MAX_CHANNELS:
        raise ValueError(f"at most {_C_voxel.VOXEL_MAX_CHANNELS} feature channels in all, got {both.shape[2]}")
    return both, None if named is None else [(k, t.shape[2]) for k, t in named]


@torch.compiler.disable
def voxel_downsample(points: Union[torch.Tensor, Pointclouds], lengths: Optional[torch.Tensor] = None, *,
                     voxel_size: float, features: Union[None, torch.Tensor, Dict[str, torch.Tensor]] = None,
                     origin: Optional[torch.Tensor] = None) -> VoxelDownsample:
    """Voxel-grid pooling of every cloud of `points` ((N, P, 3) float32 padded tensor or a `Pointclouds`; `lengths` (N,)
    int64 for a tensor, None = full).

    A row is live when it is below its cloud's length and its coordinates are finite.  The cell of a live point is
    floor((x - o) / voxel_size) per axis, in float64, with `origin` o ((3,) or (N, 3) float32) or, without one, Open3D's
    rule o = min - voxel_size / 2 per cloud and axis.  The voxels of a cloud are its distinct cells in ascending
    (z, y, x) order.  A cloud whose cells span 2^21 or more on an axis, or reach 2^31 in magnitude, is refused:
    `status` 1, no voxels.

    `features`: an (N, P, C) float32 tensor or a dict of such tensors (the `Pointclouds` route pools every feature the
    structure holds); they are averaged per voxel and not renormalised.

    Returns VoxelDownsample(points (N, P, 3) the centroids, features (as given: tensor, dict or None), num_voxels (N,)
    int64, inverse (N, P) int64 the voxel of every input row or -1, counts (N, P) int64, first_index (N, P) int64 the
    lowest member row or -1, coords (N, P, 3) int64 the cell relative to the origin, status (N,) int32), all padded to P
    voxel rows: rows at or past num_voxels hold 0 (-1 in first_index).  `voxels_to_padded` trims them.  Every mean is a
    float64 sum in a fixed order, rounded once: two calls are byte-equal; nothing synchronises.  Differentiable in
    `points` and `features` (the assignment is constant); under torch.compile the call is a graph break."""
    if isinstance(points, Pointclouds):
        if lengths is not None or features is not None:
            raise ValueError("lengths and features come with the Pointclouds: pass one or the other")
        pc = points
        points, lengths = pc.points_padded(), pc.num_points_per_cloud()
        features = pc.features_padded() or None
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("points must be a padded tensor of shape (N, P, 3), or a Pointclouds")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    N, P, _ = points.shape
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int64 or lengths.shape != (N,)):
        raise ValueError("lengths must be an int64 tensor of shape (N,)")
    if origin is not None and (not torch.is_tensor(origin) or origin.dtype != torch.float32
                               or tuple(origin.shape) not in ((3,), (N, 3))):
        raise ValueError("origin must be a float32 tensor of shape (3,) or (N, 3)")
    v = _voxel_size(voxel_size)
    both, named = _check_features(features, N, P)
    out = _VoxelDownsampleFn.apply(points, lengths, v, both, None if origin is None else origin.detach())
    centroids, num, status, inverse, counts, first, coords = out[:7]
    pooled = out[7] if both is not None else None
    if named is not None:
        parts = torch.split(pooled, [w for _, w in named], dim=2) if named else ()
        pooled = {k: t for (k, _), t in zip(named, parts)}
    return VoxelDownsample(centroids, pooled, num, inverse, counts, first, coords, status)


def voxels_to_padded(result: VoxelDownsample, check: bool = False) -> VoxelDownsample:
    """The P-row outputs of `voxel_downsample` trimmed to Vmax rows, Vmax the largest num_voxels (one host read-back);
    `inverse`, `num_voxels` and `status` stay as they are.  check=True: RuntimeError when a cloud was refused."""
    if not isinstance(result, VoxelDownsample):
        raise ValueError("voxels_to_padded takes the VoxelDownsample that voxel_downsample returns")
    N = result.num_voxels.shape[0]
    vmax = refused = 0
    if N > 0:
        vmax, refused = torch.stack([result.num_voxels.max(), result.status.max().to(torch.int64)]).tolist()
    if check and refused:
        raise RuntimeError("voxel_downsample refused a cloud (status 1): its cells span 2^21 or more on an axis or reach "
                           "2^31; choose a larger voxel_size or remove the outliers")
    cut = lambda t: None if t is None else t[:, :vmax]  # noqa: E731
    feats = result.features
    feats = {k: cut(t) for k, t in feats.items()} if isinstance(feats, dict) else cut(feats)
    return VoxelDownsample(cut(result.points), feats, result.num_voxels, result.inverse, cut(result.counts),
                           cut(result.first_index), cut(result.coords), result.status)
