"""iss_keypoints -- which points of a cloud get a descriptor: the step between the normals and `fpfh_features` /
`mutual_nearest_neighbors` in the registration chain, which otherwise describe and match every point, most of them on
flat or repetitive surface.

ISS (Intrinsic Shape Signatures, Zhong 2009; Open3D's compute_iss_keypoints, PCL's ISSKeypoint3D) takes the eigenvalues
of the scatter matrix of every point's radius neighbourhood, rejects the points whose eigenvalue ratios say "plane" or
"line", and keeps the local maxima of the smallest eigenvalue.  Composed in torch that is a ball_query table capped at
the largest neighbourhood, a gathered (N, P, K, 3) tensor, a batched eigvalsh and a second table for the suppression.
Here it is one native call (csrc/iss.hip): the cell grid of the exact searches and two walks of each point's 3x3x3 cube
under ball query's certificate, the scatter matrix summed in integers -- exact, order-free, no neighbour table, no host
read-back, capturable.  The definition is the comment block of pointops_iss_keypoints in include/pointops_amd.h.
Nothing here is differentiable.
"""
import math
import struct
from collections import namedtuple
from typing import Optional, Union

import torch

from .. import _C_iss
from ..structures.pointclouds import Pointclouds
from .knn import knn_points

ISSKeypoints = namedtuple("ISSKeypoints", "mask saliency eigenvalues num_keypoints")


def _f32(value, name):
    """`value` as the kernels receive it: rounded to float32; finite and > 0 or ValueError."""
    try:
        v = struct.unpack("f", struct.pack("f", float(value)))[0]
    except OverflowError:
        v = math.inf
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{name} must be finite and > 0 in float32, got {value}")
    return v


def _padded(points, lengths):
    if isinstance(points, Pointclouds):
        if lengths is not None:
            raise ValueError("lengths come with the Pointclouds: pass one or the other")
        points, lengths = points.points_padded(), points.num_points_per_cloud()
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("points must be a padded tensor of shape (N, P, 3), or a Pointclouds")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int64
                                or lengths.shape != (points.shape[0],)):
        raise ValueError("lengths must be an int64 tensor of shape (N,)")
    return points, lengths


@torch.compiler.disable
def iss_keypoints(points: Union[torch.Tensor, Pointclouds], lengths: Optional[torch.Tensor] = None, *,
                  salient_radius: float, non_max_radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                  min_neighbors: int = 5) -> ISSKeypoints:
    """ISS keypoints of every cloud of `points` ((N, P, 3) float32 padded tensor or a `Pointclouds`; `lengths` (N,)
    int64 for a tensor, None = full).

    The support of a point is every point closer than `salient_radius` (squared distance in float32 as `ball_query`
    forms it, the point itself included).  Its covariance about the support's mean has the eigenvalues l0 <= l1 <= l2
    (`eigenvalues`).  The point is salient, with `saliency` = l0, when l1 < gamma_21 * l2 and l0 < gamma_32 * l1 -- not a
    line, not a plane -- and l0 > 2^-20 * l2; else its saliency is 0.  A salient point is a keypoint (`mask`) when it has
    at least `min_neighbors` points within `non_max_radius`, itself included, and none of them has a larger saliency, or
    an equal one and a lower index.  The radii are scalars for the whole batch: `cloud_resolution` gives the scale
    Open3D derives its defaults from.  The covariance is summed in integers over offsets quantized to 2^-19 of the
    radius (eigenvalues within 3 * 2^-17 * salient_radius^2 of the float64 ones), so two calls are bit-equal and the
    result does not depend on the order of arrival of anything.

    Returns ISSKeypoints(mask (N, P) bool, saliency (N, P) float32, eigenvalues (N, P, 3) float32, num_keypoints (N,)
    int64); padding rows are False / 0.  Not differentiable; under torch.compile the call is a graph break."""
    points, lengths = _padded(points, lengths)
    rs, rn = _f32(salient_radius, "salient_radius"), _f32(non_max_radius, "non_max_radius")
    g21, g32 = _f32(gamma_21, "gamma_21"), _f32(gamma_32, "gamma_32")
    if int(min_neighbors) != min_neighbors or int(min_neighbors) < 0:
        raise ValueError(f"min_neighbors must be an integer >= 0, got {min_neighbors}")
    min_neighbors = min(int(min_neighbors), 2 ** 31 - 1)
    with torch.no_grad():
        mask, saliency, eigenvalues, _ = _C_iss.iss_keypoints(points.detach(), lengths, rs, rn, g21, g32, min_neighbors)
        return ISSKeypoints(mask, saliency, eigenvalues, mask.sum(1))


def cloud_resolution(points: Union[torch.Tensor, Pointclouds], lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(N,) float32: the mean distance of a cloud's points to their nearest other point, over its live rows (0 for a
    cloud of fewer than two points).  Open3D's compute_iss_keypoints defaults to salient_radius = 6 x and
    non_max_radius = 4 x this value; here the radii are scalars for the whole batch, so take them from one cloud's
    resolution or from the batch's mean."""
    points, lengths = _padded(points, lengths)
    N, P, _ = points.shape
    if lengths is None:
        lengths = torch.full((N,), P, dtype=torch.int64, device=points.device)
    with torch.no_grad():
        lengths = lengths.clamp(0, P)
        if P < 2:
            return torch.full((N,), 0.0, dtype=torch.float32, device=points.device)
        d2 = knn_points(points.detach(), points.detach(), lengths, lengths, K=2).dists[..., 1]
        live = (torch.arange(P, device=points.device)[None, :] < lengths[:, None]) & (lengths[:, None] >= 2)
        total = torch.where(live, d2.sqrt(), torch.full((), 0.0, device=points.device)).sum(1)
        return total / lengths.clamp(min=1).to(torch.float32)


def keypoints_to_padded(mask: torch.Tensor):
    """mask (N, P) bool -> (idx (N, Kmax) int64: the kept rows of every cloud in ascending order, padded with -1;
    num_keypoints (N,) int64), Kmax the largest count (one host read-back).  `idx` feeds `knn_gather` and the searches
    on the kept rows."""
    if not torch.is_tensor(mask) or mask.dim() != 2 or mask.dtype != torch.bool:
        raise ValueError("mask must be a bool tensor of shape (N, P)")
    N, P = mask.shape
    num = mask.sum(1)
    kmax = int(num.max()) if N > 0 and P > 0 else 0
    # a stable sort of "not kept" puts the kept rows first, in ascending order
    order = torch.argsort((~mask).to(torch.int8), dim=1, stable=True)[:, :kmax]
    keep = torch.arange(kmax, device=mask.device)[None, :] < num[:, None]
    return torch.where(keep, order, torch.full((), -1, dtype=torch.int64, device=mask.device)), num
