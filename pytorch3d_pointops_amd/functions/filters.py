"""remove_radius_outlier, remove_statistical_outlier -- the stray returns of a real sensor taken out of a scan before
anything else looks at it: the first step of the chain that `voxel_downsample`, `segment_plane`, `cluster_dbscan`, the
normals, `iss_keypoints` and the descriptors continue.  One far outlier stretches the bounding box every cell grid is
sized from; normals, saliency and descriptors at a stray point are garbage that flows into the matches.

Open3D calls the two filters remove_radius_outlier and remove_statistical_outlier, PCL RadiusOutlierRemoval and
StatisticalOutlierRemoval.  Composed in torch the first is `cluster_dbscan(...).core_mask`, which also pays for the
clustering, the second `knn_points` and half a dozen reductions whose sums depend on the launch; both then need an argsort
and a host read-back to give a cloud.  Here each is one native call (csrc/filters.hip): the radius filter a counting walk
of each point's 3x3x3 cube that stops once the count decides, the statistical filter a fixed-order fp64 reduction behind
the exact `knn_points`, both ending in a stable device-side compaction -- no neighbour table, no host read-back,
capturable, bit-reproducible.  The definitions are the comment block of pointops_radius_outlier in
include/pointops_amd.h.  Nothing here is differentiable.
"""
import math
import struct
from collections import namedtuple
from typing import Optional, Union

import torch

from .. import _C_filters
from ..structures.pointclouds import Pointclouds
from .knn import knn_points

RadiusOutliers = namedtuple("RadiusOutliers", "mask num_kept index counts")
StatisticalOutliers = namedtuple("StatisticalOutliers", "mask num_kept index mean_distance threshold mean std")
SelectedRows = namedtuple("SelectedRows", "points features lengths")


def _f32(value, name, positive):
    """`value` as the kernels receive it: rounded to float32; finite and > 0 (`positive`) or >= 0, or ValueError."""
    try:
        v = struct.unpack("f", struct.pack("f", float(value)))[0]
    except OverflowError:
        v = math.inf
    except (TypeError, ValueError):
        v = math.nan
    if not (math.isfinite(v) and (v > 0.0 if positive else v >= 0.0)):
        raise ValueError(f"{name} must be finite and {'> 0' if positive else '>= 0'} in float32, got {value}")
    return v


def _count(value, name, lo, hi=None):
    try:
        ok = int(value) == value and int(value) >= lo and (hi is None or int(value) <= hi)
    except (TypeError, ValueError, OverflowError):  # (not a number, NaN, inf)
        ok = False
    if not ok:
        raise ValueError(f"{name} must be an integer >= {lo}" + (f" and <= {hi}" if hi is not None else "")
                         + f", got {value}")
    return int(value)


def _padded(points, lengths, max_dim=3):
    if isinstance(points, Pointclouds):
        if lengths is not None:
            raise ValueError("lengths come with the Pointclouds: pass one or the other")
        points, lengths = points.points_padded(), points.num_points_per_cloud()
    if not torch.is_tensor(points) or points.dim() != 3 or not 1 <= points.shape[2] <= max_dim:
        raise ValueError(f"points must be a padded tensor of shape (N, P, D) with 1 <= D <= {max_dim}, or a Pointclouds")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int64
                                or lengths.shape != (points.shape[0],)):
        raise ValueError("lengths must be an int64 tensor of shape (N,)")
    return points, lengths


@torch.compiler.disable
def remove_radius_outlier(points: Union[torch.Tensor, Pointclouds], lengths: Optional[torch.Tensor] = None, *,
                          radius: float, min_neighbors: int, return_counts: bool = False) -> RadiusOutliers:
    """Which points of every cloud of `points` ((N, P, D) float32 padded tensor, D in 1..3, or a `Pointclouds`;
    `lengths` (N,) int64 for a tensor, None = full) have at least `min_neighbors` OTHER points closer than `radius`.

    Two points are neighbours when their squared distance in float32, as `ball_query` forms it, is below
    fl32(radius * radius): a pair at exactly `radius` is not.  `mask` equals `cluster_dbscan(points, radius,
    min_neighbors + 1, lengths).core_mask` on every row with finite coordinates, without the clustering.  The walk of
    a point stops as soon as its count decides; `return_counts=True` makes it finish and return the exact neighbour
    counts.

    Returns RadiusOutliers(mask (N, P) bool, num_kept (N,) int64, index (N, P) int64: the kept rows of every cloud in
    ascending order, then -1 (`select_rows` gathers by it), counts (N, P) int32 or None); padding rows are False / 0.
    Integers only: two calls are equal.  Not differentiable; under torch.compile the call is a graph break."""
    points, lengths = _padded(points, lengths)
    radius = _f32(radius, "radius", positive=True)
    min_neighbors = min(_count(min_neighbors, "min_neighbors", 0), 2 ** 31 - 1)
    with torch.no_grad():
        mask, index, num_kept, counts = _C_filters.radius_outlier(points.detach(), lengths, radius, min_neighbors,
                                                                  want_counts=bool(return_counts))
        return RadiusOutliers(mask, num_kept, index, counts)


@torch.compiler.disable
def remove_statistical_outlier(points: Union[torch.Tensor, Pointclouds], lengths: Optional[torch.Tensor] = None, *,
                               nb_neighbors: int = 20, std_ratio: float = 2.0) -> StatisticalOutliers:
    """Which points of every cloud of `points` ((N, P, D) float32 padded tensor, D in 1..3, or a `Pointclouds`;
    `lengths` (N,) int64 for a tensor, None = full) lie as close to their neighbours as the rest of their cloud does.

    `mean_distance` of a point is the mean distance to its `nb_neighbors` nearest other points (fewer in a smaller
    cloud; 0 in a cloud of one), from the exact `knn_points`, summed in float64 and rounded once.  Over the points of a
    cloud these have the float64 `mean` and the sample standard deviation `std`; a point is kept when its mean distance
    is at most `threshold` = float32(mean + std_ratio * std).  That is PCL's StatisticalOutlierRemoval; Open3D's
    remove_statistical_outlier at nb_neighbors + 1 averages the point's own zero distance in as well, which scales
    every quantity by one constant and gives the same mask.  The two sums follow one tree fixed by the row index alone,
    so two calls are byte-equal and a cloud gives the same result alone and in any batch.

    Returns StatisticalOutliers(mask (N, P) bool, num_kept (N,) int64, index (N, P) int64: the kept rows in ascending
    order, then -1, mean_distance (N, P) float32, threshold (N,) float32, mean (N,) float64, std (N,) float64).
    Not differentiable; under torch.compile the call is a graph break."""
    points, lengths = _padded(points, lengths)
    k1 = _count(nb_neighbors, "nb_neighbors", 1, _C_filters.STAT_MAX_K1 - 1) + 1
    std_ratio = _f32(std_ratio, "std_ratio", positive=False)
    N, P, _ = points.shape
    with torch.no_grad():
        pts = points.detach()
        if N > 0 and P > 0:
            dists = knn_points(pts, pts, lengths, lengths, K=k1).dists
        else:
            dists = pts[..., :1].expand(N, P, k1)  # (nothing to search: a table of no elements)
        mask, index, num_kept, mean_distance, threshold, stats = _C_filters.statistical_outlier(dists, lengths,
                                                                                                std_ratio)
        return StatisticalOutliers(mask, num_kept, index, mean_distance, threshold, stats[:, 0], stats[:, 1])


@torch.compiler.disable
def mask_to_index(mask: torch.Tensor):
    """mask (N, P) bool -> (index (N, P) int64: the rows of every cloud where `mask` holds, in ascending order, then
    -1; num_kept (N,) int64).  The compaction both filters end with, for any mask (`iss_keypoints`', a plane's inliers):
    a stable device-side scan, no argsort and no host read-back.  `index[:, :num_kept.max()]` is
    `keypoints_to_padded(mask)[0]`."""
    if not torch.is_tensor(mask) or mask.dim() != 2 or mask.dtype != torch.bool:
        raise ValueError("mask must be a bool tensor of shape (N, P)")
    with torch.no_grad():
        return _C_filters.mask_compact(mask)


def _gather_rows(t, idx, keep):
    rows = torch.gather(t, 1, idx.clamp(min=0)[..., None].expand(-1, -1, t.shape[2]))
    return rows.masked_fill(~keep[..., None], 0)


def select_rows(points: torch.Tensor, index: torch.Tensor, num_kept: torch.Tensor, features=None) -> SelectedRows:
    """The kept rows of `points` (N, P, D) as a padded batch: SelectedRows(points (N, Kmax, D), features, lengths =
    num_kept), Kmax the largest count (one host read-back), rows past a cloud's count zero.  `index`, `num_kept`: a
    filter's, or `mask_to_index`'s.  `features`: None, a tensor (N, P, C) or a dict of them, gathered the same way."""
    if not torch.is_tensor(points) or points.dim() != 3:
        raise ValueError("points must be a padded tensor of shape (N, P, D)")
    N, P = points.shape[:2]
    if not torch.is_tensor(index) or index.dtype != torch.int64 or index.shape != (N, P):
        raise ValueError("index must be an int64 tensor of shape (N, P)")
    if not torch.is_tensor(num_kept) or num_kept.dtype != torch.int64 or num_kept.shape != (N,):
        raise ValueError("num_kept must be an int64 tensor of shape (N,)")
    named = features if isinstance(features, dict) else ({} if features is None else {"": features})
    for t in named.values():
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[:2] != (N, P):
            raise ValueError("features must be padded tensors of shape (N, P, C)")
    kmax = int(num_kept.max()) if N > 0 and P > 0 else 0
    idx = index[:, :kmax]
    keep = idx >= 0
    out = {k: _gather_rows(t, idx, keep) for k, t in named.items()}
    feats = out if isinstance(features, dict) else out.get("")
    return SelectedRows(_gather_rows(points, idx, keep), feats, num_kept)


def filtered_pointclouds(clouds: Pointclouds, result) -> Pointclouds:
    """A new `Pointclouds` of the rows a filter kept, every feature carried over."""
    sel = select_rows(clouds.points_padded(), result.index, result.num_kept, clouds.features_padded())
    num = sel.lengths.tolist()
    feats = {k: [t[n, :v] for n, v in enumerate(num)] for k, t in sel.features.items()}
    return Pointclouds([sel.points[n, :v] for n, v in enumerate(num)], feats or None)
