"""cluster_dbscan / euclidean_clusters -- a raw scan cut into objects, the step in front of the registration chain
(normals -> FPFH -> mutual matches -> `ransac_alignment` -> ICP), which takes a cloud as given.

Density clustering (Open3D's cluster_dbscan, scikit-learn's DBSCAN; with min_points = 1 PCL's
EuclideanClusterExtraction) needs the connected components of the radius graph.  Composed in torch that is either a
dense P x P matrix with min-label propagation repeated up to the graph's diameter or a capped ball_query table that
silently drops edges.  Here it is one native call (csrc/cluster.hip): the cell grid of the exact searches, a walk of
each point's 3x3x3 cube under ball query's certificate, a lock-free union-find whose roots are the smallest indices,
a flatten and a relabel -- exact, canonical, integer-only, no host read-back, capturable.  The definition is the
comment block of pointops_cluster_dbscan in include/pointops_amd.h.  Nothing here is differentiable.
"""
import math
import struct
from collections import namedtuple
from typing import Optional, Union

import torch

from .. import _C_cluster
from ..structures.pointclouds import Pointclouds

DBSCANClusters = namedtuple("DBSCANClusters", "labels num_clusters core_mask")


@torch.compiler.disable
def cluster_dbscan(points: Union[torch.Tensor, Pointclouds], eps: float, min_points: int = 10,
                   lengths: Optional[torch.Tensor] = None) -> DBSCANClusters:
    """DBSCAN of every cloud of `points` ((N, P, D) float32 padded tensor, D in 1..3, or a `Pointclouds`; `lengths`
    (N,) int64 for a tensor, None = full).

    Two points are neighbours when their squared distance, in float32 as `ball_query` forms it, is below
    `eps * eps`.  A point with at least `min_points` neighbours, itself included, is a core point; the clusters are
    the connected components of the neighbour graph on the core points, numbered from 0 in the order of their smallest
    member; a non-core point next to a core point takes the smallest label among its core neighbours; every other
    point, and every padding row, is noise: -1.  The result does not depend on the order of arrival of anything: two
    calls are bit-equal.  It equals scikit-learn's `DBSCAN(eps, min_samples=min_points)` and Open3D's
    `cluster_dbscan` except for pairs at exactly `eps` (they compare `<=`, in float64).

    Returns DBSCANClusters(labels (N, P) int64, num_clusters (N,) int64, core_mask (N, P) bool).  Not differentiable;
    under torch.compile the call is a graph break."""
    if isinstance(points, Pointclouds):
        if lengths is not None:
            raise ValueError("lengths come with the Pointclouds: pass one or the other")
        points, lengths = points.points_padded(), points.num_points_per_cloud()
    if not torch.is_tensor(points) or points.dim() != 3 or not 1 <= points.shape[2] <= 3:
        raise ValueError("points must be a padded tensor of shape (N, P, D) with D in 1..3, or a Pointclouds")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int64
                                or lengths.shape != (points.shape[0],)):
        raise ValueError("lengths must be an int64 tensor of shape (N,)")
    try:
        eps32 = struct.unpack("f", struct.pack("f", float(eps)))[0]  # as the kernels receive it
    except OverflowError:
        eps32 = math.inf
    if not (math.isfinite(eps32) and eps32 > 0.0):
        raise ValueError(f"eps must be finite and > 0 in float32, got {eps}")
    if int(min_points) != min_points or int(min_points) < 1:
        raise ValueError(f"min_points must be an integer >= 1, got {min_points}")
    min_points = min(int(min_points), 2 ** 31 - 1)
    with torch.no_grad():
        labels, num_clusters, core_mask = _C_cluster.cluster_dbscan(points.detach(), lengths, eps32, min_points)
    return DBSCANClusters(labels, num_clusters, core_mask)


def euclidean_clusters(points: Union[torch.Tensor, Pointclouds], tolerance: float,
                       lengths: Optional[torch.Tensor] = None) -> DBSCANClusters:
    """Euclidean cluster extraction (PCL): the connected components of the graph that joins points closer than
    `tolerance` -- `cluster_dbscan` with min_points = 1, where every point with finite coordinates is a core point."""
    return cluster_dbscan(points, tolerance, min_points=1, lengths=lengths)
