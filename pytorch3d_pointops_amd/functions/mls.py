"""smooth_mls -- moving-least-squares smoothing: the stage of the scan-processing chain that repairs the points which
the filters keep.  Sensor noise sits along the surface normal, and the normals, the ISS eigenvalue ratios and the FPFH
bins downstream are second-order statistics of a neighbourhood that a fraction of the point spacing moves.

MLS (Alexa et al. 2003; PCL's MovingLeastSquares at polynomial order 1; the plane fit inside APSS / RIMLS) projects
every point onto the plane fitted to its weighted radius neighbourhood.  Composed in torch that is a ball_query table
capped at the largest neighbourhood, a gathered (N, P, K, 3) tensor, a weighted covariance, a batched eigh and a
projection.  Here it is one native call (csrc/mls.hip): the cell grid of the exact searches and one walk of each
point's 3x3x3 cube under ball query's certificate, the weighted moments summed in integers -- exact, order-free, no
neighbour table and no cap on the support, no host read-back, capturable.  The definition is the comment block of
pointops_mls_smooth in include/pointops_amd.h.  Nothing here is differentiable.
"""
from collections import namedtuple
from typing import Optional, Union

import torch

from .. import _C_mls
from ..structures.pointclouds import Pointclouds
from .iss import _f32, _padded

MLSSmoothing = namedtuple("MLSSmoothing", "points normals curvature num_neighbors status")

MLS_MAX_POINTS = 2 ** 20  # per cloud: the int64 moments stay below 2^63 (csrc/mls_fit.h)
MLS_MAX_ITERATIONS = 65536


@torch.compiler.disable
def smooth_mls(points: Union[torch.Tensor, Pointclouds], lengths: Optional[torch.Tensor] = None, *, radius: float,
               min_neighbors: int = 3, iterations: int = 1, return_moments: bool = False):
    """Moving-least-squares smoothing of every cloud of `points` ((N, P, 3) float32 padded tensor or a `Pointclouds`;
    `lengths` (N,) int64 for a tensor, None = full).

    The support of a point is every point closer than `radius` (squared distance in float32 as `ball_query` forms it,
    the point itself included; there is no cap on its size), weighted by the compactly supported quartic
    (1 - d^2 / radius^2)^4.  The point moves along the normal of the plane fitted to the support -- the eigenvector of
    the smallest eigenvalue l0 <= l1 <= l2 of the weighted covariance, through the weighted mean -- onto that plane.
    `normals` are unit vectors whose component of largest magnitude is positive (orient them afterwards where a
    consistent side matters), and the point moves along exactly the float32 vector that is returned; `curvature` is
    the surface variation l0 / (l0 + l1 + l2), `num_neighbors` the size of the support.  `status` is 0 for a smoothed row, 1 for a row with fewer than `min_neighbors` points in its support
    and 2 for a support that determines no plane (l1 <= 2^-20 l2: collinear or coincident points); rows of status 1
    and 2 keep their point, with normal 0 and curvature 0.  `iterations` = k applies the map k times, each pass on the
    moved points; normals, curvature, num_neighbors and status are those of the last pass.  The radius is a scalar for
    the whole batch.  The weights are quantized to 12 bits and the offsets to 2^-15 of the radius and summed in
    integers, so two calls are bit-equal and a cloud's result depends neither on the rest of the batch nor on the
    order of its rows; each cloud holds at most 2^20 points.

    Returns MLSSmoothing(points (N, P, 3) float32, normals (N, P, 3) float32, curvature (N, P) float32, num_neighbors
    (N, P) int64, status (N, P) uint8); padding rows are 0.  With `return_moments` the pair (MLSSmoothing, moments
    (N, P, 10) int64: the integer sums W, M1[3], M2[6] of the last pass).  Not differentiable; under torch.compile the
    call is a graph break."""
    points, lengths = _padded(points, lengths)
    r = _f32(radius, "radius")
    if int(min_neighbors) != min_neighbors or int(min_neighbors) < 0:
        raise ValueError(f"min_neighbors must be an integer >= 0, got {min_neighbors}")
    if int(iterations) != iterations or not 1 <= int(iterations) <= MLS_MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer in [1, {MLS_MAX_ITERATIONS}], got {iterations}")
    if points.shape[1] > MLS_MAX_POINTS:
        raise ValueError(f"smooth_mls takes clouds of up to 2^20 points, got P = {points.shape[1]}")
    min_neighbors = min(int(min_neighbors), 2 ** 31 - 1)
    with torch.no_grad():
        *out, moments = _C_mls.mls_smooth(points.detach(), lengths, r, min_neighbors, int(iterations),
                                          want_moments=bool(return_moments))
    result = MLSSmoothing(*out)
    return (result, moments) if return_moments else result
