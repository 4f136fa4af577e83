"""segment_plane / segment_planes -- the dominant plane of a scan (floor, road, table, wall), the step in front of
`cluster_dbscan`: while the floor is still in the cloud, everything standing on it is density-connected through it.

Open3D's `segment_plane`, PCL's SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE: RANSAC draws
thousands of three-point planes per cloud, counts for each the points within `distance_threshold`, keeps the one with
the most and refits it on them.  All of it runs in one native call (csrc/plane.hip): no (N, H, P) residual tensor, no
host read-back, no atomics -- bit-reproducible and capturable.  The exact definition -- valid rows, the counter-based
draws, the plane of a triple and its validity tests, the sign rule, the score, the selection, the refits -- is the
comment block of pointops_segment_plane in include/pointops_amd.h.  Nothing here is differentiable.
"""
import math
import struct
from collections import namedtuple
from typing import Optional, Sequence, Union

import torch

from .. import _C_plane
from ..structures.pointclouds import Pointclouds
from ._consensus import _cloud, _sampling

PlaneSegmentation = namedtuple("PlaneSegmentation", "planes inliers num_inliers rmse best counts hypotheses samples")
PlaneSet = namedtuple("PlaneSet", "planes labels num_inliers")


def _f32(v: float) -> float:
    """`v` as the kernels receive it."""
    return struct.unpack("f", struct.pack("f", v))[0]


def _arguments(points, distance_threshold, num_hypotheses, refine_steps, seed, mask, axis, max_angle_deg, samples):
    """Validation shared by the two public functions -> (points, lengths, mask, axis32, cos32, H, refine_steps, seed)."""
    points, lengths = _cloud(points, "points")
    N, P = points.shape[0], points.shape[1]
    if mask is not None and (not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.shape != (N, P)):
        raise ValueError("mask must be a bool tensor of shape (N, P)")
    num_hypotheses, refine_steps, seed = _sampling(samples, N, num_hypotheses, refine_steps, seed,
                                                   _C_plane.PLANE_MAX_HYPOTHESES)
    try:
        thr = _f32(float(distance_threshold))
    except OverflowError:
        thr = math.inf
    if not (math.isfinite(thr) and thr >= 0.0):
        raise ValueError(f"distance_threshold must be finite and >= 0 in float32, got {distance_threshold}")
    if (axis is None) != (max_angle_deg is None):
        raise ValueError("axis and max_angle_deg come together: pass both or neither")
    axis32 = cos32 = None
    if axis is not None:
        a = [float(v) for v in (axis.tolist() if torch.is_tensor(axis) else axis)]
        norm = math.sqrt(sum(v * v for v in a)) if len(a) == 3 else 0.0
        if len(a) != 3 or not (math.isfinite(norm) and norm > 0.0):
            raise ValueError("axis must be three finite numbers, not all zero")
        if not 0.0 <= float(max_angle_deg) <= 90.0:
            raise ValueError(f"max_angle_deg must be in [0, 90], got {max_angle_deg}")
        axis32 = tuple(_f32(v / norm) for v in a)
        # (90 degrees admits every normal: the rounded cosine of pi / 2 would throw the exactly perpendicular ones out)
        cos32 = 0.0 if float(max_angle_deg) >= 90.0 else min(max(_f32(math.cos(math.radians(float(max_angle_deg)))), 0.0), 1.0)
    return points, lengths, mask, axis32, cos32, thr, num_hypotheses, refine_steps, seed


@torch.compiler.disable
def segment_plane(points: Union[torch.Tensor, Pointclouds], *, distance_threshold: float, num_hypotheses: int = 1024,
                  refine_steps: int = 2, seed: int = 0, mask: Optional[torch.Tensor] = None,
                  axis: Optional[Sequence[float]] = None, max_angle_deg: Optional[float] = None,
                  samples: Optional[torch.Tensor] = None, return_hypotheses: bool = False) -> PlaneSegmentation:
    """The plane `a x + b y + c z + d = 0`, (a, b, c) a unit normal, that has the most rows of `points` (N,P,3) within
    `distance_threshold`, per cloud.

    `points`: a float32 padded tensor (full lengths) or a `Pointclouds`.  `mask` (N,P) bool selects the rows to
    consider; a row outside a cloud's length or outside the mask is never sampled, counted or reported.

    `num_hypotheses` triples of distinct valid rows are drawn per cloud from the counter-based hash of (`seed`, cloud
    index, hypothesis, draw) that `ransac_alignment` uses: the same on every run, for every batch split.  `samples`
    (N,H,3) int64 rows replace the draws (H = its middle dimension).  A triple is thrown out when a row is not valid,
    two rows coincide, the three points are collinear (|e1 x e2|^2 <= 1e-12 |e1|^2 |e2|^2, NaN included) or -- with
    `axis` and `max_angle_deg` -- the normal is further than that angle from the line of `axis` (PCL's perpendicular
    plane: a floor is `axis=(0, 0, 1)`).  The plane of each remaining triple is formed in float64, rounded once, and
    counted: the valid rows with |a x + b y + c z + d| <= distance_threshold in float32.  The largest count wins, the
    lowest index among equals.  The winner is then refitted `refine_steps` times on its inliers (centroid and the
    eigenvector of the smallest eigenvalue of their covariance, in float64); a refit is kept while it does not lose
    inliers and stays inside the cone.  The normal points along `axis` when one is given; otherwise its component of
    largest magnitude is positive.

    Returns PlaneSegmentation(planes (N,4) float32, inliers (N,P) bool, num_inliers (N,) int64, rmse (N,) float32 over
    the inliers, best (N,) int64 = the winning hypothesis or -1; and with `return_hypotheses` counts (N,H) int32 (-1:
    thrown out), hypotheses (N,H,4) float32, samples (N,H,3) int64 -- else None).  A cloud without a usable triple gets
    the plane (0,0,0,0), no inliers, best = -1.  Not differentiable: the outputs never require grad.  Under
    torch.compile the call is a graph break."""
    points, lengths, mask, axis32, cos32, thr, H, refine_steps, seed = _arguments(
        points, distance_threshold, num_hypotheses, refine_steps, seed, mask, axis, max_angle_deg, samples)
    with torch.no_grad():
        planes, inliers, num_inliers, rmse, best, counts, hyp, drawn = _C_plane.segment_plane(
            points, lengths, mask, samples, H, seed, thr, axis32, cos32, refine_steps,
            want_hypotheses=return_hypotheses)
    return PlaneSegmentation(planes, inliers, num_inliers, rmse, best, counts, hyp, drawn)


@torch.compiler.disable
def segment_planes(points: Union[torch.Tensor, Pointclouds], max_planes: int, *, min_inliers: int,
                   distance_threshold: float, num_hypotheses: int = 1024, refine_steps: int = 2, seed: int = 0,
                   mask: Optional[torch.Tensor] = None, axis: Optional[Sequence[float]] = None,
                   max_angle_deg: Optional[float] = None, samples: Optional[torch.Tensor] = None) -> PlaneSet:
    """Up to `max_planes` planes per cloud, peeled one after the other: call k is `segment_plane` with `seed + k` on the
    rows no earlier plane has taken.  Plane k of a cloud counts iff it has at least `min_inliers` inliers and every
    earlier plane of that cloud counted; its inliers then get label k and leave the cloud.  A plane that does not count
    is reported as zeros with `num_inliers` 0.  Only torch ops run between the calls: nothing is read back, and the
    whole function can be captured.

    Returns PlaneSet(planes (N,K,4) float32, labels (N,P) int64 with -1 on the rows of no plane, num_inliers (N,K)
    int64)."""
    if int(max_planes) != max_planes or int(max_planes) < 1:
        raise ValueError(f"max_planes must be an integer >= 1, got {max_planes}")
    if int(min_inliers) != min_inliers or int(min_inliers) < 0:
        raise ValueError(f"min_inliers must be an integer >= 0, got {min_inliers}")
    K, min_inliers = int(max_planes), int(min_inliers)
    pts, lengths, mask, _, _, _, _, _, seed = _arguments(points, distance_threshold, num_hypotheses, refine_steps,
                                                          seed, mask, axis, max_angle_deg, samples)
    if seed + K > 2 ** 63:
        raise ValueError(f"seed + max_planes must stay below 2^63, got {seed} + {K}")
    N, P = pts.shape[0], pts.shape[1]
    with torch.no_grad():
        remaining = mask.clone() if mask is not None else torch.ones((N, P), dtype=torch.bool, device=pts.device)
        if lengths is not None:
            remaining &= torch.arange(P, device=pts.device)[None, :] < lengths[:, None]
        labels = torch.full((N, P), -1, dtype=torch.int64, device=pts.device)
        alive = torch.ones((N,), dtype=torch.bool, device=pts.device)
        planes, nums = [], []
        for k in range(K):
            r = segment_plane(points, distance_threshold=distance_threshold, num_hypotheses=num_hypotheses,
                              refine_steps=refine_steps, seed=seed + k, mask=remaining, axis=axis,
                              max_angle_deg=max_angle_deg, samples=samples)
            alive = alive & (r.num_inliers >= min_inliers)
            take = r.inliers & alive[:, None]
            labels = torch.where(take, k, labels)
            remaining = remaining & ~take
            planes.append(torch.where(alive[:, None], r.planes, 0.0))
            nums.append(torch.where(alive, r.num_inliers, 0))
    return PlaneSet(torch.stack(planes, 1), labels, torch.stack(nums, 1))
