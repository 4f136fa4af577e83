"""registration_icp, evaluate_registration -- the refinement of a pose: the last link of the chain that the outlier
filters, `voxel_downsample`, the normals, `iss_keypoints`, `fpfh_features`, `mutual_nearest_neighbors` and
`ransac_alignment` lead up to.

Open3D calls them registration_icp (with TransformationEstimationPointToPlane / PointToPoint) and
evaluate_registration; PCL's IterativeClosestPoint with setMaxCorrespondenceDistance is the point-to-point half.  They
differ from `iterative_closest_point` (PyTorch3D's, kept beside them unchanged) in the two ways that matter on real
scans: a correspondence farther than `max_correspondence_distance` does not pull on the result, so the rows outside
the overlap of two scans cannot drag it off; and the default error is point-to-plane, which does not slide along a
smooth surface a fraction of the point spacing per iteration.

Every step is one native call (csrc/registration.hip): the exact K=1 search on a workspace the run owns (the grid over
the target is built once), one fused pass over the rows into 29 fp64 sums per cloud, one tiny solve per cloud, one
apply pass.  The per-cloud state -- the accumulated fp64 transform, the previous fitness and rmse, frozen or not --
stays on the device; the host loop reads back one 4-byte word every `check_every` steps, or never.  The definition of
every stage is the REGISTRATION block of include/pointops_amd.h.  Row-vector convention, as in points_alignment.py:
a transform maps x to x R + T.  Nothing here is differentiable.
"""
import math
import struct
from collections import namedtuple
from typing import Optional, Union

import torch

from .. import _C, _C_registration
from ..structures.pointclouds import Pointclouds

RegistrationResult = namedtuple(
    "RegistrationResult",
    "R T fitness inlier_rmse num_correspondences correspondences converged iterations status Xt history")
RegistrationHistory = namedtuple("RegistrationHistory", "R T fitness inlier_rmse")

ESTIMATIONS = tuple(sorted(_C_registration.ESTIMATIONS))
_LIMIT = "the fused path covers float32 clouds of dimension 3 in batches of 1 <= N < 65536"


def _cloud(x, name):
    """(padded points, lengths or None, the container or None)"""
    if isinstance(x, Pointclouds):
        return x.points_padded(), x.num_points_per_cloud(), x
    if not torch.is_tensor(x):
        raise ValueError(f"{name} must be a padded tensor of shape (N, P, 3) or a Pointclouds")
    return x, None, None


def _full_lengths(points):
    return torch.full((points.shape[0],), points.shape[1], dtype=torch.int64, device=points.device)


def _distance(value):
    try:
        v = struct.unpack("f", struct.pack("f", float(value)))[0]
    except OverflowError:
        v = math.inf
    except (TypeError, ValueError):
        v = math.nan
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"max_correspondence_distance must be finite and > 0 in float32, got {value}")
    return v


def _threshold(value, name):
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = math.nan
    if math.isnan(v):
        raise ValueError(f"{name} must be a number, got {value}")
    return v


def _search(value):
    if value not in _C_registration.SEARCHES:
        raise ValueError(f"search must be one of {_C_registration.SEARCHES}, got {value!r}")


def _transform(transform, N, like, name):
    """(R (N,3,3), T (N,3)) fp32 on the device of `like`, or (None, None): a SimilarityTransform with s == 1 or an
    (R, T) pair."""
    if transform is None:
        return None, None
    try:
        parts = tuple(transform)
    except TypeError:
        parts = ()
    if len(parts) not in (2, 3) or not all(torch.is_tensor(t) for t in parts):
        raise ValueError(f"{name} has to be a SimilarityTransform (R, T, s) with s == 1 or an (R, T) pair of tensors")
    R, T = parts[0], parts[1]
    if R.shape != (N, 3, 3) or T.shape != (N, 3) or (len(parts) == 3 and parts[2].shape != (N,)):
        raise ValueError(f"{name}: R has to be of shape (N, 3, 3), T of shape (N, 3) and s of shape (N,)")
    if len(parts) == 3 and not (like.is_cuda and torch.cuda.is_current_stream_capturing()) \
            and not bool((parts[2] == 1).all()):
        raise ValueError(f"{name}: registration is rigid, the scale s has to be 1")
    return tuple(t.detach().to(device=like.device, dtype=torch.float32).contiguous() for t in (R, T))


def _prepare(source, target, max_correspondence_distance, transform, transform_name, target_normals, estimation):
    X, len_x, source_clouds = _cloud(source, "source")
    Y, len_y, target_clouds = _cloud(target, "target")
    if estimation not in ESTIMATIONS:
        raise ValueError(f"estimation must be one of {ESTIMATIONS}, got {estimation!r}")
    r_max = _distance(max_correspondence_distance)
    if X.dim() != 3 or Y.dim() != 3 or X.shape[2] != 3 or Y.shape[2] != 3 or X.dtype != torch.float32 \
            or Y.dtype != torch.float32:
        raise ValueError(f"source and target must be float32 of shape (N, P, 3): {_LIMIT}")
    N = X.shape[0]
    if N == 0 or Y.shape[0] != N:
        raise ValueError(f"source and target must have the same batch size N >= 1: {_LIMIT}")
    if target_normals is None and target_clouds is not None:
        target_normals = target_clouds.get_features_padded("normals")
    if estimation == "point_to_plane":
        if target_normals is None:
            raise ValueError("point_to_plane needs the normals of the target: pass target_normals (N, P2, 3), or a "
                             "Pointclouds with the feature \"normals\" (estimate_pointcloud_normals computes them)")
        if not torch.is_tensor(target_normals) or target_normals.shape != Y.shape \
                or target_normals.dtype != torch.float32:
            raise ValueError("target_normals must be float32 of the target's shape (N, P2, 3)")
    else:
        target_normals = None
    R0, T0 = _transform(transform, N, X, transform_name)
    _C._require_gpu(X, Y, target_normals, len_x, len_y)  # "no CPU fallback"
    if min(X.shape[1], Y.shape[1]) < 1:
        raise ValueError("source and target must have at least one (padded) row per cloud")
    len_x = _full_lengths(X) if len_x is None else len_x
    len_y = _full_lengths(Y) if len_y is None else len_y
    return source_clouds, (X.detach(), Y.detach(), None if target_normals is None else target_normals.detach(),
                           len_x, len_y, R0, T0, r_max, estimation)


def _result(state, source_clouds) -> RegistrationResult:
    history = RegistrationHistory(state.R, state.T, state.fitness, state.inlier_rmse)
    Xt = state.Xt if source_clouds is None else source_clouds.update_padded(state.Xt)
    return RegistrationResult(state.R[-1], state.T[-1], state.fitness[-1], state.inlier_rmse[-1],
                              state.num_correspondences, state.correspondences,
                              state.status == _C_registration.CONVERGED, state.iterations, state.status, Xt, history)


@torch.compiler.disable
def registration_icp(
    source: Union[torch.Tensor, Pointclouds],
    target: Union[torch.Tensor, Pointclouds],
    max_correspondence_distance: float,
    init_transform=None,
    estimation: str = "point_to_plane",
    target_normals: Optional[torch.Tensor] = None,
    max_iterations: int = 30,
    relative_fitness: float = 1e-6,
    relative_rmse: float = 1e-6,
    check_every: int = 1,
    search: str = "exact",
) -> RegistrationResult:
    """Trimmed ICP of every cloud of `source` (N, P1, 3) onto the cloud of `target` (N, P2, 3) with the same batch
    index: float32 CUDA padded tensors (every row valid) or `Pointclouds`.

    Starting from `init_transform` (a `SimilarityTransform` with s == 1 or an `(R, T)` pair; default the identity),
    every step finds the nearest target row of every transformed source row (the exact `knn_points`, K = 1), keeps the
    pairs closer than `max_correspondence_distance` (squared distance in float32 below fl32(r * r), `ball_query`'s
    rule), and reports `fitness` = inliers / source rows and `inlier_rmse` over them.  A cloud freezes as converged
    (status 0) once both moved by less than `relative_fitness` and `relative_rmse` since the previous step (absolute
    differences, as in Open3D).  Otherwise the transform is updated: "point_to_plane" solves the 6 x 6 normal equations
    of sum ((x R + T - y) . n)^2 over the inliers, with `target_normals` (N, P2, 3; for a `Pointclouds` target the
    feature "normals" by default) used as given, and composes the exact rotation of the solved angles onto the
    accumulated float64 transform; "point_to_point" is the Kabsch solve of `corresponding_points_alignment` over the
    inliers.  Fewer than 6 (3) inliers, or normal equations that do not determine the motion (one plane as the target),
    freeze the cloud as degenerate (status 1) with its transform unchanged.  After at most `max_iterations` updates one
    evaluate-only step makes the returned fitness belong to the returned transform; a cloud still running then has
    status 2.

    The loop reads one 4-byte word from the device every `check_every` steps and stops when every cloud is frozen;
    `check_every=0` never reads -- it enqueues `max_iterations + 1` steps, which frozen clouds pass through untouched --
    gives the same bytes, and can be captured into a HIP graph (`graphs.capture`).

    Returns RegistrationResult(R (N,3,3), T (N,3), fitness (N,), inlier_rmse (N,), num_correspondences (N,) int64,
    correspondences (N,P1) int64: the target row of every inlier, else -1, converged (N,) bool, iterations (N,) int32:
    updates applied, status (N,) int32, Xt: the transformed source (a `Pointclouds` when `source` is one; padded rows
    zero), history: RegistrationHistory(R, T, fitness, inlier_rmse) with a leading dimension of `max_iterations + 1`
    steps, a frozen cloud repeating its last entry).

    All sums are float64 in a fixed order: two calls are byte-equal and a cloud gives the same bytes alone and in any
    batch of the same padded widths.  Not differentiable; under torch.compile the call is a graph break.  `target`
    must not be written while the call runs.

    `search="bounded"` replaces the exact search of every step by `knn_in_radius` with K = 1 and radius
    `max_correspondence_distance`: the pairs a step keeps are inside that radius anyway, so every output is byte-equal
    to `search="exact"`, and a source row with nothing nearby (clutter, the part of a scan outside the overlap) costs one
    walk of an empty cube where the exact search scans the whole target for it.  It is not the default because it
    loses where the radius is large against the point spacing -- the cube of a row holds about 27 rho (1.001 r)^3
    target rows -- and telling the two cases apart needs the target's extent, which lives on the device: the choice is
    the caller's."""
    _search(search)
    max_iterations, check_every = int(max_iterations), int(check_every)
    if max_iterations < 1:
        raise ValueError("max_iterations has to be >= 1.")
    if check_every < 0:
        raise ValueError("check_every has to be >= 0 (0: never read the device).")
    thresholds = _threshold(relative_fitness, "relative_fitness"), _threshold(relative_rmse, "relative_rmse")
    source_clouds, args = _prepare(source, target, max_correspondence_distance, init_transform, "init_transform",
                                   target_normals, estimation)
    with torch.no_grad():
        state = _C_registration.RegistrationState(*args, max_iterations + 1, *thresholds, search=search)
        stopped = False
        for i in range(max_iterations):
            state.step(update=True)
            if check_every and (i + 1) % check_every == 0 and int(state.all_frozen.item()):
                stopped = True
                break
        if stopped:
            state.repeat_last_entry()
        else:
            state.step(update=False)
        return _result(state, source_clouds)


@torch.compiler.disable
def evaluate_registration(
    source: Union[torch.Tensor, Pointclouds],
    target: Union[torch.Tensor, Pointclouds],
    max_correspondence_distance: float,
    transform=None,
    search: str = "exact",
) -> RegistrationResult:
    """`fitness`, `inlier_rmse` and the correspondences of `source` under `transform` (default the identity) against
    `target`: exactly the evaluate-only step of `registration_icp`, same arguments, same result type (R, T = the
    transform in float32, iterations 0, status 2, history of one entry).  `search`: as in `registration_icp`."""
    _search(search)
    source_clouds, args = _prepare(source, target, max_correspondence_distance, transform, "transform", None,
                                   "point_to_point")
    with torch.no_grad():
        state = _C_registration.RegistrationState(*args, 1, 0.0, 0.0, search=search)
        state.step(update=False)
        return _result(state, source_clouds)
