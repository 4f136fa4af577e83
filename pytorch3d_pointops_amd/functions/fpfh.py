"""fpfh_features / point_pair_features / mutual_nearest_neighbors -- local shape descriptors for registration.

ICP needs a starting pose, and a starting pose comes from matching local descriptors: normals -> FPFH (Fast Point
Feature Histograms, Rusu et al. 2009: 33 bins per point, three groups of 11) -> nearest neighbours in feature space
(`knn_points` searches any D) -> `corresponding_points_alignment` -> `iterative_closest_point`.

After the neighbour search the descriptor is two passes over the neighbour table (csrc/fpfh.hip): the pair features
and the per-point histogram (SPFH), then the distance-weighted sum of the neighbours' histograms (FPFH).  The exact
definition -- live slots, the swap rule, the bins, the weights -- is the comment block of pointops_spfh /
pointops_fpfh in include/pointops_amd.h.  Nothing here is differentiable.
"""
from typing import Optional, Tuple, Union

import torch

from .. import _C, _C_descriptors
from ..structures.pointclouds import Pointclouds
from .ball_query import ball_query
from .knn import knn_points
from .points_normals import estimate_pointcloud_normals

FPFH_BINS = _C_descriptors.SPFH_BINS
FPFH_MAX_K = _C_descriptors.SPFH_MAX_K


def _check_cloud(points, name: str = "points") -> None:
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] != 3:
        raise ValueError(f"{name} must be a padded tensor of shape (N, P, 3)")
    if points.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {points.dtype}")


def _check_table(points, normals, idx, lengths) -> None:
    _check_cloud(points)
    _check_cloud(normals, "normals")
    if normals.shape != points.shape:
        raise ValueError("normals must have the shape of points, (N, P, 3)")
    N, P = points.shape[:2]
    if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() != 3 or idx.shape[:2] != (N, P):
        raise ValueError("idx must be an int64 tensor of shape (N, P, K)")
    _check_K(idx.shape[2])
    _check_lengths(lengths, N)


def _check_K(K) -> None:
    if not 1 <= K <= FPFH_MAX_K:
        raise ValueError(f"K must be in 1..{FPFH_MAX_K}, got {K}")


def _check_lengths(lengths, N: int, name: str = "lengths") -> None:
    if lengths is not None and (not torch.is_tensor(lengths) or lengths.dtype != torch.int64
                                or lengths.shape != (N,)):
        raise ValueError(f"{name} must be an int64 tensor of shape (N,)")


@torch.compiler.disable
def point_pair_features(points: torch.Tensor, normals: torch.Tensor, idx: torch.Tensor,
                        lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Point-pair features (N,P,K,4) = (f1, f2, f3, d) of every counted slot of the neighbour table `idx` (N,P,K)
    int64 -- `knn_points` or `ball_query` of the cloud against itself --, zeros for every other slot and for rows past
    `lengths`.

    `points`, `normals` (N,P,3) float32; the normals are used as given.  A slot is counted when its neighbour j is a
    valid row other than i at a distance d > 0 and (p_j - p_i) x n_s != 0; f3 = n_s . (p_t - p_s) / d with the source
    s the end whose normal makes the smaller angle with the connecting line, f2 = v . n_t and
    f1 = atan2(w . n_t, n_s . n_t) in the Darboux frame (n_s, v, w) of the pair.  Not differentiable: the output
    never requires grad."""
    _check_table(points, normals, idx, lengths)
    with torch.no_grad():
        return _C_descriptors.spfh(points, normals, idx, lengths, want_pair_features=True)[0]


@torch.compiler.disable
def fpfh_features(points: Union[torch.Tensor, Pointclouds], normals: Optional[torch.Tensor] = None,
                  lengths: Optional[torch.Tensor] = None, *, K: int = 16, radius: Optional[float] = None,
                  idx: Optional[torch.Tensor] = None, return_spfh: bool = False
                  ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """FPFH descriptors (N,P,33) of padded clouds `points` (N,P,3) float32 with `lengths` (N,), or of a Pointclouds;
    `(fpfh, spfh)` with `return_spfh`.

    Neighbourhoods: `idx` (N,P,K) int64 when given, used as is; else `ball_query(points, points, K=K,
    radius=radius).idx` when `radius` is set; else `knn_points(points, points, K=K).idx` -- the self match is in that
    table and carries no pair, so a point has K - 1 neighbours.  1 <= K <= 255.
    `normals` (N,P,3) float32 are used as given; None: `estimate_pointcloud_normals(points, neighborhood_size=K)`,
    which knows the lengths of a Pointclouds only -- a padded tensor with `lengths` needs its normals passed.
    Bins 0-10, 11-21 and 22-32 are the histograms of f1, f2 and f3 (`point_pair_features`); each group of the SPFH
    sums to 100 (0 for a point without counted neighbours), each group of the FPFH to 200 at most.  Rows past a
    cloud's length are zero.  Bit-reproducible run to run.  Not differentiable: the outputs never require grad.
    Under torch.compile the call is a graph break."""
    if isinstance(points, Pointclouds):
        if lengths is not None:
            raise ValueError("lengths must be None with a Pointclouds: it carries its own")
        cloud, points, lengths = points, points.points_padded(), points.num_points_per_cloud()
    else:
        cloud = points
    _check_cloud(points)
    N, P = points.shape[:2]
    _check_lengths(lengths, N)
    if idx is None:
        _check_K(K)
    if normals is None:
        if cloud is points and lengths is not None:
            raise ValueError("normals=None estimates them from full clouds or a Pointclouds: pass the normals of "
                             "a padded tensor with lengths")
        normals = estimate_pointcloud_normals(cloud, neighborhood_size=idx.shape[2] if idx is not None else K)
    with torch.no_grad():
        points = points.detach()
        if idx is None and radius is None:
            idx = knn_points(points, points, lengths, lengths, K=K).idx
        elif idx is None:
            idx = ball_query(points, points, lengths, lengths, K=K, radius=radius, return_nn=False).idx
        _check_table(points, normals, idx, lengths)
        _, spfh = _C_descriptors.spfh(points, normals.detach(), idx, lengths)
        fpfh = _C_descriptors.fpfh(points, idx, lengths, spfh)
    return (fpfh, spfh) if return_spfh else fpfh


@torch.compiler.disable
def mutual_nearest_neighbors(f1: torch.Tensor, f2: torch.Tensor, lengths1: Optional[torch.Tensor] = None,
                             lengths2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(N,P1) int64: for every row i of `f1` (N,P1,D) the index j of its nearest row of `f2` (N,P2,D) when row i is
    also the nearest row of `f1` to that j, else -1; rows past `lengths1` give -1.  Two `knn_points(K=1)` searches
    (squared L2, any D) and a gather -- with FPFH rows as features, the correspondence search of a registration."""
    for t, name in ((f1, "f1"), (f2, "f2")):
        if not torch.is_tensor(t) or t.dim() != 3:
            raise ValueError(f"{name} must be a tensor of shape (N, P, D)")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    if f1.shape[0] != f2.shape[0] or f1.shape[2] != f2.shape[2]:
        raise ValueError("f1 and f2 must have the same batch and feature dimensions")
    N, P1, P2 = f1.shape[0], f1.shape[1], f2.shape[1]
    _check_lengths(lengths1, N, "lengths1")
    _check_lengths(lengths2, N, "lengths2")
    with torch.no_grad():
        f1, f2 = f1.detach(), f2.detach()
        if lengths1 is None:
            lengths1 = torch.full((N,), P1, dtype=torch.int64, device=f1.device)
        if lengths2 is None:
            lengths2 = torch.full((N,), P2, dtype=torch.int64, device=f1.device)
        if N == 0 or P1 == 0 or P2 == 0:
            _C._require_gpu(f1, f2, lengths1, lengths2)
            return torch.full((N, P1), -1, dtype=torch.int64, device=f1.device)
        fwd = knn_points(f1, f2, lengths1, lengths2, K=1).idx[..., 0]
        bwd = knn_points(f2, f1, lengths2, lengths1, K=1).idx[..., 0]
        rows = torch.arange(P1, device=f1.device)[None, :]
        # (a cloud without targets has padding in both tables: its row 0 would look mutual)
        mutual = (bwd.gather(1, fwd) == rows) & (rows < lengths1[:, None]) & (lengths2[:, None] > 0)
        return torch.where(mutual, fwd, torch.full_like(fwd, -1))
