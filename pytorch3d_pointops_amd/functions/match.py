"""match_features -- putative correspondences between two descriptor tables, with the three filters every descriptor
pipeline offers (Open3D's correspondences_from_features(mutual_filter), PCL's correspondence estimation with its
rejectors): Lowe's ratio test against the second neighbour, a distance cap and the mutual check.  The step between
`fpfh_features` (or learned descriptors) and `ransac_alignment`, whose `corr` argument is what this returns.

The searches are `_C_match.feature_knn` (csrc/feature_match.hip): `knn_points`' results byte for byte, screened on the
matrix cores where that was measured faster.  The filters are elementwise over (N, P1) and are torch ops here.  The
definition is the FEATURE MATCHING block of include/pointops_amd.h.
"""
import math
from collections import namedtuple
from typing import Optional

import torch

from .. import _C, _C_match
from .fpfh import _check_lengths
from .knn_in_radius import _fl32

FeatureMatches = namedtuple("FeatureMatches", "corr dists second num_matches")


def _squared(value, name: str, upper: Optional[float]) -> float:
    """fl32(fl32(v) * fl32(v)) of a positive finite v (at most `upper`): the float64 product of two fp32 values,
    rounded once, is the fp32 product."""
    v = _fl32(value)
    if not (math.isfinite(v) and v > 0.0) or (upper is not None and not float(value) <= upper):
        rng = f"in (0, {upper:g}]" if upper is not None else "positive and finite in float32"
        raise ValueError(f"{name} must be {rng}, got {value}")
    return _fl32(v * v)


@torch.compiler.disable
def match_features(f1: torch.Tensor, f2: torch.Tensor, lengths1: Optional[torch.Tensor] = None,
                   lengths2: Optional[torch.Tensor] = None, *, mutual: bool = True, ratio: Optional[float] = None,
                   max_distance: Optional[float] = None) -> FeatureMatches:
    """For every row i of `f1` (N, P1, D) its nearest row j1 of `f2` (N, P2, D) in squared L2 (float32, `knn_points`'
    distances and tie rule), kept as a match when it passes every filter that is set:

      max_distance  d1 < fl32(max_distance^2), `ball_query`'s comparison
      ratio         d1 < fl32(ratio^2) * d2 against the second nearest distance d2 (Lowe's test on squared distances);
                    a row whose cloud has a single target passes
      mutual        row j1 of `f2` has row i as ITS nearest row of `f1`

    Returns FeatureMatches(corr, dists, second, num_matches): corr (N, P1) int64 = j1 for kept rows, else -1 (the `corr`
    of `ransac_alignment`); dists (N, P1) = d1 and second (N, P1) = d2 for every valid row whatever the filters say
    (second = +inf with a single target; both 0 for rows past `lengths1` and clouds without targets); num_matches (N,)
    int64.  With the defaults `corr` equals `mutual_nearest_neighbors`.  `ratio` lies in (0, 1], `max_distance` is
    positive and finite.  Not differentiable; under torch.compile the call is a graph break."""
    for t, name in ((f1, "f1"), (f2, "f2")):
        if not torch.is_tensor(t) or t.dim() != 3:
            raise ValueError(f"{name} must be a tensor of shape (N, P, D)")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    if f1.shape[0] != f2.shape[0] or f1.shape[2] != f2.shape[2] or f1.shape[2] < 1:
        raise ValueError("f1 and f2 must have the same batch and feature dimensions (D >= 1)")
    N, P1, P2 = f1.shape[0], f1.shape[1], f2.shape[1]
    _check_lengths(lengths1, N, "lengths1")
    _check_lengths(lengths2, N, "lengths2")
    ratio2 = None if ratio is None else _squared(ratio, "ratio", 1.0)
    cap2 = None if max_distance is None else _squared(max_distance, "max_distance", None)
    dev = _C._require_gpu(f1, f2, lengths1, lengths2)
    with torch.no_grad():
        f1 = f1.detach()
        f2 = f1 if f2 is f1 else f2.detach()
        if lengths1 is None:
            lengths1 = torch.full((N,), P1, dtype=torch.int64, device=dev)
        if lengths2 is None:
            lengths2 = torch.full((N,), P2, dtype=torch.int64, device=dev)
        if N == 0 or P1 == 0 or P2 == 0:
            return FeatureMatches(torch.full((N, P1), -1, dtype=torch.int64, device=dev),
                                  torch.full((N, P1), 0.0, dtype=torch.float32, device=dev),
                                  torch.full((N, P1), 0.0, dtype=torch.float32, device=dev),
                                  torch.full((N,), 0, dtype=torch.int64, device=dev))
        idx, d, _ = _C_match.feature_knn(f1, f2, lengths1, lengths2, 2)
        j1, d1, d2 = idx[..., 0], d[..., 0], d[..., 1]
        rows = torch.arange(P1, device=dev)[None, :]
        nearest = (rows < lengths1[:, None]) & (lengths2[:, None] >= 1)
        has_second = nearest & (lengths2[:, None] >= 2)
        keep = nearest
        if cap2 is not None:
            keep = keep & (d1 < cap2)
        if ratio2 is not None:
            keep = keep & (~has_second | (d1 < d2 * ratio2))
        if mutual:
            back = _C_match.feature_knn(f2, f1, lengths2, lengths1, 1)[0][..., 0]
            keep = keep & (back.gather(1, j1) == rows)
        corr = torch.where(keep, j1, -1)
        dists = torch.where(nearest, d1, 0.0)
        second = torch.where(has_second, d2, torch.where(nearest, math.inf, 0.0))
        return FeatureMatches(corr, dists, second, (corr >= 0).sum(dim=1))
