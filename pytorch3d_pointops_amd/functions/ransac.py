"""ransac_alignment -- robust registration from putative matches, the step between `mutual_nearest_neighbors` and
`iterative_closest_point`.

Descriptor matches between two different scans are mostly wrong (5-30 % inliers is usual for FPFH), and
`corresponding_points_alignment` is a least-squares fit: one bad match in ten moves it.  RANSAC over the matches --
PCL's SampleConsensusPrerejective, Open3D's registration_ransac_based_on_correspondence -- draws thousands of
three-pair hypotheses per cloud, scores each against every match, keeps the one with the most inliers and refines it
on them.  All of it runs in one native call (csrc/ransac.hip): no (N, H, P) residual tensor, no batched SVD, no host
read-back, no floating-point atomics -- bit-reproducible and capturable.  The exact definition -- valid rows, the
counter-based draws, the edge test, the score, the selection, the refinement -- is the comment block of
pointops_ransac_alignment in include/pointops_amd.h.  Nothing here is differentiable.
"""
from collections import namedtuple
from typing import Optional, Union

import torch

from .. import _C_ransac
from ..structures.pointclouds import Pointclouds
from ._consensus import _cloud, _sampling
from .points_alignment import SimilarityTransform

RansacSolution = namedtuple("RansacSolution", "RTs inliers num_inliers rmse best counts hypotheses samples")


@torch.compiler.disable
def ransac_alignment(X: Union[torch.Tensor, Pointclouds], Y: Union[torch.Tensor, Pointclouds],
                     corr: Optional[torch.Tensor] = None, *, inlier_threshold: float, num_hypotheses: int = 4096,
                     estimate_scale: bool = False, edge_length_ratio: float = 0.9, refine_steps: int = 2,
                     seed: int = 0, samples: Optional[torch.Tensor] = None,
                     return_hypotheses: bool = False) -> RansacSolution:
    """The similarity transform (R, T, s), row-vector convention `s X R + T`, that brings the most matched rows of
    `X` (N,P1,3) within `inlier_threshold` of their partners in `Y` (N,P2,3), per cloud.

    `X`, `Y`: float32 padded tensors (full lengths) or `Pointclouds`.  `corr` (N,P1) int64: the row of `Y` that row i
    of `X` is matched to, or -1 -- what `mutual_nearest_neighbors` returns; None: row i matches row i (P1 == P2).  A
    row is a valid match when it lies inside both clouds' lengths; two rows may share a target.

    `num_hypotheses` triples of distinct valid matches are drawn per cloud from the counter-based hash of
    (`seed`, cloud index, hypothesis, draw): the same on every run, for every batch split.  `samples` (N,H,3) int64
    rows of `X` replace the draws (H = its middle dimension).  A triple is thrown out when a row is not a valid match,
    two rows coincide or -- without `estimate_scale`, with `edge_length_ratio` > 0 -- a side of its triangle in `X` and
    the same side in `Y` differ by more than the ratio.  Each remaining triple is aligned
    (`corresponding_points_alignment` of three pairs, no reflection) and counted: the matches with
    |s x R + T - y|^2 <= inlier_threshold^2.  The largest count wins, the lowest index among equals.  The winner is then
    refitted `refine_steps` times on its inliers; a refit is kept while it does not lose inliers.

    Returns RansacSolution(RTs = SimilarityTransform(R (N,3,3), T (N,3), s (N,)), inliers (N,P1) bool, num_inliers
    (N,) int64, rmse (N,) float32 over the inliers, best (N,) int64 = the winning hypothesis or -1; and with
    `return_hypotheses` counts (N,H) int32 (-1: thrown out), hypotheses = SimilarityTransform((N,H,3,3), (N,H,3),
    (N,H)), samples (N,H,3) int64 -- else None).  A cloud without a usable triple gets the identity, no inliers,
    best = -1.  Not differentiable: the outputs never require grad.  Under torch.compile the call is a graph break."""
    X, lengths1 = _cloud(X, "X")
    Y, lengths2 = _cloud(Y, "Y")
    if X.shape[0] != Y.shape[0]:
        raise ValueError("X and Y must have the same batch dimension")
    N, P1, P2 = X.shape[0], X.shape[1], Y.shape[1]
    if corr is None:
        if P1 != P2:
            raise ValueError("corr=None matches row i to row i: X and Y must have the same number of rows")
    elif not torch.is_tensor(corr) or corr.dtype != torch.int64 or corr.shape != (N, P1):
        raise ValueError("corr must be an int64 tensor of shape (N, P1)")
    num_hypotheses, refine_steps, seed = _sampling(samples, N, num_hypotheses, refine_steps, seed,
                                                   _C_ransac.RANSAC_MAX_HYPOTHESES)
    if not float(inlier_threshold) >= 0.0:
        raise ValueError(f"inlier_threshold must be >= 0, got {inlier_threshold}")
    if not 0.0 <= float(edge_length_ratio) <= 1.0:
        raise ValueError(f"edge_length_ratio must be in [0, 1], got {edge_length_ratio}")
    with torch.no_grad():
        R, T, s, mask, num_inliers, rmse, best, counts, hyp_R, hyp_T, hyp_s, drawn = _C_ransac.ransac_alignment(
            X, Y, corr, lengths1, lengths2, samples, num_hypotheses, seed, inlier_threshold, edge_length_ratio,
            estimate_scale, refine_steps, want_hypotheses=return_hypotheses)
    hypotheses = SimilarityTransform(hyp_R, hyp_T, hyp_s) if return_hypotheses else None
    return RansacSolution(SimilarityTransform(R, T, s), mask, num_inliers, rmse, best, counts, hypotheses, drawn)
