"""Argument checks that `ransac_alignment` and `segment_plane` share: both take clouds as padded tensors or
`Pointclouds`, and both draw `num_hypotheses` triples from `seed` (or read `samples`) and refit `refine_steps` times."""
import torch

from ..structures.pointclouds import Pointclouds


def _cloud(points, name: str):
    """(padded (N,P,3) float32 tensor, lengths or None) of a tensor or a Pointclouds."""
    lengths = None
    if isinstance(points, Pointclouds):
        points, lengths = points.points_padded(), points.num_points_per_cloud()
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[2] != 3:
        raise ValueError(f"{name} must be a padded tensor of shape (N, P, 3) or a Pointclouds")
    if points.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {points.dtype}")
    return points.detach(), lengths


def _sampling(samples, N: int, num_hypotheses, refine_steps, seed, max_hypotheses: int):
    """-> (num_hypotheses, refine_steps, seed) as checked ints; `samples` (N,H,3), when given, sets num_hypotheses."""
    if samples is not None:
        if not torch.is_tensor(samples) or samples.dtype != torch.int64 or samples.dim() != 3 \
                or samples.shape[0] != N or samples.shape[2] != 3:
            raise ValueError("samples must be an int64 tensor of shape (N, H, 3)")
        num_hypotheses = samples.shape[1]
    num_hypotheses, refine_steps, seed = int(num_hypotheses), int(refine_steps), int(seed)
    if not 1 <= num_hypotheses <= max_hypotheses:
        raise ValueError(f"num_hypotheses must be in 1..{max_hypotheses}, got {num_hypotheses}")
    if refine_steps < 0:
        raise ValueError(f"refine_steps must be >= 0, got {refine_steps}")
    if not 0 <= seed < 2 ** 63:
        raise ValueError(f"seed must be in 0..2^63-1, got {seed}")
    return num_hypotheses, refine_steps, seed
