"""The HIP operators as registered torch ops: ``torch.ops.pointops_amd.*``.

Every callable of the operator boundary (`_C.py`, the mirror of the reference's pybind module
csrc/ext.cpp:15-27) is registered with `torch.library.custom_op` -- schema inferred from the signature, a
fake (meta) implementation that gives output shapes / dtypes without touching the GPU, and autograd formulas
for the differentiable ones (the same closed-form backward kernels the eager wrappers use).  That makes the
ops visible to the dispatcher, `torch.compile` (functions/*.py route through these ops while a graph is
being traced) and the autograd profiler.  The implementations ARE the `_C` ctypes calls into
libpointops_amd.so; there is no second code path.

Eager calls of functions/*.py keep calling `_C` directly inside their autograd nodes: the dispatcher costs
~15 us per call on the host, a quarter of a small (B=2, N=1024) query.
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _C

NS = "pointops_amd"
_op = torch.library.custom_op


def _like(t: Tensor, shape, dtype=None) -> Tensor:
    return t.new_empty(tuple(shape), dtype=dtype or t.dtype)


# --------------------------------------------------------------------------- knn
@_op(f"{NS}::knn_points_idx", mutates_args=())
def knn_points_idx(p1: Tensor, p2: Tensor, lengths1: Tensor, lengths2: Tensor, norm: int, K: int,
                   version: int) -> Tuple[Tensor, Tensor]:
    return _C.knn_points_idx(p1, p2, lengths1, lengths2, norm, K, version)


@knn_points_idx.register_fake
def _(p1, p2, lengths1, lengths2, norm, K, version):
    shape = (p1.shape[0], p1.shape[1], K)
    return _like(p1, shape, torch.int64), _like(p1, shape, torch.float32)


@_op(f"{NS}::knn_points_backward", mutates_args=())
def knn_points_backward(p1: Tensor, p2: Tensor, lengths1: Tensor, lengths2: Tensor, idxs: Tensor, norm: int,
                        grad_dists: Tensor) -> Tuple[Tensor, Tensor]:
    return _C.knn_points_backward(p1, p2, lengths1, lengths2, idxs, norm, grad_dists,
                                  deterministic=torch.are_deterministic_algorithms_enabled())


@knn_points_backward.register_fake
def _(p1, p2, lengths1, lengths2, idxs, norm, grad_dists):
    return _like(p1, p1.shape, torch.float32), _like(p2, p2.shape, torch.float32)


def _neighbor_setup(norm_of):
    def setup(ctx, inputs, output):
        p1, p2, lengths1, lengths2 = inputs[:4]
        ctx.save_for_backward(p1, p2, lengths1, lengths2, output[0])
        ctx.norm = norm_of(inputs)
    return setup


def _neighbor_grad(n_inputs):
    def backward(ctx, _grad_idx, grad_dists):
        p1, p2, lengths1, lengths2, idx = ctx.saved_tensors
        g1, g2 = knn_points_backward(p1.float(), p2.float(), lengths1, lengths2, idx, ctx.norm,
                                     grad_dists.float().contiguous())
        return (g1, g2) + (None,) * (n_inputs - 2)
    return backward


knn_points_idx.register_autograd(_neighbor_grad(7), setup_context=_neighbor_setup(lambda inp: inp[4]))


# --------------------------------------------------------------------------- ball query
@_op(f"{NS}::ball_query", mutates_args=())
def ball_query(p1: Tensor, p2: Tensor, lengths1: Tensor, lengths2: Tensor, K: int,
               radius: float) -> Tuple[Tensor, Tensor]:
    return _C.ball_query(p1, p2, lengths1, lengths2, K, radius)


@ball_query.register_fake
def _(p1, p2, lengths1, lengths2, K, radius):
    shape = (p1.shape[0], p1.shape[1], K)
    return _like(p1, shape, torch.int64), _like(p1, shape, torch.float32)


ball_query.register_autograd(_neighbor_grad(6), setup_context=_neighbor_setup(lambda inp: 2))


# --------------------------------------------------------------------------- farthest point sampling
@_op(f"{NS}::sample_farthest_points", mutates_args=())
def sample_farthest_points(points: Tensor, lengths: Tensor, K: Tensor, start_idxs: Tensor,
                           max_K: Optional[int] = None) -> Tensor:
    return _C.sample_farthest_points(points, lengths, K, start_idxs, max_K=max_K)


@sample_farthest_points.register_fake
def _(points, lengths, K, start_idxs, max_K=None):
    if points.shape[0] == 0:
        max_K = 0  # (the wrapper's rule: an empty batch has no columns)
    elif max_K is None:
        max_K = torch.library.get_ctx().new_dynamic_size()  # max(K): known only on the device
    return _like(points, (points.shape[0], max_K), torch.int64)


# --------------------------------------------------------------------------- packed <-> padded
@_op(f"{NS}::packed_to_padded", mutates_args=())
def packed_to_padded(inputs_packed: Tensor, first_idxs: Tensor, max_size: int) -> Tensor:
    return _C.packed_to_padded(inputs_packed, first_idxs, max_size)


@packed_to_padded.register_fake
def _(inputs_packed, first_idxs, max_size):
    return _like(inputs_packed, (first_idxs.shape[0], max_size, inputs_packed.shape[1]))


@_op(f"{NS}::padded_to_packed", mutates_args=())
def padded_to_packed(inputs_padded: Tensor, first_idxs: Tensor, num_inputs: int) -> Tensor:
    return _C.padded_to_packed(inputs_padded, first_idxs, num_inputs)


@padded_to_packed.register_fake
def _(inputs_padded, first_idxs, num_inputs):
    return _like(inputs_padded, (num_inputs, inputs_padded.shape[2]))


def _p2p_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])
    ctx.rows = inputs[0].shape[0]


def _pad_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])
    ctx.max_size = inputs[0].shape[1]


packed_to_padded.register_autograd(
    lambda ctx, g: (padded_to_packed(g.contiguous(), ctx.saved_tensors[0], ctx.rows), None, None),
    setup_context=_p2p_setup)
padded_to_packed.register_autograd(
    lambda ctx, g: (packed_to_padded(g.contiguous(), ctx.saved_tensors[0], ctx.max_size), None, None),
    setup_context=_pad_setup)


# --------------------------------------------------------------------------- neighbour gather
@_op(f"{NS}::gather_neighbors", mutates_args=())
def gather_neighbors(x: Tensor, idx: Tensor, lengths: Optional[Tensor]) -> Tensor:
    return _C.gather_neighbors(x, idx, lengths)


@gather_neighbors.register_fake
def _(x, idx, lengths):
    return _like(x, (idx.shape[0], idx.shape[1], idx.shape[2], x.shape[2]), torch.float32)


@_op(f"{NS}::gather_neighbors_backward", mutates_args=())
def gather_neighbors_backward(grad_out: Tensor, idx: Tensor, lengths: Optional[Tensor], M: int) -> Tensor:
    return _C.gather_neighbors_backward(grad_out, idx, lengths, M,
                                        deterministic=torch.are_deterministic_algorithms_enabled())


@gather_neighbors_backward.register_fake
def _(grad_out, idx, lengths, M):
    return _like(grad_out, (grad_out.shape[0], M, grad_out.shape[3]), torch.float32)


def _gather_setup(ctx, inputs, output):
    x, idx, lengths = inputs
    ctx.has_lengths = lengths is not None
    ctx.save_for_backward(idx, *([lengths] if lengths is not None else []))
    ctx.M = x.shape[1]


def _gather_grad(ctx, grad_out):
    idx = ctx.saved_tensors[0]
    lengths = ctx.saved_tensors[1] if ctx.has_lengths else None
    return gather_neighbors_backward(grad_out.float().contiguous(), idx, lengths, ctx.M), None, None


gather_neighbors.register_autograd(_gather_grad, setup_context=_gather_setup)


# --------------------------------------------------------------------------- covariances
@_op(f"{NS}::point_covariances", mutates_args=())
def point_covariances(knn: Tensor) -> Tensor:
    return _C.point_covariances(knn)


@point_covariances.register_fake
def _(knn):
    return _like(knn, (knn.shape[0], knn.shape[1], knn.shape[3], knn.shape[3]))


@_op(f"{NS}::point_covariances_backward", mutates_args=())
def point_covariances_backward(knn: Tensor, grad_cov: Tensor) -> Tensor:
    return _C.point_covariances_backward(knn, grad_cov)


@point_covariances_backward.register_fake
def _(knn, grad_cov):
    return _like(knn, knn.shape)


point_covariances.register_autograd(
    lambda ctx, g: point_covariances_backward(ctx.saved_tensors[0], g.float().contiguous()),
    setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0].contiguous()))


# --------------------------------------------------------------------------- local frames (normals)
@_op(f"{NS}::local_frames", mutates_args=())
def local_frames(points: Tensor, lengths: Tensor, idx: Tensor, disambiguate: bool) -> Tuple[Tensor, Tensor]:
    return _C.local_frames(points, lengths, idx, disambiguate)


@local_frames.register_fake
def _(points, lengths, idx, disambiguate):
    N, P = points.shape[:2]
    return _like(points, (N, P, 3), torch.float32), _like(points, (N, P, 3, 3), torch.float32)


@_op(f"{NS}::local_frames_backward", mutates_args=())
def local_frames_backward(curvatures: Tensor, frames: Tensor, grad_curvatures: Tensor, grad_frames: Tensor,
                          lengths: Tensor, disambiguate: bool) -> Tensor:
    return _C.local_frames_backward(curvatures, frames, grad_curvatures, grad_frames, lengths, disambiguate)


@local_frames_backward.register_fake
def _(curvatures, frames, grad_curvatures, grad_frames, lengths, disambiguate):
    return _like(frames, frames.shape, torch.float32)


def _local_frames_setup(ctx, inputs, output):
    points, lengths, idx, disambiguate = inputs
    ctx.save_for_backward(points, lengths, idx, *output)
    ctx.disambiguate = disambiguate


def _local_frames_grad(ctx, grad_curvatures, grad_frames):
    # grad_C from the eigenpairs, then the existing covariance chain: gather -> covariance backward -> scatter
    points, lengths, idx, curvatures, frames = ctx.saved_tensors
    gl = torch.zeros_like(curvatures) if grad_curvatures is None else grad_curvatures.float().contiguous()
    gf = torch.zeros_like(frames) if grad_frames is None else grad_frames.float().contiguous()
    grad_cov = local_frames_backward(curvatures, frames, gl, gf, lengths, ctx.disambiguate)
    knn = gather_neighbors(points, idx, lengths)
    grad_knn = point_covariances_backward(knn, grad_cov)
    return gather_neighbors_backward(grad_knn, idx, lengths, points.shape[1]), None, None, None


local_frames.register_autograd(_local_frames_grad, setup_context=_local_frames_setup)


# --------------------------------------------------------------------------- points alignment
@_op(f"{NS}::points_alignment", mutates_args=())
def points_alignment(X: Tensor, Y: Tensor, idx: Optional[Tensor], lengths: Optional[Tensor], weights: Optional[Tensor],
                     estimate_scale: bool, allow_reflection: bool, eps: float) -> Tuple[Tensor, Tensor, Tensor, Tensor,
                                                                                         Tensor]:
    # (always with the fp64 moments: the registered backward starts from them)
    return _C.points_alignment(X, Y, idx, lengths, weights, estimate_scale, allow_reflection, eps, want_moments=True)


@points_alignment.register_fake
def _(X, Y, idx, lengths, weights, estimate_scale, allow_reflection, eps):
    N, _, D = X.shape
    return (_like(X, (N, D, D), torch.float32), _like(X, (N, D), torch.float32), _like(X, (N,), torch.float32),
            _like(X, (N, D), torch.float32), _like(X, (N, _C.alignment_moment_count(D)), torch.float64))


@_op(f"{NS}::points_alignment_backward", mutates_args=())
def points_alignment_backward(X: Tensor, Y: Tensor, lengths: Optional[Tensor], weights: Optional[Tensor],
                              grad_moments: Tensor) -> List[Tensor]:
    gX, gY, gW = _C.points_alignment_backward(X, Y, lengths, weights, grad_moments)
    return [gX, gY] if gW is None else [gX, gY, gW]  # grad_X, grad_Y, then grad_weights where there are weights


@points_alignment_backward.register_fake
def _(X, Y, lengths, weights, grad_moments):
    return [_like(t, t.shape) for t in (X, Y, *([] if weights is None else [weights]))]


def _alignment_setup(ctx, inputs, output):
    X, Y, idx, lengths, weights, estimate_scale, allow_reflection, eps = inputs
    ctx.has_idx = idx is not None
    ctx.has = (lengths is not None, weights is not None)
    ctx.save_for_backward(X, Y, output[4], *[t for t in (lengths, weights) if t is not None])
    ctx.flags = (estimate_scale, allow_reflection, eps)


def _alignment_grad(ctx, gR, gT, gs, _gsing, _gmoments):
    # functions/points_alignment.py `_alignment.backward`: float64 autograd of the N tiny solves, then one kernel
    from .functions.points_alignment import _solve_from_moments

    if ctx.has_idx:
        raise RuntimeError("points_alignment: differentiable without idx only (pointops_points_alignment_backward)")
    X, Y, moments, *rest = ctx.saved_tensors
    lengths = rest.pop(0) if ctx.has[0] else None
    weights = rest.pop(0) if ctx.has[1] else None
    N, P, d = X.shape
    if N == 0 or P == 0:  # no element at all: the (empty) inputs are their own gradients, no kernel runs
        return X.detach(), Y.detach(), None, None, (weights.detach() if weights is not None else None), None, None, None
    has = (lengths > 0)[:, None] if lengths is not None else torch.ones((N, 1), dtype=torch.bool, device=X.device)
    px = torch.where(has, X[:, 0].double(), 0.0)
    py = torch.where(has, Y[:, 0].double(), 0.0)
    with torch.enable_grad():
        M = moments.detach().clone().requires_grad_(True)
        outs = _solve_from_moments(M, px, py, d, *ctx.flags)
        wanted = [(o, g.double()) for o, g in zip(outs, (gR, gT, gs)) if o.requires_grad and g is not None]
        (gM,) = torch.autograd.grad([o for o, _ in wanted], [M], [g for _, g in wanted])
    grads = points_alignment_backward(X, Y, lengths, weights, gM)
    return grads[0], grads[1], None, None, (grads[2] if weights is not None else None), None, None, None


points_alignment.register_autograd(_alignment_grad, setup_context=_alignment_setup)


# --------------------------------------------------------------------------- chamfer
@_op(f"{NS}::chamfer_reduce", mutates_args=())
def chamfer_reduce(dists: Tensor, lengths: Tensor, weights: Optional[Tensor], mean: bool) -> Tensor:
    return _C.chamfer_reduce(dists, lengths, weights, mean)


@chamfer_reduce.register_fake
def _(dists, lengths, weights, mean):
    return _like(dists, (dists.shape[0],), torch.float32)


def _chamfer_reduce_setup(ctx, inputs, output):
    dists, lengths, weights, mean = inputs
    ctx.has_w = weights is not None
    ctx.save_for_backward(lengths, *([weights] if weights is not None else []))
    ctx.mean, ctx.P = mean, dists.shape[1]


def _chamfer_reduce_grad(ctx, g):
    # the closed form of functions/chamfer.py `_masked_point_reduce`: g[n] * w[n] / clamp(len[n], 1) for i < len[n]
    lengths = ctx.saved_tensors[0]
    scale = g.float()
    if ctx.has_w:
        scale = scale * ctx.saved_tensors[1]
    if ctx.mean:
        scale = scale / lengths.clamp(min=1)
    mask = torch.arange(ctx.P, device=g.device)[None] < lengths[:, None]
    return scale[:, None] * mask, None, None, None


chamfer_reduce.register_autograd(_chamfer_reduce_grad, setup_context=_chamfer_reduce_setup)


@_op(f"{NS}::chamfer_forward", mutates_args=())
def chamfer_forward(dists: Tensor, idx: Tensor, x_lengths: Tensor, y_lengths: Tensor, weights: Optional[Tensor],
                    x_feats: List[Tensor], y_feats: List[Tensor], abs_cosine: bool, mean: bool) -> Tensor:
    return _C.chamfer_forward(dists, idx, x_lengths, y_lengths, weights, list(x_feats), list(y_feats), abs_cosine,
                              mean)


@chamfer_forward.register_fake
def _(dists, idx, x_lengths, y_lengths, weights, x_feats, y_feats, abs_cosine, mean):
    return _like(dists, (1 + len(x_feats), dists.shape[0]), torch.float32)


@_op(f"{NS}::chamfer_backward", mutates_args=())
def chamfer_backward(x: Tensor, y: Tensor, idx: Tensor, x_lengths: Tensor, y_lengths: Tensor,
                     weights: Optional[Tensor], grad_out: Tensor, norm: int, x_feats: List[Tensor],
                     y_feats: List[Tensor], abs_cosine: bool, mean: bool) -> List[Tensor]:
    gx, gy, gxf, gyf = _C.chamfer_backward(x, y, idx, x_lengths, y_lengths, weights, grad_out, norm, list(x_feats),
                                           list(y_feats), abs_cosine, mean)
    return [gx, gy, *gxf, *gyf]  # grad_x, grad_y, then the x feature grads, then the y feature grads


@chamfer_backward.register_fake
def _(x, y, idx, x_lengths, y_lengths, weights, grad_out, norm, x_feats, y_feats, abs_cosine, mean):
    return [torch.empty_like(t) for t in (x, y, *x_feats, *y_feats)]


# --------------------------------------------------------------------------- sample_pdf (in place)
@_op(f"{NS}::sample_pdf", mutates_args=("outputs",))
def sample_pdf(bins: Tensor, weights: Tensor, outputs: Tensor, eps: float) -> None:
    _C.sample_pdf(bins, weights, outputs, eps)


@sample_pdf.register_fake
def _(bins, weights, outputs, eps):
    return None


def registered_ops():
    """Names of the registered operators (tests check them against `_C`)."""
    return sorted(n for n in dir(getattr(torch.ops, NS)) if not n.startswith("_") and n != "name")
