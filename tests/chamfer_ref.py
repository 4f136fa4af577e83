"""A float64 restatement of the reference's chamfer_distance (functions/chamfer.py:85-365) -- the checker of every
chamfer route, not a product path.

Neighbours come from the oracle's K=1 search (fp32, ties to the lower index: the reference's own semantics); with
that index fixed, everything else is float64 torch on the CPU with autograd:

* point term from the coordinates: |x - y|^2, or for norm=1 sum |x - y| with the sign of the reference's knn
  backward (x > y ? 1 : -1, so a coordinate tie still has a gradient), held in a detached factor;
* feature term 1 - cos (or 1 - |cos|) with F.cosine_similarity(eps=1e-6), ATen's clamped-norm gradient included;
* rows i >= x_len contribute nothing; an empty target (y_len = 0) gives the oracle's knn / knn_gather values, zeros
  for the point term and for the neighbour's feature;
* weights, the mean / sum / max point reductions, the (x, y) pair for point_reduction=None and the batch
  reductions as the reference has them (all-zero weights, where the product deviates, are not modelled).

`chamfer_distance_ref` returns the outputs and the gradients of sum(output * upstream) over every output.
"""
from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F


class CachedKnn:
    """The oracle's K=1 index per (direction, norm), computed once per case."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.memo = {}

    def __call__(self, key, a, b, la, lb, norm):
        if (key, norm) not in self.memo:
            idx, _ = self.oracle.knn_points_idx(a, b, la, lb, norm, 1)
            self.memo[(key, norm)] = idx[..., 0]
        return self.memo[(key, norm)]


def flatten_outputs(loss, loss_features):
    """[(tag, tensor)] of every output, in a fixed order: "loss" (or "loss0", "loss1" for the (x, y) pair), then
    "lossf/<name>" likewise; None entries are skipped."""
    out = []

    def put(tag, t):
        if isinstance(t, tuple):
            for i, u in enumerate(t):
                put(f"{tag}{i}", u)
        elif t is not None:
            out.append((tag, t))

    put("loss", loss)
    for name in sorted(loss_features or {}):
        put(f"lossf/{name}", loss_features[name])
    return out


def _direction(knn, key, a, b, a_np, b_np, la, lb, a_feats, b_feats, names, w, point_reduction, norm, abs_cosine):
    N, P1, _ = a.shape
    idx = torch.from_numpy(np.clip(knn(key, a_np, b_np, la, lb, norm), 0, max(b.shape[1] - 1, 0)))
    rows = torch.arange(N)[:, None]
    inside = torch.arange(P1)[None] < torch.from_numpy(np.asarray(la, np.int64))[:, None]  # (N, P1)
    has_b = torch.from_numpy(np.asarray(lb, np.int64) > 0)[:, None]  # (N, 1)
    point_ok = inside & has_b
    nearest = b[rows, idx]  # (N, P1, D)
    diff = a - nearest
    if norm == 2:
        d = (diff * diff).sum(-1)
    else:
        sign = torch.where(a.detach() > nearest.detach(), 1.0, -1.0).to(a.dtype)
        d = (sign * diff).sum(-1)
    terms = {"": torch.where(point_ok, d, torch.zeros((), dtype=a.dtype))}
    for name in names:
        near_f = b_feats[name][rows, idx] * has_b[..., None].to(a.dtype)  # knn_gather: zeros for an empty target
        cos = F.cosine_similarity(a_feats[name], near_f, dim=2, eps=1e-6)
        t = 1 - (cos.abs() if abs_cosine else cos)
        terms[name] = torch.where(inside, t, torch.zeros((), dtype=a.dtype))
    if w is not None:
        terms = {k: v * w[:, None] for k, v in terms.items()}
    if point_reduction == "max":
        terms = {k: v.max(1).values for k, v in terms.items()}
    elif point_reduction is not None:
        terms = {k: v.sum(1) for k, v in terms.items()}
        if point_reduction == "mean":
            den = torch.from_numpy(np.asarray(la, np.int64)).clamp(min=1).to(a.dtype)
            terms = {k: v / den for k, v in terms.items()}
    return terms


def chamfer_distance_ref(knn, x, y, x_lengths, y_lengths, x_features=None, y_features=None, weights=None,
                         batch_reduction: Optional[str] = "mean", point_reduction: Optional[str] = "mean", norm=2,
                         single_directional=False, abs_cosine=True, feature_names=None,
                         upstream: Optional[Callable[[str, Tuple[int, ...]], np.ndarray]] = None) -> Dict:
    """x, y: fp32 arrays (N, P, D); lengths int arrays; features dicts of fp32 arrays (N, P, C); weights (N,) or
    None; `knn` a CachedKnn.  upstream(tag, shape) is the gradient of each output (tags of flatten_outputs; ones
    when None).  Returns {"outputs": [(tag, float64 array)], "grad_x", "grad_y", "grad_xf": {name}, "grad_yf": {name}}."""
    names = list(feature_names or [])
    xt = torch.from_numpy(np.asarray(x, np.float32)).double().requires_grad_(True)
    yt = torch.from_numpy(np.asarray(y, np.float32)).double().requires_grad_(True)
    xf = {k: torch.from_numpy(np.asarray(x_features[k], np.float32)).double().requires_grad_(True) for k in names}
    yf = {k: torch.from_numpy(np.asarray(y_features[k], np.float32)).double().requires_grad_(True) for k in names}
    w = None if weights is None else torch.from_numpy(np.asarray(weights, np.float32)).double()
    N = xt.shape[0]
    assert w is None or float(w.sum()) > 0.0, "all-zero weights are not modelled"

    def direction(key, a, b, a_np, b_np, la, lb, af, bf):
        return _direction(knn, key, a, b, a_np, b_np, la, lb, af, bf, names, w, point_reduction, norm, abs_cosine)

    fwd = direction("xy", xt, yt, x, y, x_lengths, y_lengths, xf, yf)
    bwd = None if single_directional else direction("yx", yt, xt, y, x, y_lengths, x_lengths, yf, xf)

    if single_directional:
        both = fwd
    elif point_reduction == "max":
        both = {"": torch.maximum(fwd[""], bwd[""])}
    elif point_reduction is not None:
        both = {k: fwd[k] + bwd[k] for k in fwd}
    else:
        both = {k: (fwd[k], bwd[k]) for k in fwd}

    if batch_reduction is not None:
        both = {k: v.sum() for k, v in both.items()}
        if batch_reduction == "mean":
            div = max(N, 1) if w is None else w.sum()
            both = {k: v / div for k, v in both.items()}

    loss = both[""]
    loss_features = {k: both[k] for k in names} if names else None
    outs = flatten_outputs(loss, loss_features)
    total = xt.new_zeros(())
    for tag, t in outs:
        g = np.ones(tuple(t.shape)) if upstream is None else upstream(tag, tuple(t.shape))
        total = total + (t * torch.from_numpy(np.asarray(g, np.float64))).sum()
    leaves = [xt, yt] + [xf[k] for k in names] + [yf[k] for k in names]
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    grads = [torch.zeros_like(leaf) if g is None else g for leaf, g in zip(leaves, grads)]
    F_ = len(names)
    return dict(outputs=[(tag, t.detach().numpy()) for tag, t in outs],
                grad_x=grads[0].numpy(), grad_y=grads[1].numpy(),
                grad_xf={k: grads[2 + i].numpy() for i, k in enumerate(names)},
                grad_yf={k: grads[2 + F_ + i].numpy() for i, k in enumerate(names)})
