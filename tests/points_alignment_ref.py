"""Float64 checker for the registration feature (functions/points_alignment.py): both definitions restated in plain
float64 torch on the CPU, independent of the package, with autograd.

Alignment (row vectors, Xt = s X R + T).  w (N,P) are the weights, already zero past each cloud's length:
    W = max(sum w, eps);  xm = sum w x / W;  ym = sum w y / W
    C = sum w^2 (x - xm)(y - ym)^T / W = U S V^T;  E = diag(1, .., 1, det(U V^T))  (E = I with allow_reflection)
    R = U E V^T;  s = tr(E S) / max(sum w^2 |x - xm|^2 / W, eps) with estimate_scale, else 1;  T = ym - s xm R
ICP.  Xt_0 = X (or the initial transform applied); iteration i: nn = nearest row of Y (brute force, squared L2, ties to
the lower index, lengths honoured; an empty target cloud answers row 0), (R,T,s) = alignment of X to Y[nn] with the
validity mask as weights and eps = 1e-9, Xt = s X R + T, rmse = sqrt(sum_valid |Xt - Y[nn]|^2 / max(len, 1e-9)),
relative change (prev - rmse) / prev -- 1 on the first iteration, 0 where prev == 0 --, stop when it is <= thr for
every cloud.
"""
from collections import namedtuple

import torch

RefICP = namedtuple("RefICP", "converged rmse Xt R T s history iterations")


def valid_mask(lengths, P):
    return torch.arange(P)[None, :] < torch.as_tensor(lengths).cpu()[:, None]


def alignment(X, Y, w=None, estimate_scale=False, allow_reflection=False, eps=1e-9):
    """X, Y (N,P,d), w (N,P) or None -> R (N,d,d), T (N,d), s (N,), S (N,d); float64, differentiable."""
    X, Y = X.double().cpu(), Y.double().cpu()
    N, P, d = X.shape
    w = torch.ones((N, P), dtype=torch.float64) if w is None else w.double().cpu()
    W = w.sum(1).clamp(min=eps)
    xm = torch.einsum("np,npd->nd", w, X) / W[:, None]
    ym = torch.einsum("np,npd->nd", w, Y) / W[:, None]
    dx = (X - xm[:, None, :]) * w[:, :, None]
    dy = (Y - ym[:, None, :]) * w[:, :, None]
    C = torch.einsum("npa,npb->nab", dx, dy) / W[:, None, None]
    U, S, Vh = torch.linalg.svd(C)
    E = torch.ones((N, d), dtype=torch.float64)
    if not allow_reflection:
        E = torch.cat([E[:, :-1], torch.linalg.det(U @ Vh)[:, None]], dim=1)
    R = (U * E[:, None, :]) @ Vh
    if estimate_scale:
        s = (E * S).sum(1) / ((dx * dx).sum((1, 2)) / W).clamp(min=eps)
    else:
        s = torch.ones(N, dtype=torch.float64)
    T = ym - s[:, None] * torch.einsum("na,nab->nb", xm, R)
    return R, T, s, S


def apply(X, R, T, s):
    return s[:, None, None] * (X.double().cpu() @ R) + T[:, None, :]


def well_determined(S, rel=1e-3):
    """(N,) bool: sigma_{d-1} + sigma_d >= rel * sigma_1 -- the rotation is well determined."""
    return (S[:, -2] + S[:, -1]) >= rel * S[:, 0]


def nearest(Xt, Y, len_x, len_y, chunk=2048):
    """(N,P1) int64: brute-force nearest row of Y for every row of Xt (0 for rows past len_x or an empty target)."""
    N, P1, d = Xt.shape
    idx = torch.zeros((N, P1), dtype=torch.int64)
    for n in range(N):
        lx, ly = int(len_x[n]), int(len_y[n])
        if lx == 0 or ly == 0:
            continue
        y = Y[n, :ly]
        for a in range(0, lx, chunk):
            x = Xt[n, a:min(a + chunk, lx)]
            d2 = torch.zeros((x.shape[0], ly), dtype=torch.float64)
            for k in range(d):
                d2 += (x[:, k, None] - y[None, :, k]) ** 2
            idx[n, a:a + x.shape[0]] = d2.argmin(1)  # the first minimum: ties to the lower index
    return idx


def gather(Y, idx):
    return torch.gather(Y, 1, idx[:, :, None].expand(-1, -1, Y.shape[2]))


def icp(X, Y, len_x=None, len_y=None, init=None, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False,
        allow_reflection=False):
    X, Y = X.double().cpu(), Y.double().cpu()
    N, P1, d = X.shape
    len_x = torch.full((N,), P1) if len_x is None else torch.as_tensor(len_x).cpu()
    len_y = torch.full((N,), Y.shape[1]) if len_y is None else torch.as_tensor(len_y).cpu()
    mask = valid_mask(len_x, P1).double()
    Xt = X.clone() if init is None else apply(X, *[t.double().cpu() for t in init]) * mask[..., None]
    prev, history, converged = None, [], False
    for _ in range(max_iterations):
        Ynn = gather(Y, nearest(Xt, Y, len_x, len_y))
        R, T, s, _ = alignment(X, Ynn, mask, estimate_scale, allow_reflection, 1e-9)
        history.append((R, T, s))
        Xt = apply(X, R, T, s) * mask[..., None]
        rmse = ((((Xt - Ynn) ** 2).sum(2) * mask).sum(1) / len_x.double().clamp(min=1e-9)).sqrt()
        rel = torch.ones_like(rmse) if prev is None else torch.where(prev > 0, (prev - rmse) / prev,
                                                                     torch.zeros_like(rmse))
        prev = rmse
        if bool((rel <= relative_rmse_thr).all()):
            converged = True
            break
    R, T, s = history[-1]
    return RefICP(converged, prev, Xt, R, T, s, history, len(history))


def rotation(axis, angle):
    """(3,3) float64 rotation about `axis` by `angle` (Rodrigues), for the row-vector convention x -> x R."""
    a = torch.as_tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    ang = torch.as_tensor(angle, dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + torch.sin(ang) * K + (1 - torch.cos(ang)) * (K @ K)
