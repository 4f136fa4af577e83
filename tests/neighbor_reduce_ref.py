"""Plain numpy float64 evaluation of the NEIGHBOUR REDUCE block of include/pointops_amd.h: loops over k, nothing else.
Every function also returns the sum of magnitudes its error bound is stated in."""
import numpy as np


def valid_slots(idx, lengths, M):
    K = idx.shape[2]
    ok = (idx >= 0) & (idx < M)
    if lengths is not None:
        ok &= np.arange(K)[None, None, :] < lengths[:, None, None]
    return ok


def forward(x, idx, lengths, weights, reduce):
    """-> out (N,L,C) float64, arg (N,L,C) int64 (255 = none; max only, else None), mag = sum_k |w x| (N,L,C)."""
    x = x.astype(np.float64)
    N, M, C = x.shape
    _, L, K = idx.shape
    ok = valid_slots(idx, lengths, M)
    out, mag = np.zeros((N, L, C)), np.zeros((N, L, C))
    arg = np.full((N, L, C), 255, dtype=np.int64)
    n = np.arange(N)[:, None]
    for k in range(K):
        v = x[n, np.where(ok[:, :, k], idx[:, :, k], 0)]  # (N, L, C)
        m = ok[:, :, k, None]
        if reduce == "max":
            take = m & ((arg == 255) | (v > out))
            out, arg = np.where(take, v, out), np.where(take, k, arg)
        else:
            p = v * (weights[:, :, k, None].astype(np.float64) if weights is not None else 1.0)
            out, mag = out + np.where(m, p, 0.0), mag + np.where(m, np.abs(p), 0.0)
    if reduce == "mean":
        out = out / np.maximum(ok.sum(2), 1)[:, :, None]
    return out, (arg if reduce == "max" else None), mag


def backward(x, idx, lengths, weights, reduce, g, arg=None):
    """-> grad_x, its magnitude sum |w g| and segment length s per target row (N,M), grad_w and its magnitude
    sum_c |g x| (zeros without weights).  `arg`: the forward's, for max."""
    x, g = x.astype(np.float64), g.astype(np.float64)
    N, M, C = x.shape
    _, L, K = idx.shape
    ok = valid_slots(idx, lengths, M)
    count = np.maximum(ok.sum(2), 1)
    gx, gx_mag, seg = np.zeros((N, M, C)), np.zeros((N, M, C)), np.zeros((N, M), dtype=np.int64)
    gw, gw_mag = np.zeros((N, L, K)), np.zeros((N, L, K))
    for n in range(N):
        for l in range(L):
            for k in range(K):
                if not ok[n, l, k]:
                    continue
                m = idx[n, l, k]
                f = 1.0
                if weights is not None:
                    f = float(weights[n, l, k])
                if reduce == "mean":
                    f = float(np.float32(1.0) / np.float32(count[n, l]))
                p = f * g[n, l]
                if reduce == "max":
                    p = np.where(arg[n, l] == k, p, 0.0)
                gx[n, m] += p
                gx_mag[n, m] += np.abs(p)
                seg[n, m] += 1
                gw[n, l, k] = np.sum(g[n, l] * x[n, m])
                gw_mag[n, l, k] = np.sum(np.abs(g[n, l] * x[n, m]))
    return gx, gx_mag, seg, gw, gw_mag


def interpolate(x, idx, d2, lengths_x, lengths_y):
    """knn_interpolate from the fp32 d2 and idx the search returned -> out (N,L,C) float64, max_k |x_k| (N,L,C)."""
    x, d2 = x.astype(np.float64), d2.astype(np.float64)
    N, M, C = x.shape
    _, L, K = idx.shape
    ok = valid_slots(idx, lengths_x, M) & (np.arange(L)[None, :, None] < lengths_y[:, None, None])
    w = np.where(ok, 1.0 / np.maximum(d2, 1e-16), 0.0)
    w = w / np.maximum(w.sum(2, keepdims=True), np.finfo(np.float64).tiny)
    out, top = np.zeros((N, L, C)), np.zeros((N, L, C))
    n = np.arange(N)[:, None]
    for k in range(K):
        v = x[n, np.where(ok[:, :, k], idx[:, :, k], 0)]
        out += w[:, :, k, None] * v
        top = np.maximum(top, np.where(ok[:, :, k, None], np.abs(v), 0.0))
    return out, top
