"""The numpy definition of tests/neighbor_mlp_ref.py for the "16-bit features" part of the NEIGHBOUR MLP-MAX block of
include/pointops_amd.h: a = x[j] + center is added in float32, the ReLU applied and h rounded to T through a torch CPU cast
(exactly reproducible, so h and the mask h > 0 are exact); everything after h is float64.  The inputs are float32 arrays
that hold values of T.  Every result comes with `mag`, the same expression on absolute values."""
import numpy as np
import torch

from neighbor_reduce_ref import valid_slots


def _hidden(x, idx, center, ok, dtype):
    """h (N,L,K,C1) float64, 0 in invalid slots, and the mask h > 0 of the valid slots."""
    rows = x[np.arange(x.shape[0])[:, None, None], np.where(ok, idx, 0)].astype(np.float32)
    a = rows if center is None else rows + center.astype(np.float32)[:, :, None, :]
    h = torch.from_numpy(np.maximum(a, np.float32(0))).to(dtype).double().numpy()
    h = np.where(ok[..., None], h, 0)
    return h, h > 0


def forward(x, idx, weight, bias, center, lengths, dtype):
    """-> y, mag (N,L,K,C2) and the valid mask (N,L,K)."""
    ok = valid_slots(idx, lengths, x.shape[1])
    h, _ = _hidden(x, idx, center, ok, dtype)
    b = np.zeros(weight.shape[1]) if bias is None else bias.astype(np.float64)
    return h @ weight.astype(np.float64) + b, h @ np.abs(weight.astype(np.float64)) + np.abs(b), ok


def backward(x, idx, weight, center, lengths, g, out, arg, relu_out, dtype):
    """`out`, `arg`: the device's, so the selection is the same on both sides.
    -> {x, center, weight, bias: (grad, mag)}, s (N,M) entries per target row."""
    (N, M, C1), (_, L, K) = x.shape, idx.shape
    ok = valid_slots(idx, lengths, M)
    h, pos = _hidden(x, idx, center, ok, dtype)
    w = weight.astype(np.float64)
    gy = np.where((arg != 255) & ((out > 0) | (not relu_out)), g, 0).astype(np.float64)
    sel = (arg[:, :, None, :] == np.arange(K)[None, None, :, None]).astype(np.float64)  # (N,L,K,C2)
    d = [np.where(pos, np.einsum("nlkc,ic->nlki", sel * gv[:, :, None, :], wv), 0)
         for gv, wv in ((gy, w), (np.abs(gy), np.abs(w)))]
    gx, s = np.zeros((2, N, M, C1)), np.zeros((N, M), dtype=np.int64)
    n, l, k = np.nonzero(ok)
    for t in range(2):
        np.add.at(gx[t], (n, idx[n, l, k]), d[t][n, l, k])
    np.add.at(s, (n, idx[n, l, k]), 1)
    hsel = np.take_along_axis(h, np.where(arg == 255, 0, arg).astype(np.int64)[..., None], 2)  # (N,L,C2,C1)
    gw = [np.einsum("nlc,nlci->ic", gv, hsel) for gv in (gy, np.abs(gy))]
    gb = [gv.sum((0, 1)) for gv in (gy, np.abs(gy))]
    return dict(x=(gx[0], gx[1]), center=(d[0].sum(2), d[1].sum(2)), weight=tuple(gw), bias=tuple(gb)), s
