"""The numpy definition of the "two layers" part of the NEIGHBOUR MLP-MAX block of include/pointops_amd.h, in the manner
of tests/neighbor_mlp16_ref.py: h1 goes through the exactly reproducible torch CPU cast; everything after h1 is float64
(h2 is NOT rounded here: its rounding is part of what the bounds allow).  The inputs are float32 arrays that hold values
of T.  Every result comes with `mag`, the same expression on absolute values (for h2: |h1| @ |weight| + |bias| where the
pre-activation is positive).
`amb`: the valid (edge, c2) entries whose float64 pre-activation z = h1 @ weight + bias lies within
(C1 + 2) 2^-23 (|h1| @ |weight| + |bias|) of 0.  h1 is exact and a product of two T values is exact in fp32, so the device's
sign of z can differ from float64's only there: only there is the hidden mask h2 > 0 undetermined.  (Where the magnitude
itself is 0 every term is an exact zero on both sides, and the entry is not ambiguous.)"""
import numpy as np

from neighbor_mlp16_ref import _hidden
from neighbor_reduce_ref import valid_slots


def _layers(x, idx, weight, bias, center, lengths, dtype):
    ok = valid_slots(idx, lengths, x.shape[1])
    h1, pos1 = _hidden(x, idx, center, ok, dtype)
    w = weight.astype(np.float64)
    b = np.zeros(w.shape[1]) if bias is None else bias.astype(np.float64)
    z, zmag = h1 @ w + b, h1 @ np.abs(w) + np.abs(b)
    amb = ok[..., None] & (zmag > 0) & (np.abs(z) <= (x.shape[2] + 2) * 2.0 ** -23 * zmag)
    return ok, h1, pos1, z, zmag, amb


def forward(x, idx, weight, bias, weight2, bias2, center, lengths, dtype):
    """-> y, mag (N,L,K,C3), the valid mask (N,L,K) and amb (N,L,K,C2)."""
    ok, _, _, z, zmag, amb = _layers(x, idx, weight, bias, center, lengths, dtype)
    w2 = weight2.astype(np.float64)
    b2 = np.zeros(w2.shape[1]) if bias2 is None else bias2.astype(np.float64)
    return np.maximum(z, 0) @ w2 + b2, zmag @ np.abs(w2) + np.abs(b2), ok, amb


def backward(x, idx, weight, bias, weight2, center, lengths, g, out, arg, relu_out, dtype):
    """`out`, `arg`: the device's, so the selection is the same on both sides.
    -> {x, center, weight, bias, weight2, bias2: (grad, mag)}, s (N,M) entries per target row."""
    (N, M, C1), (_, L, K) = x.shape, idx.shape
    ok, h1, pos1, z, zmag, _ = _layers(x, idx, weight, bias, center, lengths, dtype)
    w, w2, pos2 = weight.astype(np.float64), weight2.astype(np.float64), z > 0
    gy = np.where((arg != 255) & ((out > 0) | (not relu_out)), g, 0).astype(np.float64)
    sel = ((arg[:, :, None, :] == np.arange(K)[None, None, :, None]) & ok[..., None]).astype(np.float64)  # (N,L,K,C3)
    res = []
    for gv, wv, w2v, h2 in ((gy, w, w2, np.maximum(z, 0)), (np.abs(gy), np.abs(w), np.abs(w2), np.where(pos2, zmag, 0))):
        e3 = sel * gv[:, :, None, :]
        e2 = np.where(pos2, e3 @ w2v.T, 0)
        e1 = np.where(pos1, e2 @ wv.T, 0)
        gx = np.zeros((N, M, C1))
        n, l, k = np.nonzero(ok)
        np.add.at(gx, (n, idx[n, l, k]), e1[n, l, k])
        res.append(dict(x=gx, center=e1.sum(2), weight=np.einsum("nlki,nlkc->ic", h1, e2), bias=e2.sum((0, 1, 2)),
                        weight2=np.einsum("nlkc,nlkd->cd", h2, e3), bias2=gv.sum((0, 1))))
    s = np.zeros((N, M), dtype=np.int64)
    np.add.at(s, (n, idx[n, l, k]), 1)
    return {name: (res[0][name], res[1][name]) for name in res[0]}, s
