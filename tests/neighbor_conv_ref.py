"""Plain numpy float64 evaluation of the NEIGHBOUR CONVOLUTION block of include/pointops_amd.h: loops over rows and slots,
nothing else.  Every result comes with `mag`, the same expression on absolute values, which the error bounds are stated in."""
import numpy as np

from neighbor_reduce_ref import valid_slots


def _coefficients(coeff, n, l, k, P):
    return coeff[n, l, k].astype(np.float64) if coeff is not None else np.eye(P)[k]


def forward(x, idx, weight, lengths, coeff):
    """-> out, mag (N,L,Cout), A, Aabs (N,L,P,Cin), n (N,L) valid slots."""
    x, weight = x.astype(np.float64), weight.astype(np.float64)
    (N, M, Cin), (_, L, K), (P, _, Cout) = x.shape, idx.shape, weight.shape
    ok = valid_slots(idx, lengths, M)
    A, Aabs = np.zeros((N, L, P, Cin)), np.zeros((N, L, P, Cin))
    out, mag = np.zeros((N, L, Cout)), np.zeros((N, L, Cout))
    for n in range(N):
        for l in range(L):
            for k in range(K):
                if ok[n, l, k]:
                    t = np.outer(_coefficients(coeff, n, l, k, P), x[n, idx[n, l, k]])
                    A[n, l] += t
                    Aabs[n, l] += np.abs(t)
            out[n, l] = np.einsum("pc,pco->o", A[n, l], weight)
            mag[n, l] = np.einsum("pc,pco->o", Aabs[n, l], np.abs(weight))
    return dict(out=out, mag=mag, A=A, Aabs=Aabs, n=ok.sum(2))


def backward(x, idx, weight, lengths, coeff, g, fwd):
    """-> {x, weight, coeff: (grad, mag)}, seg (N,M) entries per target row; `fwd`: forward's."""
    x, weight, g = x.astype(np.float64), weight.astype(np.float64), g.astype(np.float64)
    (N, M, Cin), (_, L, K), (P, _, Cout) = x.shape, idx.shape, weight.shape
    ok = valid_slots(idx, lengths, M)
    gx, gw, gc = (np.zeros((2, *s)) for s in (x.shape, weight.shape, (N, L, K, P)))
    seg = np.zeros((N, M), dtype=np.int64)
    for n in range(N):
        for l in range(L):
            T = np.einsum("o,pco->pc", g[n, l], weight)
            Tabs = np.einsum("o,pco->pc", np.abs(g[n, l]), np.abs(weight))
            gw[0] += fwd["A"][n, l][:, :, None] * g[n, l]
            gw[1] += fwd["Aabs"][n, l][:, :, None] * np.abs(g[n, l])
            for k in range(K):
                if ok[n, l, k]:
                    m, cf = idx[n, l, k], _coefficients(coeff, n, l, k, P)
                    seg[n, m] += 1
                    gx[0, n, m] += cf @ T
                    gx[1, n, m] += np.abs(cf) @ Tabs
                    gc[0, n, l, k] = T @ x[n, m]
                    gc[1, n, l, k] = Tabs @ np.abs(x[n, m])
    return dict(x=gx, weight=gw, coeff=gc), seg
