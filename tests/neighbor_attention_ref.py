"""Plain numpy float64 evaluation of the NEIGHBOUR ATTENTION block of include/pointops_amd.h: loops over rows, heads and
slots, nothing else.  `forward` also returns the magnitudes the error bounds are stated in."""
import numpy as np

from neighbor_reduce_ref import valid_slots


def forward(q, k, v, idx, lengths, bias, heads, scale):
    """-> out, lse (N,L,H), mag = sum_k w_k |v_kc|; per (row, slot, head): w, counted, A = |scale| sum |q k| + |bias|, shift = s - m."""
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    N, L, C = q.shape
    M, K, D = k.shape[1], idx.shape[2], C // heads
    ok = valid_slots(idx, lengths, M)
    r = dict(out=np.zeros((N, L, C)), mag=np.zeros((N, L, C)), lse=np.full((N, L, heads), -np.inf),
             w=np.zeros((N, L, K, heads)), A=np.zeros((N, L, K, heads)), shift=np.zeros((N, L, K, heads)),
             counted=np.zeros((N, L, K, heads), dtype=bool))
    for n in range(N):
        for l in range(L):
            for h in range(heads):
                c = slice(h * D, h * D + D)
                s = np.full(K, -np.inf)
                for j in range(K):
                    if ok[n, l, j]:
                        b = float(bias[n, l, j, h]) if bias is not None else 0.0
                        s[j] = scale * np.sum(q[n, l, c] * k[n, idx[n, l, j], c]) + b
                        r["A"][n, l, j, h] = abs(scale) * np.sum(np.abs(q[n, l, c] * k[n, idx[n, l, j], c])) + \
                            (abs(b) if np.isfinite(b) else 0.0)
                cnt = s > -np.inf
                if not cnt.any():
                    continue
                m = s[cnt].max()
                e = np.where(cnt, np.exp(np.where(cnt, s, m) - m), 0.0)
                w = e / e.sum()
                r["counted"][n, l, :, h], r["w"][n, l, :, h], r["lse"][n, l, h] = cnt, w, m + np.log(e.sum())
                r["shift"][n, l, :, h] = np.where(cnt, np.where(cnt, s, m) - m, 0.0)
                for j in np.nonzero(cnt)[0]:
                    r["out"][n, l, c] += w[j] * v[n, idx[n, l, j], c]
                    r["mag"][n, l, c] += w[j] * np.abs(v[n, idx[n, l, j], c])
    return r


def backward(q, k, v, idx, lengths, heads, scale, g, fwd):
    """-> grad_q (N,L,C), grad_k, grad_v (N,M,C), grad_bias (N,L,K,H), seg (N,M) entries per target row; `fwd`: forward's."""
    q, k, v, g = (a.astype(np.float64) for a in (q, k, v, g))
    N, L, C = q.shape
    M, K, D = k.shape[1], idx.shape[2], C // heads
    ok = valid_slots(idx, lengths, M)
    gq, gk, gv = np.zeros((N, L, C)), np.zeros((N, M, C)), np.zeros((N, M, C))
    gb, seg = np.zeros((N, L, K, heads)), np.zeros((N, M), dtype=np.int64)
    for n in range(N):
        for l in range(L):
            for j in range(K):
                if not ok[n, l, j]:
                    continue
                m = idx[n, l, j]
                seg[n, m] += 1
                for h in range(heads):
                    c = slice(h * D, h * D + D)
                    w = fwd["w"][n, l, j, h]
                    ds = w * (np.sum(g[n, l, c] * v[n, m, c]) - np.sum(g[n, l, c] * fwd["out"][n, l, c]))
                    gb[n, l, j, h] = ds
                    gq[n, l, c] += scale * ds * k[n, m, c]
                    gk[n, m, c] += scale * ds * q[n, l, c]
                    gv[n, m, c] += w * g[n, l, c]
    return gq, gk, gv, gb, seg
