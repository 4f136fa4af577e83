"""The checker of knn_in_radius: the KNN IN RADIUS block of include/pointops_amd.h restated in numpy, all pairs.

Everything is np.float32 and unfused, in the order of the header: d2 = ((dx*dx) + dy*dy) + dz*dz over the D coordinates,
r2 = fl32(radius * radius), a candidate iff d2 < r2 (a NaN d2 fails), the result the first min(K, #candidates) candidates
in ascending (d2, j) order -- so a tie goes to the lower index."""
import numpy as np

ROWS = 256  # query rows per block of the all-pairs table


def r2_of(radius):
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(radius) * np.float32(radius)


def dist2(p1, p2):
    """(P1, P2) float32 squared distances of two clouds (P, D), the header's expression."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        d = p1[:, None, :] - p2[None, :, :]
        acc = d[..., 0] * d[..., 0]
        for k in range(1, p1.shape[1]):
            acc = acc + d[..., k] * d[..., k]
    return acc.astype(np.float32, copy=False)


def knn_in_radius(p1, p2, lengths1, lengths2, K, radius):
    """-> dict(idx (N,P1,K) int64 padded -1, dists (N,P1,K) float32 padded 0, counts (N,P1) int32)"""
    p1, p2 = np.asarray(p1, np.float32), np.asarray(p2, np.float32)
    N, P1, _ = p1.shape
    P2 = p2.shape[1]
    l1 = np.full(N, P1) if lengths1 is None else np.clip(np.asarray(lengths1), 0, P1)
    l2 = np.full(N, P2) if lengths2 is None else np.clip(np.asarray(lengths2), 0, P2)
    r2 = r2_of(radius)
    idx = np.full((N, P1, K), -1, np.int64)
    dists = np.zeros((N, P1, K), np.float32)
    counts = np.zeros((N, P1), np.int32)
    for n in range(N):
        a, b = int(l1[n]), int(l2[n])
        for r0 in range(0, a if b else 0, ROWS):  # (row blocks: the pairs of a block fit in memory at any P2)
            r1 = min(r0 + ROWS, a)
            d2 = dist2(p1[n, r0:r1], p2[n, :b])
            with np.errstate(invalid="ignore"):
                rows, cols = np.nonzero(d2 < r2)
            vals = d2[rows, cols]
            order = np.lexsort((cols, vals, rows))  # per row: ascending d2, equal d2 in ascending j
            rows, cols, vals = rows[order], cols[order], vals[order]
            rank = np.arange(len(rows)) - np.searchsorted(rows, np.arange(r1 - r0))[rows]
            keep = rank < K
            idx[n, r0 + rows[keep], rank[keep]] = cols[keep]
            dists[n, r0 + rows[keep], rank[keep]] = vals[keep]
            counts[n, r0:r1] = np.minimum(np.bincount(rows, minlength=r1 - r0), K)
    return dict(idx=idx, dists=dists, counts=counts)


def mask_knn(knn_idx, knn_dists, lengths1, lengths2, radius):
    """The header's identity: the table of knn_points(K) -> the table of knn_in_radius, on finite inputs."""
    N, P1, K = knn_idx.shape
    with np.errstate(invalid="ignore"):
        keep = knn_dists < r2_of(radius)
    keep &= np.arange(K)[None, None, :] < np.asarray(lengths2)[:, None, None]
    keep &= np.arange(P1)[None, :, None] < np.asarray(lengths1)[:, None, None]
    return dict(idx=np.where(keep, knn_idx, -1).astype(np.int64),
                dists=np.where(keep, knn_dists, np.float32(0)).astype(np.float32),
                counts=keep.sum(2).astype(np.int32))
