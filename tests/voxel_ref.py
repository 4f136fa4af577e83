"""numpy checker of voxel_downsample: the definition in the comment block of pointops_voxel_downsample
(include/pointops_amd.h) restated step by step, independent of the package.  numpy's float64 subtraction, division and
floor are IEEE operations applied one at a time: "unfused and in the order written".

    downsample(points, lengths, v, features, origin) -> dict of the eight outputs, padded to P voxel rows; the means are
        float64: the EXACT sum of the members (math.fsum) divided by the count -- the definition allows any fixed
        summation order, so the checker pins the integers and bounds the means (mean_bound)
    exact_means(values, inverse, num_voxels) -> the same means from a given assignment (the device's own `inverse`)
    mean_bound(values, inverse, counts, m) -> 2^-24 |m| + n 2^-52 max_j |x_j| per voxel row and channel
"""
import math

import numpy as np

EXTENT = 2.0 ** 21
CELL = 2.0 ** 31


def live_rows(points, lengths):
    N, P = points.shape[:2]
    L = np.full(N, P, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, P)
    return (np.arange(P)[None, :] < L[:, None]) & np.isfinite(points).all(2)


def cloud_cells(pts, live, v, origin):
    """pts (P, 3) float32, live (P,) bool, origin (3,) float32 or None -> (status, cells (P, 3) int64 (0 on rows of no
    voxel), member (P,) bool)."""
    P = len(pts)
    none = (np.zeros((P, 3), np.int64), np.zeros(P, bool))
    if not live.any():
        return (0,) + none
    v64 = np.float64(np.float32(v))
    mn, mx = pts[live].min(0), pts[live].max(0)  # float32
    o = origin.astype(np.float64) if origin is not None else mn.astype(np.float64) - np.float64(0.5) * v64
    with np.errstate(all="ignore"):
        cell = lambda x: np.floor((x.astype(np.float64) - o) / v64)  # noqa: E731
        c_lo, c_hi = cell(mn), cell(mx)
        fits = (c_hi - c_lo < EXTENT) & (np.abs(c_lo) < CELL) & (np.abs(c_hi) < CELL)  # (a NaN does not fit)
        if not fits.all():
            return (1,) + none
        c = np.zeros((P, 3), np.int64)
        c[live] = cell(pts[live]).astype(np.int64)
    return 0, c, live.copy()


def downsample(points, lengths, v, features=None, origin=None):
    points = np.asarray(points, np.float32)
    N, P = points.shape[:2]
    C = 0 if features is None else features.shape[2]
    live = live_rows(points, lengths)
    out = dict(num_voxels=np.zeros(N, np.int64), status=np.zeros(N, np.int32), inverse=np.full((N, P), -1, np.int64),
               counts=np.zeros((N, P), np.int64), first_index=np.full((N, P), -1, np.int64),
               coords=np.zeros((N, P, 3), np.int64), centroids=np.zeros((N, P, 3), np.float64),
               pooled=None if features is None else np.zeros((N, P, C), np.float64))
    for n in range(N):
        o = None if origin is None else np.asarray(origin, np.float32).reshape(-1, 3)[n if np.ndim(origin) == 2 else 0]
        status, c, member = cloud_cells(points[n], live[n], v, o)
        out["status"][n] = status
        rows = np.flatnonzero(member)
        if not len(rows):
            continue
        order = rows[np.lexsort((rows, c[rows, 0], c[rows, 1], c[rows, 2]))]  # (z, y, x), then the row index
        cs = c[order]
        head = np.ones(len(order), bool)
        head[1:] = (cs[1:] != cs[:-1]).any(1)
        vid = np.cumsum(head) - 1
        V = int(vid[-1]) + 1
        out["num_voxels"][n] = V
        out["inverse"][n, order] = vid
        out["counts"][n, :V] = np.bincount(vid, minlength=V)
        out["first_index"][n, :V] = order[head]
        out["coords"][n, :V] = cs[head]
    out["centroids"] = exact_means(points, out["inverse"], out["num_voxels"])
    if features is not None:
        out["pooled"] = exact_means(np.asarray(features, np.float32), out["inverse"], out["num_voxels"])
    return out


def exact_means(values, inverse, num_voxels):
    """values (N, P, K) float32, inverse (N, P) -> (N, P, K) float64: fsum of every voxel's members / its count, 0 on the
    rows at or past num_voxels."""
    N, P, K = values.shape
    m = np.zeros((N, P, K), np.float64)
    for n in range(N):
        rows = np.flatnonzero(inverse[n] >= 0)
        if not len(rows):
            continue
        order = rows[np.argsort(inverse[n, rows], kind="stable")]
        vid = inverse[n, order]
        starts = np.flatnonzero(np.r_[True, vid[1:] != vid[:-1]])
        ends = np.r_[starts[1:], len(order)]
        x = values[n, order].astype(np.float64)
        assert len(starts) == int(num_voxels[n]) and np.array_equal(vid[starts], np.arange(len(starts)))
        single = ends - starts == 1
        m[n, vid[starts[single]]] = x[starts[single]]
        for a, b in zip(starts[~single], ends[~single]):
            for k in range(K):
                m[n, vid[a], k] = math.fsum(x[a:b, k]) / float(b - a)
    return m


def mean_bound(values, inverse, counts, m):
    """The bound on |out - m| per voxel row and channel: one rounding to float32 of the mean, 2^-24 |m|, plus twice the
    worst case of a float64 sum of n float32 terms in any order with the float64 division, n 2^-52 max_j |x_j|."""
    N, P, K = values.shape
    biggest = np.zeros((N, P, K), np.float64)
    for n in range(N):
        rows = np.flatnonzero(inverse[n] >= 0)
        np.maximum.at(biggest[n], inverse[n, rows], np.abs(values[n, rows].astype(np.float64)))
    return 2.0 ** -24 * np.abs(m) + counts[..., None].astype(np.float64) * 2.0 ** -52 * biggest


def blobs(seed, P, k=6, sigma=0.08):
    """P points in a few Gaussian blobs inside the unit cube (float32)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.2, 0.8, (k, 3))
    return (centres[rng.integers(0, k, P)] + rng.normal(0, sigma, (P, 3))).astype(np.float32)
