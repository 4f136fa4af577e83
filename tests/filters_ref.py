"""Checker for the outlier filters (functions/filters.py): the definitions in the comment block of
pointops_radius_outlier / pointops_statistical_outlier / pointops_mask_compact (include/pointops_amd.h) restated in numpy,
stage by stage and independent of the package.

    d2(i, j) = (dx*dx + dy*dy) + dz*dz in float32, unfused (numpy's float32 arithmetic is IEEE and unfused, as the build's
               -ffp-contract=off makes the kernels')
    radius       c_i = #{ j != i : d2 < fl32(r * r) };  mask = c_i >= min_neighbors
    knn          the K1 smallest d2 of a row, ties to the lower index (only the values are kept, and no tie changes those), the
                 row itself among them
    row mean     the float64 sum of sqrt((double)d2) in ascending k over cnt = min(K1, len) terms, / (cnt - 1), rounded once
    statistics   S1 and S2 by the documented tree, replayed literally (`tree_sum`): chunks of 4096 rows, 256 lanes adding
                 their 16 rows in order, the fold with strides 128 .. 1, the chunks in order
    compaction   the kept rows in ascending order, then -1

Floating-point results are compared bit for bit, never within a tolerance.
"""
import numpy as np

BLOCK = 1024  # rows of the P x P comparison formed at a time
LANES, ROWS_PER_LANE = 256, 16
CHUNK = LANES * ROWS_PER_LANE


def _lengths(lengths, N, P):
    return np.full(N, P, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, P)


def d2_rows(p, a, b):
    """(b - a, P) float32: d2(i, j) for rows a <= i < b of the (P, D) float32 points of one cloud."""
    p = np.ascontiguousarray(p, np.float32)
    q = p[a:b]
    with np.errstate(invalid="ignore", over="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        d = dx * dx
        for k in range(1, p.shape[1]):
            dk = q[:, None, k] - p[None, :, k]
            d = d + dk * dk
    return d


# ------------------------------------------------------------------------------------------------ compaction
def compact(mask):
    """(index (N, P) int64, num_kept (N,) int64) of a mask (N, P): anything not 0 is kept."""
    mask = np.asarray(mask) != 0
    N, P = mask.shape
    index = np.full((N, P), -1, np.int64)
    for n in range(N):
        rows = np.flatnonzero(mask[n])
        index[n, :len(rows)] = rows
    return index, mask.sum(1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ radius
def radius_counts(p, radius):
    """(P,) int32: the number of OTHER rows within the radius, for the (P, D) float32 points of one cloud."""
    P = p.shape[0]
    r2 = np.float32(radius) * np.float32(radius)
    c = np.zeros(P, np.int32)
    for a in range(0, P, BLOCK):
        hit = d2_rows(p, a, min(a + BLOCK, P)) < r2
        hit[np.arange(hit.shape[0]), np.arange(a, a + hit.shape[0])] = False
        c[a:a + BLOCK] = hit.sum(1)
    return c


def radius(points, lengths, radius_, min_neighbors):
    """dict(mask (N, P) bool, counts (N, P) int32, index (N, P) int64, num_kept (N,) int64) of a padded batch."""
    points = np.asarray(points, np.float32)
    N, P = points.shape[:2]
    L = _lengths(lengths, N, P)
    counts = np.zeros((N, P), np.int32)
    mask = np.zeros((N, P), bool)
    for n in range(N):
        counts[n, :L[n]] = radius_counts(points[n, :L[n]], radius_)
        mask[n, :L[n]] = counts[n, :L[n]] >= min_neighbors
    index, num = compact(mask)
    return dict(mask=mask, counts=counts, index=index, num_kept=num)


# ------------------------------------------------------------------------------------------------ statistical
def knn_d2(p, K1):
    """(P, K1) float32: the K1 smallest d2 of every row of one cloud, ascending, ties to the lower index; slots past
    the cloud's size hold 0 (knn_points' padding)."""
    P = p.shape[0]
    out = np.zeros((P, K1), np.float32)
    k = min(K1, P)
    for a in range(0, P, BLOCK):
        d = d2_rows(p, a, min(a + BLOCK, P))
        # (the VALUES of the k smallest under "ties to the lower index" are those of any selection of k smallest)
        out[a:a + BLOCK, :k] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
    return out


def knn_table(points, lengths, K1):
    """(N, P, K1) float32 of a padded batch: knn_d2 of every cloud, 0 on padding rows."""
    points = np.asarray(points, np.float32)
    N, P = points.shape[:2]
    L = _lengths(lengths, N, P)
    out = np.zeros((N, P, K1), np.float32)
    for n in range(N):
        out[n, :L[n]] = knn_d2(points[n, :L[n]], K1)
    return out


def row_means(d2, cnt):
    """(rows,) float32: step 1 for the (rows, K1) float32 table of rows below the length."""
    rows = d2.shape[0]
    if cnt < 2:
        return np.zeros(rows, np.float32)
    s = np.zeros(rows, np.float64)
    with np.errstate(invalid="ignore"):
        for k in range(cnt):
            s = s + np.sqrt(d2[:, k].astype(np.float64))
        return (s / np.float64(cnt - 1)).astype(np.float32)


def tree_sum(v):
    """The documented tree over the float64 terms v[0 .. P) of one cloud, replayed addition by addition (vectorised
    over the lanes, which never changes what is added to what)."""
    v = np.asarray(v, np.float64)
    total = np.float64(0.0)
    for c0 in range(0, len(v), CHUNK):
        chunk = np.zeros(CHUNK, np.float64)
        part = v[c0:c0 + CHUNK]
        chunk[:len(part)] = part
        rows = chunk.reshape(ROWS_PER_LANE, LANES)  # rows[j, t] = row c0 + t + 256 j
        s = np.zeros(LANES, np.float64)
        for j in range(ROWS_PER_LANE):
            s = s + rows[j]
        h = LANES // 2
        while h > 0:
            s[:h] = s[:h] + s[h:2 * h]
            h //= 2
        total = total + s[0]
    return total


def statistics(m, length, P):
    """(mean, std, n_f) in float64 of one cloud: m (P,) float32 row means, rows at or past `length` ignored."""
    live = np.arange(P) < length
    fin = live & np.isfinite(m)
    nf = int(fin.sum())
    m64 = m.astype(np.float64)
    S1 = tree_sum(np.where(fin, m64, 0.0))
    mean = S1 / np.float64(nf) if nf > 0 else np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        dev = np.where(fin, m64, mean) - mean
    S2 = tree_sum(np.where(fin, dev * dev, 0.0))
    std = np.sqrt(S2 / np.float64(nf - 1)) if nf >= 2 else np.float64(0.0)
    return mean, std, nf


def statistical_from_dists(dists, lengths, std_ratio):
    """Steps 1-4 from a (N, P, K1) float32 table of squared distances: dict(mean_distance (N, P) float32, stats (N, 3)
    float64, threshold (N,) float32, mask (N, P) bool, index, num_kept)."""
    dists = np.asarray(dists, np.float32)
    N, P, K1 = dists.shape
    L = _lengths(lengths, N, P)
    md = np.zeros((N, P), np.float32)
    stats = np.zeros((N, 3), np.float64)
    thr = np.zeros(N, np.float32)
    mask = np.zeros((N, P), bool)
    for n in range(N):
        ln = int(L[n])
        md[n, :ln] = row_means(dists[n, :ln], min(K1, ln))
        mean, std, nf = statistics(md[n], ln, P)
        stats[n] = (mean, std, nf)
        thr[n] = np.float32(mean + np.float64(np.float32(std_ratio)) * std)
        with np.errstate(invalid="ignore"):
            mask[n, :ln] = np.isfinite(md[n, :ln]) & (md[n, :ln] <= thr[n])
    index, num = compact(mask)
    return dict(mean_distance=md, stats=stats, threshold=thr, mask=mask, index=index, num_kept=num)


def statistical_float64(dists, lengths, std_ratio):
    """The same filter evaluated plainly in float64 -- np.mean, np.std(ddof=1), no float32 rounding of m_i, no
    prescribed order: (m (N, P) float64, threshold (N,) float64, mask (N, P) bool).  What the checker is held to."""
    dists = np.asarray(dists, np.float64)
    N, P, K1 = dists.shape
    L = _lengths(lengths, N, P)
    m = np.zeros((N, P))
    thr = np.zeros(N)
    mask = np.zeros((N, P), bool)
    for n in range(N):
        ln, cnt = int(L[n]), min(K1, int(L[n]))
        if cnt >= 2:
            m[n, :ln] = np.sqrt(dists[n, :ln, :cnt]).sum(1) / (cnt - 1)
        rows = m[n, :ln]
        mean = rows.mean() if ln > 0 else 0.0
        std = rows.std(ddof=1) if ln >= 2 else 0.0
        thr[n] = mean + float(np.float32(std_ratio)) * std
        mask[n, :ln] = rows <= thr[n]
    return m, thr, mask


# ------------------------------------------------------------------------------------------------ scenes
def uniform_scene(seed, P, D=3, neighbours=15.0, radius_=0.1):
    """(P, D) float32 uniform in a box sized so that a ball of `radius_` holds about `neighbours` other points."""
    rng = np.random.default_rng(seed)
    ball = {1: 2.0 * radius_, 2: np.pi * radius_ ** 2, 3: 4.0 / 3.0 * np.pi * radius_ ** 3}[D]
    side = (P * ball / neighbours) ** (1.0 / D)
    return rng.uniform(0.0, side, (P, D)).astype(np.float32)


def slab_scene(seed, P, D=3, radius_=0.1):
    """The uniform scene flattened along its last axis to a tenth of the radius: a dense sheet (line for D = 2)."""
    p = uniform_scene(seed, P, D, neighbours=15.0, radius_=radius_)
    if D > 1:
        p[:, -1] *= np.float32(0.1 * radius_ / max(float(p[:, -1].max()), 1e-9))
    return p


def outlier_scene(seed, P, D=3, radius_=0.1, far=1e3):
    """The uniform scene with row 7 moved `far` away along every axis: it stretches the bounding box a grid is sized
    from, has no neighbour and must go."""
    p = uniform_scene(seed, P, D, radius_=radius_)
    p[7] = np.float32(far)
    return p


def lattice_scene(side, D=3, step=0.125):
    """(side^D, D) float32: a periodic-looking cubic lattice with a power-of-two step (coordinates exact)."""
    axes = np.meshgrid(*([np.arange(side, dtype=np.float32) * np.float32(step)] * D), indexing="ij")
    return np.stack([a.ravel() for a in axes], axis=1)
