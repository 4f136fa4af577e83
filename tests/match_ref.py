"""numpy restatement of match_features (the FEATURE MATCHING block of include/pointops_amd.h) and of the screen of
csrc/feature_screen.h -- the checker of tests/test_match_cpu.py and tests/test_match_gpu.py.

    knn          squared L2 as the float32 sum in d order (`acc = acc + diff * diff`, every operation rounded to float32),
                 the K smallest (dist, idx) per row, ties to the lower index, 0 padding: pointops_knn_points_idx
    match        the three filters in float32 on top of it
    screen       n, g and s as fmaf chains (fma32 below is exact: float64 product, float64 sum, one repair where the
                 float64 sum sits on a float32 tie), the bound E, the per-lane lists of M keys and the certificate:
                 which rows the kernel must send to its exact fallback

Nothing here reads the library."""
import numpy as np

M = 8            # kScreenM
MAX_NORM = np.float32(2.0 ** 126)  # kScreenMaxNorm
F32 = np.float32


def fl32(x):
    return F32(x)


# ------------------------------------------------------------------------------------------------ the search
def pair_distances(a, b):
    """(P1, P2) float32: sum over d, in d order, of fl(fl(a - b)^2), accumulated in float32 from 0."""
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    with np.errstate(all="ignore"):
        for d in range(a.shape[1]):
            diff = a[:, d, None] - b[None, :, d]
            acc = acc + diff * diff
    assert acc.dtype == F32
    return acc


def knn(f1, f2, lengths1, lengths2, K):
    """(idx (N,P1,K) int64, dists (N,P1,K) float32) of finite inputs."""
    N, P1, _ = f1.shape
    idx = np.zeros((N, P1, K), np.int64)
    dists = np.zeros((N, P1, K), F32)
    for n in range(N):
        l1, l2 = int(min(max(lengths1[n], 0), P1)), int(min(max(lengths2[n], 0), f2.shape[1]))
        k = min(K, l2)
        if l1 == 0 or k == 0:
            continue
        d = pair_distances(f1[n, :l1], f2[n, :l2])
        order = np.argsort(d, axis=1, kind="stable")[:, :k]  # stable: equal distances keep index order
        idx[n, :l1, :k] = order
        dists[n, :l1, :k] = np.take_along_axis(d, order, axis=1)
    return idx, dists


def full_lengths(f, lengths):
    return np.full(f.shape[0], f.shape[1], np.int64) if lengths is None else np.asarray(lengths, np.int64)


def match_features(f1, f2, lengths1=None, lengths2=None, mutual=True, ratio=None, max_distance=None):
    """dict(corr, dists, second, num_matches) by the definition."""
    lengths1, lengths2 = full_lengths(f1, lengths1), full_lengths(f2, lengths2)
    N, P1, P2 = f1.shape[0], f1.shape[1], f2.shape[1]
    rows = np.arange(P1)[None, :]
    nearest = (rows < lengths1[:, None]) & (lengths2[:, None] >= 1) & (P2 >= 1)
    has_second = nearest & (lengths2[:, None] >= 2)
    if P1 == 0 or P2 == 0 or N == 0:
        z = np.zeros((N, P1), F32)
        return dict(corr=np.full((N, P1), -1, np.int64), dists=z, second=z.copy(), num_matches=np.zeros(N, np.int64))
    idx, d = knn(f1, f2, lengths1, lengths2, 2)
    j1, d1, d2 = idx[..., 0], d[..., 0], d[..., 1]
    keep = nearest.copy()
    if max_distance is not None:
        m = fl32(max_distance)
        keep &= d1 < fl32(m * m)
    if ratio is not None:
        rho = fl32(ratio)
        with np.errstate(all="ignore"):
            keep &= ~has_second | (d1 < fl32(rho * rho) * d2)
    if mutual:
        back = knn(f2, f1, lengths2, lengths1, 1)[0][..., 0]
        keep &= np.take_along_axis(back, j1, axis=1) == rows
    corr = np.where(keep, j1, -1).astype(np.int64)
    return dict(corr=corr, dists=np.where(nearest, d1, F32(0)).astype(F32),
                second=np.where(has_second, d2, np.where(nearest, F32(np.inf), F32(0))).astype(F32),
                num_matches=(corr >= 0).sum(1).astype(np.int64))


KEYS = ("corr", "dists", "second", "num_matches")


# ------------------------------------------------------------------------------------------------ the screen
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 arrays of normal magnitudes: the float64 product of two float32
    is exact; the float64 sum is rounded once, and rounding that to float32 is a second rounding only when the float64
    sum sits exactly on a float32 tie while the true sum does not -- then one float64 step towards the true sum repairs
    it (TwoSum gives the sign of what the float64 sum lost)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)
    tie = (t.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    fix = tie & (err != 0) & np.isfinite(t)
    if fix.any():
        t = np.where(fix, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
    return t.astype(F32)


def norms(f):
    """(..., P) float32: n = fma(a_k, a_k, n), k ascending from 0."""
    n = np.zeros(f.shape[:-1], F32)
    for k in range(f.shape[-1]):
        n = fma32(f[..., k], f[..., k], n)
    return n


def dots(a, b):
    """(P1, P2) float32: g = fma(a_k, b_k, g), k ascending from 0."""
    g = np.zeros((a.shape[0], b.shape[0]), F32)
    for k in range(a.shape[1]):
        g = fma32(np.broadcast_to(a[:, k, None], g.shape), np.broadcast_to(b[None, :, k], g.shape), g)
    return g


def screen_values(a, b):
    """s (P1,P2) = fl(fl(n1 + n2) - 2 g), n1, n2 of one cloud."""
    n1, n2 = norms(a), norms(b)
    g = dots(a, b)
    with np.errstate(all="ignore"):
        s = (n1[:, None] + n2[None, :]) - (g + g)
    assert s.dtype == F32
    return s, n1, n2


def screen_c(D):
    return 4 * D + 8


def screen_bound(D, n1, n2max):
    """E, rounded upwards (screen_bound of feature_screen.h): float64 expression, conversion, one step up if it fell."""
    c = float(screen_c(D))
    with np.errstate(all="ignore"):
        e = (c * 2.0 ** -24) * (np.asarray(n1, np.float64) + np.float64(n2max)) + c * 2.0 ** -149
        f = e.astype(F32)
        return np.where(f.astype(np.float64) < e, np.nextafter(f, F32(np.inf)), f).astype(F32)


def row_finite(D, n1, n2max):
    with np.errstate(all="ignore"):
        t = (np.asarray(n1, F32) + F32(n2max)).astype(F32)
        return (D <= 256) & (np.asarray(n1) >= 0) & (n2max >= 0) & (t <= MAX_NORM)


def uncertified_rows(f1, f2, lengths1=None, lengths2=None, K=2):
    """(N, P1) bool: the rows with a nearest that the kernel's certificate cannot cover.  A lane half h (bit 2 of the
    target index) keeps the M smallest (s, j) of its targets; the collected targets of a row are both lists; s_cut is
    the smaller of the two M-th keys (+inf for a list that never filled); the row is certified when the cloud has at
    most M targets or fl(r_K + E) < s_cut, and never when a norm is not finite or above 2^126."""
    lengths1, lengths2 = full_lengths(f1, lengths1), full_lengths(f2, lengths2)
    N, P1, D = f1.shape
    out = np.zeros((N, P1), bool)
    for n in range(N):
        l1, l2 = int(min(max(lengths1[n], 0), P1)), int(min(max(lengths2[n], 0), f2.shape[1]))
        if l1 == 0 or l2 == 0:
            continue
        n2 = norms(f2[n, :l2])
        n2max = n2.max() if np.isfinite(n2).all() else F32(np.nan)
        half = (np.arange(l2) >> 2) & 1
        for lo in range(0, l1, 128):  # (blocks of rows: the float64 temporaries stay in cache)
            a, b = f1[n, lo:min(lo + 128, l1)], f2[n, :l2]
            s, n1, _ = screen_values(a, b)
            fin = row_finite(D, n1, n2max)
            if l2 <= M:
                out[n, lo:lo + len(a)] = ~fin
                continue
            r = pair_distances(a, b)
            E = screen_bound(D, n1, n2max)
            collected = np.zeros(s.shape, bool)
            s_cut = np.full(len(a), np.inf, F32)
            for h in (0, 1):
                js = np.nonzero(half == h)[0]
                order = np.argsort(s[:, js], axis=1, kind="stable")[:, :M]
                np.put_along_axis(collected, js[order], True, axis=1)
                if len(js) >= M:
                    s_cut = np.minimum(s_cut, np.take_along_axis(s[:, js], order[:, M - 1:M], axis=1)[:, 0])
            rK = np.sort(np.where(collected, r, F32(np.inf)), axis=1)[:, K - 1]
            with np.errstate(all="ignore"):
                ok = fin & ((rK + E).astype(F32) < s_cut)
            out[n, lo:lo + len(a)] = ~ok
    return out
