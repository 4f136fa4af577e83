"""Numpy checker of the FPFH definition (include/pointops_amd.h, pointops_spfh / pointops_fpfh), parametrised by the
dtype it computes in -- float32 follows the definition operation by operation, float64 is the yardstick -- and the
inputs the CPU and GPU suites share.  Vectorised over clouds, points and slots; no device code."""
import numpy as np

from pytorch3d_pointops_amd import synth

BINS, GROUP = 33, 11
EPS = 2.0 ** -24
T_PAIR = 32 * EPS          # pair features: f3; f2 and f1 divided by their conditioning terms
T_DIST = 4 * EPS           # d, relative
T_FPFH = 16 * 200 * EPS    # FPFH values lie in [0, 200]
KS = (1, 2, 8, 16, 50, 255)
CLOUDS = ("uniform", "sphere", "heightfield")


# ------------------------------------------------------------------------------------------------ the definition
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _lengths(lengths, N, P):
    return np.full((N,), P, np.int64) if lengths is None else np.asarray(lengths, np.int64)


def pair_features(points, normals, idx, lengths=None, dtype=np.float64):
    """dict of (N,P,K) arrays: `f` (N,P,K,4) = (f1, f2, f3, d), zero where not `counted`; `live`, `counted`; `d2`; the
    conditioning terms `s` = |dp x ns| / d and `c` = hypot(w.nt, ns.nt); `a1`, `a2` (the swap is |a1| < |a2|)."""
    pts, nrm = np.asarray(points).astype(dtype), np.asarray(normals).astype(dtype)
    idx = np.asarray(idx)
    N, P, K = idx.shape
    len_ = _lengths(lengths, N, P)[:, None, None]
    rows = np.arange(P)[None, :, None]
    ok = (rows < len_) & (idx >= 0) & (idx < len_) & (idx != rows)
    j = np.where(ok, idx, 0)
    n_ = np.arange(N)[:, None, None]
    pj, nj = pts[n_, j], nrm[n_, j]
    ni = np.broadcast_to(nrm[:, :, None, :], nj.shape)
    dp = pj - pts[:, :, None, :]
    d2 = _dot(dp, dp)
    live = ok & (d2 > 0)
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
        a1, a2 = _dot(ni, dp) / d, _dot(nj, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        sw = swap[..., None]
        ns, nt, dps = np.where(sw, nj, ni), np.where(sw, ni, nj), np.where(sw, -dp, dp)
        f3 = np.where(swap, -a2, a1)
        v = _cross(dps, ns)
        vn = np.sqrt(_dot(v, v))
        counted = live & (vn > 0)
        v = v / vn[..., None]
        w = _cross(ns, v)
        f2 = _dot(v, nt)
        y, x = _dot(w, nt), _dot(ns, nt)
        f1 = np.arctan2(y, x)
        f = np.where(counted[..., None], np.stack([f1, f2, f3, d], -1), 0).astype(dtype)
        s, c = vn / d, np.hypot(y, x)
    return dict(f=f, live=live, counted=counted, d2=np.where(live, d2, 0), s=s, c=c, a1=a1, a2=a2)


def bins(f, dtype=np.float32):
    """(…,3) integer bins of features (…, >= 3): the definition's operations in `dtype`, clamped like fmaxf / fminf (a
    NaN lands in bin 0)."""
    f = np.asarray(f).astype(dtype)
    one, lo, hi = dtype(1.0), dtype(0.0), dtype(10.0)
    pi, c1, c2 = dtype(np.pi), dtype(11.0 / (2.0 * np.pi)), dtype(5.5)
    with np.errstate(all="ignore"):
        raw = np.stack([np.floor((f[..., 0] + pi) * c1), np.floor((f[..., 1] + one) * c2),
                        np.floor((f[..., 2] + one) * c2)], -1)
    return np.fmin(np.fmax(raw, lo), hi).astype(np.int64)


def spfh_from_bins(b, counted, dtype=np.float32):
    """(N,P,33) from bins (N,P,K,3) and the counted mask (N,P,K)."""
    hot = (b[..., None] == np.arange(GROUP)) & counted[..., None, None]      # (N,P,K,3,11)
    counts = hot.sum(2).reshape(*counted.shape[:2], BINS)
    m = counted.sum(2)
    with np.errstate(all="ignore"):
        scale = np.where(m > 0, dtype(100.0) / m.astype(dtype), dtype(0.0)).astype(dtype)
    return (counts.astype(dtype) * scale[..., None]).astype(dtype)


def fpfh_from_spfh(spfh, idx, live, d2, dtype=np.float64):
    """(N,P,33): the weighted sum in k order, the three group sums in bin order."""
    sp = np.asarray(spfh).astype(dtype)
    N, P, K = idx.shape
    n_ = np.arange(N)[:, None]
    acc = np.zeros((N, P, BINS), dtype)
    with np.errstate(all="ignore"):
        for k in range(K):
            lk = live[:, :, k]
            term = sp[n_, np.where(lk, idx[:, :, k], 0)] / np.where(lk, d2[:, :, k], 1).astype(dtype)[..., None]
            acc = np.where(lk[..., None], acc + term, acc)
        out = np.zeros_like(acc)
        for c in range(3):
            g = acc[..., GROUP * c:GROUP * (c + 1)]
            S = np.zeros((N, P), dtype)
            for q in range(GROUP):
                S = S + g[..., q]
            out[..., GROUP * c:GROUP * (c + 1)] = np.where(S[..., None] > 0, g * dtype(100.0) / S[..., None], 0)
    return (out + sp).astype(dtype)


def fpfh(points, normals, idx, lengths=None, dtype=np.float64):
    """(fpfh, spfh, pair-feature dict), all in `dtype`."""
    pf = pair_features(points, normals, idx, lengths, dtype)
    sp = spfh_from_bins(bins(pf["f"], dtype), pf["counted"], dtype)
    return fpfh_from_spfh(sp, np.asarray(idx), pf["live"], pf["d2"], dtype), sp, pf


def wrap(a):
    """An angle difference folded into [-pi, pi]."""
    return (a + np.pi) % (2 * np.pi) - np.pi


def pair_feature_report(got, ref):
    """`got` (N,P,K,4) against the float64 `ref` of pair_features: per kept slot the errors over their bounds.
    -> dict(kept mask, excluded fraction of the live slots, max ratio per feature (f1, f2, f3, d))."""
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        kept = ref["live"] & (ref["s"] >= 1e-2) & (ref["c"] >= 1e-2) \
            & (np.abs(np.abs(ref["a1"]) - np.abs(ref["a2"])) >= 1e-5)
        err = np.abs(got - ref["f"])
        err[..., 0] = np.abs(wrap(got[..., 0] - ref["f"][..., 0]))
        bound = np.stack([T_PAIR / (ref["s"] * ref["c"]), T_PAIR / ref["s"], np.full_like(ref["s"], T_PAIR),
                          T_DIST * ref["f"][..., 3]], -1)
        ratio = np.where(kept[..., None], err / bound, 0)
    live = max(int(ref["live"].sum()), 1)
    return dict(kept=kept, excluded=float((ref["live"] & ~kept).sum()) / live,
                ratio=[float(ratio[..., e].max()) if ratio.size else 0.0 for e in range(4)])


# ------------------------------------------------------------------------------------------------ the inputs
def lengths_for(P, K):
    return np.array([P, P - 137, K + 1], np.int64)


def shape_for(K):
    """(N, P) of the case: P = 300 for K = 8 and for K = 255."""
    return 3, (300 if K in (8, 255) else 700)


def cloud(name, N, P, seed=0):
    """(points, normals) (N,P,3) fp32: `uniform` points with seeded random unit normals; a unit `sphere` with 2 % radial
    noise and normals = radial direction + 0.15 Gaussian, renormalised; the `heightfield` z = 0.3 sin 3x cos 2y over
    [-1,1]^2 with its analytic normals + 0.05 Gaussian."""
    rng = np.random.default_rng(7000 + seed)
    if name == "uniform":
        pts = np.stack([synth.distribution("uniform", 7100 + seed + n, P) for n in range(N)])
        return pts, synth.unit_normals(7200 + seed, (N, P, 3))
    if name == "sphere":
        u = rng.standard_normal((N, P, 3))
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        pts = u * (1.0 + 0.02 * rng.standard_normal((N, P, 1)))
        nrm = u + 0.15 * rng.standard_normal((N, P, 3))
        return pts.astype(np.float32), (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    if name == "heightfield":
        x, y = rng.uniform(-1, 1, (N, P)), rng.uniform(-1, 1, (N, P))
        pts = np.stack([x, y, 0.3 * np.sin(3 * x) * np.cos(2 * y)], -1)
        nrm = np.stack([-0.9 * np.cos(3 * x) * np.cos(2 * y), 0.6 * np.sin(3 * x) * np.sin(2 * y), np.ones_like(x)], -1)
        nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True) + 0.05 * rng.standard_normal((N, P, 3))
        return pts.astype(np.float32), nrm.astype(np.float32)
    raise ValueError(name)


def knn_self(points, lengths, K):
    """(N,P,K) int64 table of each cloud against itself in float64, laid out like knn_points: ascending (distance,
    index), 0 for rows past the length and for slots past it."""
    pts = np.asarray(points, np.float64)
    N, P, _ = pts.shape
    idx = np.zeros((N, P, K), np.int64)
    for n in range(N):
        L = int(lengths[n])
        d = ((pts[n, :L, None, :] - pts[n, None, :L, :]) ** 2).sum(-1)
        order = np.argsort(d, axis=1, kind="stable")[:, :K]
        idx[n, :L, :order.shape[1]] = order
    return idx


_MOTION = None


def rigid_motion():
    """A fixed rotation (3,3) and translation (3,) in float64."""
    global _MOTION
    if _MOTION is None:
        q, _ = np.linalg.qr(np.random.default_rng(7300).standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        _MOTION = (q, np.array([0.3, -0.2, 0.5]))
    return _MOTION


def moved(points, normals):
    """The cloud under rigid_motion(), computed in float64 and rounded to fp32."""
    R, t = rigid_motion()
    return ((np.asarray(points, np.float64) @ R.T) + t).astype(np.float32), \
        (np.asarray(normals, np.float64) @ R.T).astype(np.float32)
