"""Checker for iss_keypoints (functions/iss.py): the definition in the comment of pointops_iss_keypoints
(include/pointops_amd.h) restated in numpy, stage by stage, independent of the package.

    support     S_i = { j : d2(i, j) < fl32(rs * rs) },  d2 = (dx*dx + dy*dy) + dz*dz in float32, unfused
    moments     s = 2^(19 - e), e the smallest integer with fl32(rs) <= 2^e;  q = rint((x_j - x_i) * s) in float64, half
                to even;  n = |S_i|, M1 = sum q, M2 = sum q q^T (xx, xy, xz, yy, yz, zz) in int64
    covariance  m = M1 / n;  C = (M2 / n - m m^T) * s^-2 in float64;  n = 0: C = 0
    eigenvalues ascending, rounded to float32 (here numpy's eigvalsh; the device runs a cyclic Jacobi)
    decide      saliency = l0 when l0 > 2^-20 l2 and l1 < g21 l2 and l0 < g32 l1, in float32, else 0
    nms         T_i = { j : d2(i, j) < fl32(rn * rn) };  kept iff saliency_i > 0, |T_i| >= min_neighbors and no j in T_i
                has a larger saliency, or an equal one and a lower index

`iss_float64` is Open3D's compute_iss_keypoints restated on the same supports: the float64 covariance about the support
mean, unquantized, and the quotient tests.
"""
import math

import numpy as np

from cluster_ref import blobs_scene  # noqa: F401  (the scenes of the tests)

BLOCK = 256  # rows of the P x P comparison formed at a time
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def scale(rs):
    """s = 2^(19 - e), e the smallest integer with fl32(rs) <= 2^e."""
    m, k = math.frexp(float(np.float32(rs)))  # rs = m 2^k, 0.5 <= m < 1
    return math.ldexp(1.0, 19 - (k - 1 if m == 0.5 else k))


def within(q, p, radius):
    """(len(q), len(p)) bool: d2 < fl32(radius * radius) between the float32 rows q and all rows p."""
    r2 = np.float32(radius) * np.float32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        return ((dx * dx + dy * dy) + dz * dz) < r2


def moments_cloud(p, rs):
    """(P, 10) int64 of one cloud of (P, 3) float32 points: n, M1[3], M2[6]."""
    p = np.ascontiguousarray(p, np.float32)
    P = p.shape[0]
    s = scale(rs)
    out = np.zeros((P, 10), np.int64)
    p64 = p.astype(np.float64)
    for a in range(0, P, BLOCK):
        hit = within(p[a:a + BLOCK], p, rs)
        ii, jj = np.nonzero(hit)  # the hits only, row by row: the offsets of everything else are never formed
        q = np.rint((p64[jj] - p64[a + ii]) * s).astype(np.int64)
        terms = np.concatenate([q] + [(q[:, u] * q[:, v])[:, None] for u, v in PAIRS], axis=1)
        # row sums as differences of a running sum (int64 wraps around and back: exact whenever the row sums fit)
        run = np.concatenate([np.zeros((1, 9), np.int64), np.cumsum(terms, axis=0)])
        n = hit.sum(1)
        end = np.cumsum(n)
        out[a:a + BLOCK, 0] = n
        out[a:a + BLOCK, 1:] = run[end] - run[end - n]
    return out


def _per_cloud(points, lengths):
    points = np.asarray(points, np.float32)
    N, P = points.shape[:2]
    lengths = np.full(N, P, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, P)
    return points, [int(x) for x in lengths]


def moments(points, lengths, rs):
    """(N, P, 10) int64 of a padded batch; zero on padding rows."""
    points, lengths = _per_cloud(points, lengths)
    out = np.zeros(points.shape[:2] + (10,), np.int64)
    for n, L in enumerate(lengths):
        out[n, :L] = moments_cloud(points[n, :L], rs)
    return out


def covariance(mom, rs):
    """(..., 3, 3) float64 from (..., 10) int64 moments, in the order the definition writes."""
    mom = np.asarray(mom, np.int64)
    s = scale(rs)
    inv2 = (1.0 / s) * (1.0 / s)
    n = mom[..., 0].astype(np.float64)
    safe = np.where(n > 0, n, 1.0)
    m = mom[..., 1:4].astype(np.float64) / safe[..., None]
    C = np.zeros(mom.shape[:-1] + (3, 3))
    for k, (u, v) in enumerate(PAIRS):
        c = (mom[..., 4 + k].astype(np.float64) / safe - m[..., u] * m[..., v]) * inv2
        C[..., u, v] = C[..., v, u] = np.where(n > 0, c, 0.0)
    return C


def eigenvalues64(C):
    return np.linalg.eigvalsh(C)  # ascending


def decide(eig, g21, g32):
    """(...,) float32 saliency from (..., 3) float32 ascending eigenvalues."""
    eig = np.asarray(eig, np.float32)
    l0, l1, l2 = eig[..., 0], eig[..., 1], eig[..., 2]
    ok = (l0 > np.float32(2.0 ** -20) * l2) & (l1 < np.float32(g21) * l2) & (l0 < np.float32(g32) * l1)
    return np.where(ok, l0, np.float32(0.0)).astype(np.float32)


def nms_cloud(sal, p, rn, min_neighbors):
    p = np.ascontiguousarray(p, np.float32)
    P = p.shape[0]
    keep = np.zeros(P, bool)
    idx = np.arange(P)
    for a in range(0, P, BLOCK):
        hit = within(p[a:a + BLOCK], p, rn)
        si, ii = sal[a:a + BLOCK, None], idx[a:a + BLOCK, None]
        beats = (sal[None, :] > si) | ((sal[None, :] == si) & (idx[None, :] < ii))
        keep[a:a + BLOCK] = (sal[a:a + BLOCK] > 0) & (hit.sum(1) >= min_neighbors) & ~(hit & beats).any(1)
    return keep


def nms(saliency, points, lengths, rn, min_neighbors):
    """(N, P) bool from the (N, P) float32 saliency of a padded batch; False on padding rows."""
    points, lengths = _per_cloud(points, lengths)
    saliency = np.asarray(saliency, np.float32)
    out = np.zeros(points.shape[:2], bool)
    for n, L in enumerate(lengths):
        out[n, :L] = nms_cloud(saliency[n, :L], points[n, :L], rn, min_neighbors)
    return out


def iss(points, lengths, rs, rn, g21=0.975, g32=0.975, min_neighbors=5):
    """The stages chained -> dict(moments, C, eigenvalues float32, saliency, mask, num_keypoints)."""
    points, L = _per_cloud(points, lengths)
    mom = moments(points, lengths, rs)
    C = covariance(mom, rs)
    eig = eigenvalues64(C).astype(np.float32)
    live = np.arange(points.shape[1])[None, :] < np.asarray(L)[:, None]
    eig = np.where(live[..., None], eig, np.float32(0.0))
    sal = np.where(live, decide(eig, g21, g32), np.float32(0.0))
    mask = nms(sal, points, lengths, rn, min_neighbors)
    return dict(moments=mom, C=C, eigenvalues=eig, saliency=sal, mask=mask, num_keypoints=mask.sum(1).astype(np.int64))


def iss_float64(p, rs, rn, g21=0.975, g32=0.975, min_neighbors=5):
    """Open3D's algorithm on one cloud (P, 3) float32, over the same supports: the float64 covariance about the support
    mean, the quotient tests, the same suppression -> (eigenvalues (P, 3) float64 ascending, saliency float64, mask)."""
    p = np.ascontiguousarray(p, np.float32)
    P = p.shape[0]
    p64 = p.astype(np.float64)
    eig = np.zeros((P, 3))
    for a in range(0, P, BLOCK):
        hit = within(p[a:a + BLOCK], p, rs).astype(np.float64)
        n = np.maximum(hit.sum(1), 1.0)
        mean = hit @ p64 / n[:, None]
        d = (p64[None, :, :] - mean[:, None, :]) * hit[:, :, None]
        eig[a:a + BLOCK] = np.linalg.eigvalsh(np.einsum("ijk,ijl->ikl", d, d) / n[:, None, None])
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (eig[:, 1] / eig[:, 2] < g21) & (eig[:, 0] / eig[:, 1] < g32) & (eig[:, 0] > 0)
    sal = np.where(ok, eig[:, 0], 0.0)
    return eig, sal, nms_cloud(sal, p, rn, min_neighbors)


# ------------------------------------------------------------------------------------------------ hand-made scenes
def tilted_plane(P=400, seed=5):
    """P points of the plane through (0.3, 0.2, 0.1) spanned by two tilted unit vectors, within a 0.4 square."""
    rng = np.random.default_rng(seed)
    u = np.array([1.0, 0.5, 0.25]) / np.linalg.norm([1.0, 0.5, 0.25])
    w = np.cross(u, [0.0, 0.0, 1.0])
    w /= np.linalg.norm(w)
    ab = rng.uniform(-0.2, 0.2, (P, 2))
    return (np.array([0.3, 0.2, 0.1]) + ab[:, :1] * u + ab[:, 1:] * w).astype(np.float32)


def cube_corner(m=7, h=(0.1, 0.09, 0.08)):
    """The three faces of a box that meet at the origin, m x m points each, at spacings h along x, y, z (unequal, so
    the corner's eigenvalues are apart; row 0 is the corner).  With rs = 0.13, rn = 0.11 the corner is THE keypoint."""
    gx, gy, gz = [np.arange(m) * x for x in h]
    faces = []
    for (u, v), put in (((gx, gy), lambda a, b, z: (a, b, z)), ((gx, gz), lambda a, b, z: (a, z, b)),
                        ((gy, gz), lambda a, b, z: (z, a, b))):
        a, b = [x.ravel() for x in np.meshgrid(u, v, indexing="ij")]
        faces.append(np.stack(put(a, b, np.zeros_like(a)), 1))
    return np.unique(np.concatenate(faces), axis=0).astype(np.float32)  # (lexicographic: the corner comes first)


def doubled(p):
    """Every point twice: rows P..2P-1 repeat rows 0..P-1."""
    return np.concatenate([p, p]).astype(np.float32)
