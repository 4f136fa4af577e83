"""Checker for smooth_mls (functions/mls.py): the definition in the comment of pointops_mls_smooth
(include/pointops_amd.h) restated in numpy, stage by stage, independent of the package.

    support     S_i = { j : d2(i, j) < fl32(r * r) },  d2 = (dx*dx + dy*dy) + dz*dz in float32, unfused;  n_i = |S_i|
    weight      t = d2 / r2, u = 1 - t, w = u * u, w = w * w in float32;  wq = rint(float64(w) * 2^12), half to even
    moments     s = 2^(15 - e), e the smallest integer with fl32(r) <= 2^e;  q = rint((x_j - x_i) * s) in float64;
                W = sum wq, M1 = sum wq q, M2 = sum wq q q^T (xx, xy, xz, yy, yz, zz) in int64
    fit         m = M1 / W, delta = m / s, C = (M2 / W - m m^T) * s^-2 in float64;  W = 0: C = 0, delta = 0;
                l0 <= l1 <= l2 and n, the eigenvector of l0 (here numpy's eigh; the device runs a cyclic Jacobi), its sign
                such that the component of largest magnitude is positive, ties to the lower axis
    status      1 when n_i < min_neighbors, else 2 when l1 <= 2^-20 l2, else 0;  rows of status 1, 2: the point unchanged,
                normal 0, curvature 0
    output      normals = n^ = fl32(n);  h = (delta_x n^_x + delta_y n^_y) + delta_z n^_z in float64;
                points = fl32(float64(x) + h n^): the point moves along the returned normal;
                curvature = fl32(l0 / ((l0 + l1) + l2))
    iterations  the map applied k times; normals, curvature, n_i, status of the last pass

`mls_float64` is the same plane fit without any quantization: float64 weights (1 - d^2 / r^2)^4 from float64 distances,
float64 weighted mean and covariance, over the same supports.  A row is WELL CONDITIONED when l1 - l0 >= 0.05 l2 (the
normal is then stable against the perturbation the quantization is).  On the well-conditioned rows of the two scenes
below the points of `smooth` and of `mls_float64` differ by at most MEASURED_UNITS quanta of 2^-15 * 2^e (measured on
the noisy sphere at seed 1: 4.54 quanta; the noisy plane at seed 2: 0.43); the 12 bits of the weight dominate -- one
quantum of the offsets alone would give about 1/2.  tests/test_mls_cpu.py asserts twice that on further seeds.
"""
import math

import numpy as np

BLOCK = 256  # rows of the P x P comparison formed at a time
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
BITS, WEIGHT_BITS = 15, 12
MEASURED_UNITS = 4.54  # max |smooth - mls_float64| over the well-conditioned rows, in quanta (see above)


def exponent(r):
    """e, the smallest integer with fl32(r) <= 2^e."""
    m, k = math.frexp(float(np.float32(r)))  # r = m 2^k, 0.5 <= m < 1
    return k - 1 if m == 0.5 else k


def scale(r):
    return math.ldexp(1.0, BITS - exponent(r))


def quantum(r):
    """2^-15 * 2^e: the unit of the quantized offsets."""
    return 1.0 / scale(r)


def dist2(q, p):
    """(len(q), len(p)) float32: ball query's squared distance between the float32 rows q and all rows p."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def weight(d2, r2):
    """int64 wq of float32 d2 (any shape) and the float32 scalar r2; meaningful where d2 < r2."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = d2.astype(np.float32) / np.float32(r2)
        u = np.float32(1.0) - t
        w = u * u
        w = w * w
        wq = np.rint(w.astype(np.float64) * float(1 << WEIGHT_BITS))
    return np.where((wq >= 0) & (wq <= float(1 << WEIGHT_BITS)), wq, 0.0).astype(np.int64)  # (NaN, inf: no hit)


def moments_cloud(p, r):
    """((P, 10) int64: W, M1[3], M2[6];  (P,) int64 support sizes) of one cloud of (P, 3) float32 points."""
    p = np.ascontiguousarray(p, np.float32)
    P = p.shape[0]
    s = scale(r)
    r2 = np.float32(r) * np.float32(r)
    out, nn = np.zeros((P, 10), np.int64), np.zeros(P, np.int64)
    p64 = p.astype(np.float64)
    for a in range(0, P, BLOCK):
        d2 = dist2(p[a:a + BLOCK], p)
        hit = d2 < r2
        wq = np.where(hit, weight(d2, r2), 0)
        with np.errstate(invalid="ignore", over="ignore"):
            off = np.rint((p64[None, :, :] - p64[a:a + BLOCK, None, :]) * s)
        q = np.where(hit[..., None], off, 0.0).astype(np.int64)
        nn[a:a + BLOCK] = hit.sum(1)
        out[a:a + BLOCK, 0] = wq.sum(1)
        wqq = wq[..., None] * q
        out[a:a + BLOCK, 1:4] = wqq.sum(1)
        for k, (u, v) in enumerate(PAIRS):
            out[a:a + BLOCK, 4 + k] = (wqq[..., u] * q[..., v]).sum(1)
    return out, nn


def fit(mom, r):
    """From (..., 10) int64 moments: dict(delta (..., 3), C (..., 3, 3), eig (..., 3) ascending, n (..., 3) sign-fixed)
    in float64, in the order the definition writes."""
    mom = np.asarray(mom, np.int64)
    s = scale(r)
    inv2 = (1.0 / s) * (1.0 / s)
    W = mom[..., 0].astype(np.float64)
    safe = np.where(W > 0, W, 1.0)
    m = mom[..., 1:4].astype(np.float64) / safe[..., None]
    delta = np.where(W[..., None] > 0, m / s, 0.0)
    C = np.zeros(mom.shape[:-1] + (3, 3))
    for k, (u, v) in enumerate(PAIRS):
        c = (mom[..., 4 + k].astype(np.float64) / safe - m[..., u] * m[..., v]) * inv2
        C[..., u, v] = C[..., v, u] = np.where(W > 0, c, 0.0)
    eig, vec = np.linalg.eigh(C)
    return dict(delta=delta, C=C, eig=eig, n=fix_sign(vec[..., :, 0]))


def fix_sign(n):
    """The component of largest magnitude positive, ties to the lower axis (argmax takes the first maximum)."""
    big = np.argmax(np.abs(n), axis=-1)
    lead = np.take_along_axis(n, big[..., None], axis=-1)
    return np.where(lead < 0, -n, n)


def status_of(nn, eig, min_neighbors):
    st = np.where(eig[..., 1] <= 2.0 ** -20 * eig[..., 2], 2, 0)
    return np.where(nn < min_neighbors, 1, st).astype(np.uint8)


def well_conditioned(eig):
    return eig[..., 1] - eig[..., 0] >= 0.05 * eig[..., 2]


def project(x, delta, n, eig, status):
    """(points float32, normals float32, curvature float32) of float32 points x from the float64 fit."""
    n = n.astype(np.float32).astype(np.float64)  # n^: the returned normal
    h = (delta[..., 0] * n[..., 0] + delta[..., 1] * n[..., 1]) + delta[..., 2] * n[..., 2]
    ok = status == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        moved = (x.astype(np.float64) + h[..., None] * n).astype(np.float32)
        curv = (eig[..., 0] / ((eig[..., 0] + eig[..., 1]) + eig[..., 2])).astype(np.float32)
    pts = np.where(ok[..., None], moved, x.astype(np.float32))
    return pts, np.where(ok[..., None], n, 0.0).astype(np.float32), np.where(ok, curv, np.float32(0.0))


def _per_cloud(points, lengths):
    points = np.asarray(points, np.float32)
    N, P = points.shape[:2]
    lengths = np.full(N, P, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, P)
    return points, [int(x) for x in lengths]


def smooth_once(points, lengths, r, min_neighbors=3):
    """One pass over a padded batch -> dict(points, normals, curvature, num_neighbors, status, moments; and the float64
    stages delta, eig, n, h, well); zero on padding rows."""
    points, L = _per_cloud(points, lengths)
    N, P = points.shape[:2]
    mom, nn = np.zeros((N, P, 10), np.int64), np.zeros((N, P), np.int64)
    for n, ln in enumerate(L):
        mom[n, :ln], nn[n, :ln] = moments_cloud(points[n, :ln], r)
    f = fit(mom, r)
    live = np.arange(P)[None, :] < np.asarray(L, np.int64).reshape(N, 1)
    st = np.where(live, status_of(nn, f["eig"], min_neighbors), 0).astype(np.uint8)
    pts, nrm, curv = project(points, f["delta"], f["n"], f["eig"], st)
    z = np.float32(0.0)
    nh = f["n"].astype(np.float32).astype(np.float64)
    h = (f["delta"][..., 0] * nh[..., 0] + f["delta"][..., 1] * nh[..., 1]) + f["delta"][..., 2] * nh[..., 2]
    return dict(points=np.where(live[..., None], pts, z), normals=np.where(live[..., None], nrm, z),
                curvature=np.where(live, curv, z), num_neighbors=nn, status=st, moments=mom, delta=f["delta"],
                eig=f["eig"], n=f["n"], h=h, well=well_conditioned(f["eig"]) & (st == 0), live=live)


def smooth(points, lengths, r, min_neighbors=3, iterations=1):
    """`iterations` passes; everything but the points is the last pass's."""
    out = None
    for _ in range(iterations):
        out = smooth_once(points, lengths, r, min_neighbors)
        points = out["points"]
    return out


def mls_float64(p, r, min_neighbors=3):
    """The unquantized plane fit on one cloud (P, 3) float32, over the same supports -> dict(points float64, n, eig,
    curvature, status)."""
    p = np.ascontiguousarray(p, np.float32)
    P = p.shape[0]
    p64 = p.astype(np.float64)
    r2 = np.float32(r) * np.float32(r)
    rr = float(np.float32(r)) ** 2
    pts, nrm, eig, nn = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P, np.int64)
    for a in range(0, P, BLOCK):
        hit = dist2(p[a:a + BLOCK], p) < r2
        d = p64[None, :, :] - p64[a:a + BLOCK, None, :]
        w = np.where(hit, np.clip(1.0 - (d * d).sum(2) / rr, 0.0, None) ** 4, 0.0)
        W = w.sum(1)
        mean = (w[..., None] * d).sum(1) / W[:, None]
        c = d - mean[:, None, :]
        C = np.einsum("ij,ijk,ijl->ikl", w, c, c) / W[:, None, None]
        l, v = np.linalg.eigh(C)
        n = fix_sign(v[..., :, 0])
        h = (mean * n).sum(1)
        pts[a:a + BLOCK] = p64[a:a + BLOCK] + h[:, None] * n
        nrm[a:a + BLOCK], eig[a:a + BLOCK], nn[a:a + BLOCK] = n, l, hit.sum(1)
    st = status_of(nn, eig, min_neighbors)
    ok = st == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = np.where(ok, eig[:, 0] / eig.sum(1), 0.0)
    return dict(points=np.where(ok[:, None], pts, p64), n=np.where(ok[:, None], nrm, 0.0), eig=eig, curvature=curv,
                status=st, well=well_conditioned(eig) & ok)


# ------------------------------------------------------------------------------------------------ scenes
def noisy_sphere(P=600, sigma=0.01, seed=1):
    """P points of the unit sphere, moved along the radius by N(0, sigma)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (1.0 + sigma * rng.normal(size=(P, 1)))).astype(np.float32)


def noisy_plane(P=1500, sigma=0.01, seed=2):
    """P points of the unit square of the plane z = 0, moved along z by N(0, sigma)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0, 1, (P, 2)), sigma * rng.normal(size=(P, 1))], axis=1).astype(np.float32)


def collinear(P=40):
    """P points of a line (exact multiples of a float32 direction): every support is a line, status 2."""
    t = np.arange(P, dtype=np.float32)[:, None] * np.float32(0.03125)
    return (t * np.array([1.0, 0.5, 0.25], np.float32)).astype(np.float32)


def doubled(p):
    """Every point twice: rows P..2P-1 repeat rows 0..P-1."""
    return np.concatenate([p, p]).astype(np.float32)
