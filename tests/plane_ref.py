"""Checker for segment_plane (functions/plane.py): the definition in the comment of pointops_segment_plane
(include/pointops_amd.h) restated in numpy, independent of the package.

Draws and selection are integers (ransac_ref.hash32 / draw / select: the same counter-based hash).  The plane of a triple
and its validity tests are float64 in the operation order of the definition -- multiplies and adds only, so the flags
are bit-reproducible --, rounded once to float32.  Residuals, counts and masks take `dtype`: np.float32 reproduces the
kernels' operation order (numpy's float32 arithmetic is IEEE and unfused, as the build's -ffp-contract=off makes the
kernels'), np.float64 is the reference.  Refits are float64 (np.linalg.eigh of the centred covariance), rounded once.

So that no threshold decision is ever compared across precisions, the GPU suite checks in stages: the samples against
`draw_samples`; flags and planes against `planes_of` on the device's samples; the counts against `counts` in float32 on
the device's planes; `best` against `select` on the device's counts; the final mask against `evaluate` in float32 on the
device's final plane.

rmse bound (`rmse_bound`).  r = ((x a + y b) + z c) + d in fp32 has four roundings that matter beyond the products'
own: each intermediate is at most S = 3 max|p| + |d| in magnitude (|a|, |b|, |c| <= 1), so |r - r64| <= 4u S with
u = 2^-24 (the three products' roundings are inside the first two sums' bound to first order: 3u max|p| each is counted
in S).  The rms over the inliers is 1-Lipschitz in the residual vector's max norm, and the final rounding to fp32 costs
u rmse <= u thr.  The fp64 sum is exact at this scale.  Together |rmse - rmse64| <= 5 * 2^-24 * (3 max|p| + |d| + thr).
"""
import numpy as np

import ransac_ref

THR = 0.02
U32 = 2.0 ** -24
DEGENERATE = 1e-12


# ------------------------------------------------------------------------------------------------ rows and draws
def valid_rows(lengths, mask, N, P):
    """(N,P) bool: row i < lengths[n] and mask[n,i]."""
    ok = np.arange(P)[None, :] < ransac_ref.lengths_of(lengths, N, P)[:, None]
    return ok if mask is None else ok & np.asarray(mask, bool)


def draw_samples(valid, H, seed, first_cloud=0):
    """(N,H,3) int64 rows: the drawn triples, -1 for a cloud with fewer than three valid rows."""
    N = valid.shape[0]
    out = np.full((N, H, 3), -1, np.int64)
    for n in range(N):
        v = np.nonzero(valid[n])[0]
        if len(v) >= 3:
            out[n] = v[ransac_ref.draw(seed, first_cloud + n, H, len(v))]
    return out


def gather_triples(X, valid, samples):
    """p (N,H,3 points,3) float32 and ok (N,H): the three rows are distinct valid rows."""
    N, P = valid.shape
    inside = (samples >= 0) & (samples < P)
    rows = np.where(inside, samples, 0)
    n = np.arange(N)[:, None, None]
    good = inside & (valid[n, rows] if P else False)
    ok = good.all(2) & (samples[..., 0] != samples[..., 1]) & (samples[..., 0] != samples[..., 2]) \
        & (samples[..., 1] != samples[..., 2])
    p = X[n, rows] if P else np.zeros(samples.shape + (3,), np.float32)
    return np.where(good[..., None], p, np.float32(0)), ok


# ------------------------------------------------------------------------------------------------ planes
def cone_of(axis, max_angle_deg):
    """(axis as three float32 of unit length, cos as float32), as functions/plane.py hands them to the kernels."""
    if axis is None:
        return None
    a = np.asarray(axis, np.float64)
    a32 = (a / np.sqrt((a * a).sum())).astype(np.float32)
    c32 = np.float32(0.0 if max_angle_deg >= 90.0 else min(max(np.cos(np.radians(float(max_angle_deg))), 0.0), 1.0))
    return a32, c32


def _sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def _axis_dot(v, cone):
    a = cone[0].astype(np.float64)
    return (v[..., 0] * a[0] + v[..., 1] * a[1]) + v[..., 2] * a[2]


def in_cone(v, sq, cone):
    dot, c = _axis_dot(v, cone), np.float64(cone[1])
    return dot * dot >= (c * c) * sq


def orient(n, d, cone):
    """The sign rule on float64 normals n (...,3) and offsets d (...)."""
    if cone is not None:
        flip = _axis_dot(n, cone) < 0.0
    else:
        a = np.abs(n)
        k = np.where(a[..., 1] > a[..., 0], 1, 0)
        k = np.where(a[..., 2] > np.take_along_axis(a, k[..., None], -1)[..., 0], 2, k)
        flip = np.take_along_axis(n, k[..., None], -1)[..., 0] < 0.0
    return np.where(flip[..., None], -n, n), np.where(flip, -d, d)


def planes_of(p, ok, cone=None):
    """Triples p (...,3,3) float32 with flags ok -> (planes (...,4) float32, valid (...), planes64 (...,4) float64 before
    the rounding): step 4 of the definition; invalid slots hold zeros."""
    with np.errstate(all="ignore"):
        p = np.asarray(p, np.float32).astype(np.float64)
        p0 = p[..., 0, :]
        e1, e2 = p[..., 1, :] - p0, p[..., 2, :] - p0
        c = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                      e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                      e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
        sq = _sq(c)
        valid = ok & (sq > (DEGENERATE * _sq(e1)) * _sq(e2))
        if cone is not None:
            valid &= in_cone(c, sq, cone)
        n = c / np.sqrt(sq)[..., None]
        d = -((n[..., 0] * p0[..., 0] + n[..., 1] * p0[..., 1]) + n[..., 2] * p0[..., 2])
        n, d = orient(n, d, cone)
        pl64 = np.concatenate([n, d[..., None]], -1)
        pl32 = pl64.astype(np.float32)
        valid &= np.isfinite(pl32[..., 3])
    pl64 = np.where(valid[..., None], pl64, 0.0)
    return np.where(valid[..., None], pl32, np.float32(0)), valid, pl64


def ulp32(x):
    """The spacing of float32 at |x| (float64 array), at least the smallest normal's."""
    return np.spacing(np.maximum(np.abs(x), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ residuals
def residual(planes, pts, dtype=np.float32):
    """r of points pts (M,3) under planes (...,4) -> (..., M), in the kernels' order."""
    pl, x = np.asarray(planes, dtype)[..., None, :], np.asarray(pts, dtype)
    return ((x[:, 0] * pl[..., 0] + x[:, 1] * pl[..., 1]) + x[:, 2] * pl[..., 2]) + pl[..., 3]


def counts(planes, valid, X, rows, thr, dtype=np.float32, block=256):
    """(N,H) int32 counts of planes (N,H,4) with flags valid (N,H) over the valid rows `rows` (N,P): -1 where invalid."""
    N, H = valid.shape
    t = dtype(np.float32(thr))
    out = np.full((N, H), -1, np.int32)
    for n in range(N):
        x = X[n, rows[n]]
        for a in range(0, H, block):
            out[n, a:a + block] = (np.abs(residual(planes[n, a:a + block], x, dtype)) <= t).sum(1)
        out[n, ~valid[n]] = -1
    return out


def evaluate(planes, X, rows, thr, dtype=np.float32):
    """One plane per cloud -> mask (N,P) bool, count (N,) int64, rmse (N,) float64 (r*r and the sum in float64)."""
    N, P = rows.shape
    t = dtype(np.float32(thr))
    mask = np.zeros((N, P), bool)
    rmse = np.zeros(N)
    for n in range(N):
        v = np.nonzero(rows[n])[0]
        if len(v) == 0:
            continue
        r = residual(planes[n], X[n, v], dtype)
        inl = np.abs(r) <= t
        mask[n, v[inl]] = True
        rmse[n] = np.sqrt((r[inl].astype(np.float64) ** 2).sum() / max(int(inl.sum()), 1))
    return mask, mask.sum(1).astype(np.int64), rmse


def rmse64(planes, X, mask):
    """rmse of the given mask under the given (fp32) planes, everything in float64."""
    out = np.zeros(len(mask))
    for n in range(len(mask)):
        v = np.nonzero(mask[n])[0]
        if len(v):
            r = residual(planes[n], X[n, v], np.float64)
            out[n] = np.sqrt((r * r).sum() / len(v))
    return out


def rmse_bound(planes, X, thr):
    """(N,) the absolute bound of the module docstring (a coordinate that is not finite is in no inlier: left out)."""
    mx = np.abs(np.where(np.isfinite(X), X, 0)).reshape(len(X), -1).max(1) if X.shape[1] else np.zeros(len(X))
    return 5.0 * U32 * (3.0 * mx + np.abs(planes[:, 3].astype(np.float64)) + thr)


# ------------------------------------------------------------------------------------------------ refits
def fit_mask(X, mask, cone=None):
    """Float64 least-squares plane of every cloud's masked rows: (planes (N,4) float64, ok (N,), eigenvalues (N,3))."""
    N = len(mask)
    planes, ok, lam = np.zeros((N, 4)), np.zeros(N, bool), np.zeros((N, 3))
    for n in range(N):
        q = X[n, mask[n]].astype(np.float64)
        if len(q) < 3 or not np.isfinite(q).all():
            continue
        m = q.mean(0)
        w, v = np.linalg.eigh((q - m).T @ (q - m) / len(q))
        nrm = v[:, 0]
        if cone is not None and not in_cone(nrm, _sq(nrm), cone):
            continue
        nrm, d = orient(nrm, np.float64(-(nrm @ m)), cone)
        planes[n, :3], planes[n, 3], ok[n], lam[n] = nrm, d, True, w
    return planes, ok, lam


def refine(plane, best, X, rows, thr, refine_steps, cone=None, dtype=np.float32):
    """Steps 7-9 from the winners' planes (N,4): evaluate, then refit / evaluate / accept.  Returns planes (float32),
    mask, count, rmse and the number of accepted refits per cloud."""
    N = len(best)
    planes = np.array(plane, np.float32)
    none = best < 0
    planes[none] = 0
    mask, cnt, rmse = evaluate(planes, X, rows, thr, dtype)
    mask[none], cnt[none], rmse[none] = False, 0, 0.0
    stopped = none.copy()
    accepted = np.zeros(N, np.int64)
    for _ in range(refine_steps):
        fit, fit_ok, _ = fit_mask(X, mask, cone)
        fit = fit.astype(np.float32)  # (the kernels round the fit to fp32 once)
        mc, cc, rc = evaluate(fit, X, rows, thr, dtype)
        ok = ~stopped & fit_ok & (cc >= cnt)
        stopped |= ~ok
        planes[ok], mask[ok], cnt[ok], rmse[ok] = fit[ok], mc[ok], cc[ok], rc[ok]
        accepted += ok
    return planes, mask, cnt, rmse, accepted


def run(X, lengths=None, mask=None, *, thr=THR, H=256, refine_steps=2, seed=0, samples=None, first_cloud=0,
        axis=None, max_angle_deg=None, dtype=np.float64):
    """The whole definition; a dict of every stage."""
    X = np.asarray(X, np.float32)
    N, P = X.shape[:2]
    rows = valid_rows(lengths, mask, N, P)
    cone = cone_of(axis, max_angle_deg)
    samples = draw_samples(rows, H, seed, first_cloud) if samples is None else np.asarray(samples, np.int64)
    p, ok = gather_triples(X, rows, samples)
    hyp, valid, hyp64 = planes_of(p, ok, cone)
    cnt = counts(hyp, valid, X, rows, thr, dtype)
    best = ransac_ref.select(cnt)
    n, b = np.arange(N), np.maximum(best, 0)
    planes, m, num, rmse, accepted = refine(hyp[n, b], best, X, rows, thr, refine_steps, cone, dtype)
    return dict(rows=rows, samples=samples, valid=valid, hyp=hyp, hyp64=hyp64, counts=cnt, best=best, planes=planes,
                mask=m, num_inliers=num, rmse=rmse, accepted=accepted)


# ------------------------------------------------------------------------------------------------ scenes
def basis(normal):
    """Two unit vectors that complete the unit vector `normal` to an orthonormal frame."""
    k = int(np.argmin(np.abs(normal)))
    b1 = np.cross(normal, np.eye(3)[k])
    b1 /= np.linalg.norm(b1)
    return b1, np.cross(normal, b1)


def scatter_on_plane(rng, count, normal, centre, thr, extent=0.5, noise=0.1, aspect=1.0):
    """`count` float64 points on the patch [-extent, extent] x [-aspect extent, aspect extent] of the plane through
    `centre`, at most `noise` thr off it."""
    b1, b2 = basis(normal)
    u, v = rng.uniform(-extent, extent, count), rng.uniform(-extent, extent, count) * aspect
    s = rng.uniform(-noise, noise, count) * thr
    return centre + u[:, None] * b1 + v[:, None] * b2 + s[:, None] * normal


def scene(seed, P, ratio, N=1, thr=THR, lengths=False, offset=0.0, masked=None, normal=None):
    """One seeded scene: per cloud a planted patch (extent 1 x 1, noise 0.1 thr along the normal) holding `ratio` of the
    valid rows, every other valid row 5 thr to half a unit off the plane on either side.  `masked`: that many valid
    rows (the mask switches off the others, scattered); `lengths`: ragged.  `offset` moves everything along (1,1,1).
    Returns a dict with X (N,P,3) float32, len (None unless `lengths`), mask (None unless `masked`), planted (N,P) bool,
    normal (N,3), centre (N,3), thr."""
    rng = np.random.default_rng(7100 + seed)
    X = np.zeros((N, P, 3), np.float32)
    lens = np.full(N, P, np.int64)
    if lengths:
        lens = np.maximum(P - rng.integers(0, max(P // 4, 1), N), min(P, 3)).astype(np.int64)
    mask = None
    if masked is not None:
        mask = np.zeros((N, P), bool)
        for n in range(N):
            mask[n, rng.permutation(int(lens[n]))[:masked]] = True
    planted = np.zeros((N, P), bool)
    normals, centres = np.zeros((N, 3)), np.zeros((N, 3))
    for n in range(N):
        nrm = rng.standard_normal(3) if normal is None else np.asarray(normal, np.float64)
        nrm = nrm / np.linalg.norm(nrm)
        centre = rng.uniform(-0.2, 0.2, 3) + offset
        normals[n], centres[n] = nrm, centre
        # rows outside the cloud or the mask hold points ON the plane: counting one of them would show
        X[n] = scatter_on_plane(rng, P, nrm, centre, thr, noise=0.0).astype(np.float32)
        v = np.nonzero(valid_rows(lens[n:n + 1], None if mask is None else mask[n:n + 1], 1, P)[0])[0]
        k = max(int(round(ratio * len(v))), min(3, len(v)))
        chosen = v[rng.permutation(len(v))[:k]]
        planted[n, chosen] = True
        X[n, chosen] = scatter_on_plane(rng, k, nrm, centre, thr).astype(np.float32)
        others = v[~planted[n, v]]
        far = scatter_on_plane(rng, len(others), nrm, centre, thr, noise=0.0)
        far += (rng.uniform(5.0 * thr, 0.5, len(others)) * rng.choice([-1.0, 1.0], len(others)))[:, None] * nrm
        X[n, others] = far.astype(np.float32)
    return dict(X=X, len=lens if lengths else None, mask=mask, planted=planted, normal=normals, centre=centres, thr=thr)


def scene_margins(sc):
    """(largest planted distance, smallest other valid distance) from the planted plane, in units of thr."""
    X = sc["X"].astype(np.float64)
    N, P = X.shape[:2]
    rows = valid_rows(sc["len"], sc["mask"], N, P)
    worst_in, best_out = 0.0, np.inf
    for n in range(N):
        d = np.abs((X[n] - sc["centre"][n]) @ sc["normal"][n])
        p, o = sc["planted"][n], rows[n] & ~sc["planted"][n]
        worst_in = max(worst_in, d[p].max() if p.any() else 0.0)
        best_out = min(best_out, d[o].min() if o.any() else np.inf)
    return worst_in / sc["thr"], best_out / sc["thr"]


def planted_fit(sc, cone=None):
    """The float64 least-squares plane of the planted rows (N,4) and the eigenvalues of their covariance (N,3)."""
    planes, ok, lam = fit_mask(sc["X"], sc["planted"], cone)
    assert ok.all()
    return planes, lam


# ------------------------------------------------------------------------------------------------ the GPU suite's scenes
CHUNK = 512  # records per scoring workgroup (test_plane_cpu.py holds it to _C_plane.PLANE_CHUNK)

# name -> scene() arguments, plus the run's H / refine_steps / axis / max_angle_deg; planted=False: too few hypotheses
# to promise the planted set, the stages are still compared
SCENES = {
    "p255": dict(seed=1, P=255, ratio=0.5, H=256, refine_steps=0),
    "p256": dict(seed=2, P=256, ratio=0.5, H=256, refine_steps=1),
    "p257": dict(seed=3, P=257, ratio=0.5, H=256, refine_steps=3),
    "p1000": dict(seed=4, P=1000, ratio=0.4, H=1024, N=3, lengths=True),
    "p2047": dict(seed=5, P=2047, ratio=0.4, H=256),  # the compaction walks 2048 rows per step
    "p2048": dict(seed=6, P=2048, ratio=0.4, H=256),
    "p2049": dict(seed=7, P=2049, ratio=0.4, H=256),
    # three tiles: the third adds the counts of two.  The mask switches rows off in all of them: the third tile is row
    # 4096 alone, valid in cloud 0 (its record follows those of both earlier tiles) and masked out in cloud 1
    "p4097": dict(seed=52, P=4097, ratio=0.4, H=256, N=2, masked=3600),
    # 33 tiles, and the first P at which the evaluation's 32 blocks walk their rows twice
    "p65537": dict(seed=60, P=65537, ratio=0.5, H=64, refine_steps=1),
    "chunk-1": dict(seed=8, P=CHUNK + 90, masked=CHUNK - 1, ratio=0.5, H=256),
    "chunk": dict(seed=9, P=CHUNK + 90, masked=CHUNK, ratio=0.5, H=256),
    "chunk+1": dict(seed=10, P=CHUNK + 90, masked=CHUNK + 1, ratio=0.5, H=256),
    "2chunk+1": dict(seed=11, P=2 * CHUNK + 90, masked=2 * CHUNK + 1, ratio=0.5, H=256),
    # the pivot of the refit.  (At 1e3 the fp32 residual is good to about 1e-4, so a float32 count differs from the float64
    # one once in a few thousand residuals: few hypotheses, and a seed where none does -- test_plane_cpu.py holds it.)
    "offset": dict(seed=30, P=300, ratio=0.5, H=32, offset=1000.0, thr=0.05),
    "cone-in": dict(seed=13, P=300, ratio=0.5, H=256, normal=(0.05, -0.08, 1.0), axis=(0.0, 0.0, 1.0), max_angle_deg=10.0),
    "h1": dict(seed=14, P=300, ratio=0.5, H=1, planted=False),
    "h63": dict(seed=15, P=300, ratio=0.5, H=63, planted=False),
    "h64": dict(seed=16, P=300, ratio=0.5, H=64, planted=False),
    "h65": dict(seed=17, P=300, ratio=0.5, H=65, planted=False),
}


def make_scene(name):
    """(scene dict, keyword arguments of run() / of segment_plane's checker)."""
    a = dict(SCENES[name])
    a.pop("planted", None)
    kw = dict(H=a.pop("H"), refine_steps=a.pop("refine_steps", 2), seed=100 + a["seed"], thr=a.get("thr", THR),
              axis=a.pop("axis", None), max_angle_deg=a.pop("max_angle_deg", None))
    return scene(**a), kw


def cone_outside_scene():
    """(scene, run keywords): the planted floor leans 30 degrees off z and the cone allows 10, so the floor's triples
    are thrown out and whatever wins holds far fewer rows than the floor has."""
    sc = scene(21, 300, 0.5, normal=(0.0, np.sin(np.radians(30.0)), np.cos(np.radians(30.0))))
    return sc, dict(H=256, refine_steps=2, seed=121, thr=THR, axis=(0.0, 0.0, 1.0), max_angle_deg=10.0)


def floor_and_blobs_scene():
    """(X (1,2080,3) float32, floor (1,2080) bool, eps, min_points, thr): a floor of 40 x 40 points 0.05 apart and three
    blobs of 160 points resting on it, from 0.03 above it, a unit apart; the rows are shuffled."""
    rng = np.random.default_rng(7600)
    gx, gy = np.meshgrid(np.arange(40) * 0.05, np.arange(40) * 0.05)
    floor = np.stack([gx.ravel(), gy.ravel(), np.zeros(1600)], 1) + rng.uniform(-0.002, 0.002, (1600, 3))
    blobs = []
    for cx, cy in ((0.4, 0.4), (1.4, 0.5), (0.9, 1.5)):
        b = rng.uniform(-0.1, 0.1, (160, 3)) + np.array([cx, cy, 0.0])
        b[:, 2] = rng.uniform(0.03, 0.23, 160)
        blobs.append(b)
    pts = np.concatenate([floor] + blobs)
    order = rng.permutation(len(pts))
    return pts[order][None].astype(np.float32), (order < 1600)[None], 0.08, 4, 0.01


def rejected_refit_scene():
    """(X, samples, thr): three points on z = 0 (the only triple), five points 0.8 thr above the plane and one 0.8 thr
    below it.  The winner z = 0 holds all nine; the least-squares refit moves about 0.36 thr towards the five and
    loses the one below, so it is rejected."""
    thr = 0.05
    rng = np.random.default_rng(7300)
    X = rng.uniform(0, 1, (1, 9, 3)).astype(np.float32)
    X[0, :3, 2] = 0.0
    X[0, 3:8, 2] = np.float32(0.8 * thr)
    X[0, 8, :2] = X[0, :8, :2].mean(0)  # the one sits at the centroid, where the refit's tilt cannot reach it
    X[0, 8, 2] = np.float32(-0.8 * thr)
    return X, np.array([[[0, 1, 2]]], np.int64), thr
