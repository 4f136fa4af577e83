"""numpy checker of registration_icp: the REGISTRATION block of include/pointops_amd.h restated stage by stage in float64
(sums in long double), independent of the package, and the experiment every registration test builds on.

Stages, each for ONE cloud:
    nearest          the K=1, L2 search by brute force, distances in unfused float32 as knn_points forms them
    evaluate         inlier mask, count, fitness, inlier_rmse from d2
    plane_moments    A (6,6), b (6) of the point-to-plane normal equations and the majorants of their terms
    point_moments    the weighted-Kabsch inputs of point-to-point
    cholesky_solve   the 6x6 Cholesky with the degeneracy rule
    rotation_delta   Rd = (Rz Ry Rx)^T, exact
    compose          R <- R Rd, T <- (T - c0) Rd + c0 + t
    kabsch           the point-to-point solve (numpy SVD)
    apply            Xt = X R + T in the float32 arithmetic of the kernel
    icp              the whole loop

The sums: every term is formed and added in numpy's long double (64-bit mantissa on x86), so for the few thousand terms
of a test cloud the returned sums are exact to about 2^-53 of sum |terms| -- "exact" against the float64 bounds below.

The bound on the device's sums.  The kernel forms a term of A as J[r] * J[c] and of b as -J[r] * rho in float64 from
float32 inputs: p = Xt - c0 and the differences of rho round once (u = 2^-53 each, usually not at all), each product
once, the subtraction of a cross product once, the two additions of rho once each.  Relative to the MAJORANT of a term
-- the product of (|p_y n_z| + |p_z n_y|)-style sums of absolute values, which is what `abs_A` and `abs_b` accumulate --
J errs by at most 3u, rho by 4u, a term by 8u; adding n terms in any order errs by at most (n - 1) u sum |terms|.  In
all: (n + 7) u * majorant <= n * 2^-52 * majorant for n >= 7.  That is the bound the GPU test applies, with n the number
of inliers (thousands in the stage test)."""
import math
from collections import namedtuple

import numpy as np

U52 = 2.0 ** -52
DEGENERATE_PIVOT = 1e-10   # kIcpDegeneratePivot: a definition (pointops_amd.h, step 6)
MIN_INLIERS = {"point_to_plane": 6, "point_to_point": 3}
RUNNING, CONVERGED, DEGENERATE = 2, 0, 1
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ stages
def nearest(Xt, Y, len_x, len_y):
    """(idx (P1,) int64, d2 (P1,) float32) of the rows < len_x of Xt among the rows < len_y of Y: the smallest
    (d2, index) pair with d2 = (dx*dx + dy*dy) + dz*dz in unfused float32; rows >= len_x, and every row when len_y is
    0, get 0 / 0."""
    Xt, Y = np.asarray(Xt, np.float32), np.asarray(Y, np.float32)
    P1 = Xt.shape[0]
    idx, d2 = np.zeros(P1, np.int64), np.zeros(P1, np.float32)
    if len_x == 0 or len_y == 0:
        return idx, d2
    for a in range(0, len_x, 512):
        x = Xt[a:min(a + 512, len_x), None, :]
        d = x - Y[None, :len_y, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = dd.argmin(1)  # (the first of equal minima: the smallest index)
        idx[a:a + len(j)] = j
        d2[a:a + len(j)] = dd[np.arange(len(j)), j]
    return idx, d2


def r2_of(r_max):
    return np.float32(r_max) * np.float32(r_max)


def evaluate(d2, len_x, len_y, r_max):
    """(mask (P1,) bool, c, fitness float32, inlier_rmse float32, sum d2 exact, as a float)"""
    d2 = np.asarray(d2, np.float32)
    mask = (np.arange(d2.shape[0]) < len_x) & (len_y > 0) & (d2 < r2_of(r_max))
    c = int(mask.sum())
    s = math.fsum(float(v) for v in d2[mask])
    return mask, c, np.float32(c / max(int(len_x), 1)), np.float32(math.sqrt(s / max(c, 1))), s


def _cross_terms(p, n):
    """J (c,6) and its majorant from p (c,3), n (c,3), long double"""
    J = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                  p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], 1)
    ap, an = np.abs(p), np.abs(n)
    M = np.stack([ap[:, 1] * an[:, 2] + ap[:, 2] * an[:, 1], ap[:, 2] * an[:, 0] + ap[:, 0] * an[:, 2],
                  ap[:, 0] * an[:, 1] + ap[:, 1] * an[:, 0], an[:, 0], an[:, 1], an[:, 2]], 1)
    return J, M


PlaneMoments = namedtuple("PlaneMoments", "A b abs_A abs_b c0")


def plane_moments(Xt, Y, normals, idx, mask):
    """A = sum J^T J (6,6), b = -sum J rho (6,) over the inliers about the pivot c0 = Xt[0], and the majorants of their
    terms (module docstring); float64 arrays of long-double sums."""
    rows = np.flatnonzero(mask)
    c0 = np.asarray(Xt[0], np.float64) if Xt.shape[0] else np.zeros(3)
    x = np.asarray(Xt, np.float32)[rows].astype(LD)
    q = np.asarray(Y, np.float32)[idx[rows]].astype(LD)
    n = np.asarray(normals, np.float32)[idx[rows]].astype(LD)
    J, M = _cross_terms(x - c0.astype(LD), n)
    rho = ((x - q) * n).sum(1)
    arho = (np.abs(x - q) * np.abs(n)).sum(1)
    A = (J[:, :, None] * J[:, None, :]).sum(0)
    b = -(J * rho[:, None]).sum(0)
    abs_A = (M[:, :, None] * M[:, None, :]).sum(0)
    abs_b = (M * arho[:, None]).sum(0)
    return PlaneMoments(*(np.asarray(v, np.float64) for v in (A, b, abs_A, abs_b)), c0)


def upper(A):
    """the 21 entries of the upper triangle, row by row: the kernel's layout"""
    return np.array([A[r, c] for r in range(6) for c in range(r, 6)])


def point_moments(X, Y, idx, mask):
    """(xs (c,3), ys (c,3)) long double: the ORIGINAL source rows and their targets, the inliers only"""
    rows = np.flatnonzero(mask)
    return np.asarray(X, np.float32)[rows].astype(LD), np.asarray(Y, np.float32)[idx[rows]].astype(LD)


def alignment_moments(X, Y, idx, mask):
    """The 24 moments of pointops_points_alignment with weights 1 / 0 about the pivots X[0], Y[0] (Sw, Sw2, Swx, Swy,
    Sw2x, Sw2y, Sxy row-major, Sxx), and the sums of the absolute values of their terms."""
    xs, ys = point_moments(X, Y, idx, mask)
    xc, yc = xs - np.asarray(X[0], np.float32).astype(LD), ys - np.asarray(Y[0], np.float32).astype(LD)
    c = LD(xs.shape[0])

    def both(f):
        return f(xc, yc), f(np.abs(xc), np.abs(yc))

    parts = [both(lambda a, b: np.array([c, c])), both(lambda a, b: a.sum(0)), both(lambda a, b: b.sum(0)),
             both(lambda a, b: a.sum(0)), both(lambda a, b: b.sum(0)),
             both(lambda a, b: (a[:, :, None] * b[:, None, :]).sum(0).ravel()), both(lambda a, b: np.array([(a * a).sum()]))]
    return (np.concatenate([np.asarray(p[0], np.float64) for p in parts]),
            np.concatenate([np.asarray(p[1], np.float64) for p in parts]))


def cholesky_solve(A, b):
    """x with A x = b by A = L L^T, or None when pivot j is not greater than DEGENERATE_PIVOT * A[j][j] (step 6)."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    L = np.zeros((6, 6))
    for j in range(6):
        piv = A[j, j] - float(np.dot(L[j, :j], L[j, :j]))
        if not piv > DEGENERATE_PIVOT * A[j, j]:
            return None
        L[j, j] = math.sqrt(piv)
        for i in range(j + 1, 6):
            L[i, j] = (A[j, i] - float(np.dot(L[i, :j], L[j, :j]))) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (b[i] - float(np.dot(L[i, :i], y[:i]))) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - float(np.dot(L[i + 1:, i], x[i + 1:]))) / L[i, i]
    return x


def rotation_delta(alpha, beta, gamma):
    ca, sa, cb, sb, cg, sg = (math.cos(alpha), math.sin(alpha), math.cos(beta), math.sin(beta), math.cos(gamma),
                              math.sin(gamma))
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).T


def compose(R, T, Rd, c0, t):
    return R @ Rd, (T - c0) @ Rd + c0 + t


def kabsch(xs, ys):
    """(R, T) minimising sum |x R + T - y|^2 over the rows: no scale, no reflection (row-vector convention)."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    xm, ym = xs.mean(0), ys.mean(0)
    C = (xs - xm).T @ (ys - ym) / xs.shape[0]
    Um, _, Vh = np.linalg.svd(C)
    E = np.diag([1.0, 1.0, np.sign(np.linalg.det(Um @ Vh)) or 1.0])
    R = Um @ E @ Vh
    return R, ym - xm @ R


def apply(X, R, T, len_x):
    """Xt = X R + T from the float32 roundings of R, T: v = ((x0 R[0][k] + x1 R[1][k]) + x2 R[2][k]) + T[k] in unfused
    float32; rows >= len_x zero."""
    X = np.asarray(X, np.float32)
    R32, T32 = np.asarray(R, np.float64).astype(np.float32), np.asarray(T, np.float64).astype(np.float32)
    out = np.zeros_like(X)
    for k in range(3):
        out[:, k] = ((X[:, 0] * R32[0, k] + X[:, 1] * R32[1, k]) + X[:, 2] * R32[2, k]) + T32[k]
    out[len_x:] = 0
    return out


# ------------------------------------------------------------------------------------------------ the loop
RefRegistration = namedtuple("RefRegistration", "R T fitness inlier_rmse c correspondences status iterations Xt history")


def update(X, Xt, Y, normals, idx, mask, c, estimation, R, T):
    """Steps 5 and 6: (R, T, moved)"""
    if c < MIN_INLIERS[estimation]:
        return R, T, False
    if estimation == "point_to_plane":
        m = plane_moments(Xt, Y, normals, idx, mask)
        x = cholesky_solve(m.A, m.b)
        if x is None:
            return R, T, False
        R, T = compose(R, T, rotation_delta(*x[:3]), m.c0, x[3:])
        return R, T, True
    R, T = kabsch(*point_moments(X, Y, idx, mask))
    return R, T, True


def icp(X, Y, len_x, len_y, r_max, estimation="point_to_plane", normals=None, R0=None, T0=None, max_iterations=30,
        relative_fitness=1e-6, relative_rmse=1e-6, search=nearest):
    """The whole loop for ONE cloud, brute-force nearest neighbours: max_iterations updating steps, then one
    evaluate-only step, stopping early once the cloud is frozen."""
    R = np.eye(3) if R0 is None else np.asarray(R0, np.float32).astype(np.float64)
    T = np.zeros(3) if T0 is None else np.asarray(T0, np.float32).astype(np.float64)
    Xt = apply(X, R, T, len_x)
    status, iterations, prev, history = RUNNING, 0, None, []
    for i in range(max_iterations + 1):
        idx, d2 = search(Xt, Y, len_x, len_y)
        mask, c, fit, rmse, _ = evaluate(d2, len_x, len_y, r_max)
        corr = np.where(mask, idx, -1)
        settled = prev is not None and abs(float(fit) - float(prev[0])) < relative_fitness \
            and abs(float(rmse) - float(prev[1])) < relative_rmse
        prev = (fit, rmse)
        if settled:
            status = CONVERGED
        elif i < max_iterations:
            R, T, moved = update(X, Xt, Y, normals, idx, mask, c, estimation, R, T)
            if moved:
                iterations += 1
                Xt = apply(X, R, T, len_x)
            else:
                status = DEGENERATE
        history.append((R.copy(), T.copy(), fit, rmse))
        if status != RUNNING:
            break
    return RefRegistration(R, T, fit, rmse, c, corr, status, iterations, Xt, history)


# ------------------------------------------------------------------------------------------------ the experiment
def surface(x, y):
    return 0.2 * np.sin(3.0 * x) * np.cos(2.0 * y)


def surface_normals(x, y):
    n = np.stack([-0.6 * np.cos(3.0 * x) * np.cos(2.0 * y), 0.4 * np.sin(3.0 * x) * np.sin(2.0 * y), np.ones_like(x)], 1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def rotation(axis, angle):
    """(3,3) rotation about `axis` by `angle` (Rodrigues) for the row-vector convention x -> x R."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K).T


R_MAX = 0.08
ANGLE, SHIFT = 0.12, np.array([0.02, -0.02, 0.02])  # |t| ~ 0.035
Scene = namedtuple("Scene", "X Y normals R_true T_true overlap")


def scene(seed, P1, P2, clutter=True, angle=ANGLE, shift=SHIFT):
    """The experiment of the issue at any size: the target is P2 points on z = 0.2 sin 3x cos 2y over a square whose
    side keeps the density of 3000 points on [-1, 1]^2; the source is a moved subset of 3/4 of P1 of its rows (of all
    P1 without `clutter`) plus P1/4 rows of clutter 1.5 above the surface, in random order.  (R_true, T_true) takes the
    source onto the target: X R_true + T_true = Y[subset] up to float32 rounding, so at the true pose the overlap rows
    are inliers at any sensible threshold and the clutter rows, 1.5 away, are not.  The motion is `angle` rad about a
    fixed oblique axis and |shift| ~ 0.035."""
    rng = np.random.default_rng(seed)
    half = math.sqrt(P2 / 3000.0)
    xy = rng.uniform(-half, half, (P2, 2))
    Y = np.concatenate([xy, surface(xy[:, 0], xy[:, 1])[:, None]], 1)
    normals = surface_normals(xy[:, 0], xy[:, 1])
    n_over = P1 - P1 // 4 if clutter else P1
    assert n_over <= P2
    rows = rng.permutation(P2)[:n_over]
    moved = Y[rows]
    if clutter:
        cxy = rng.uniform(-half, half, (P1 - n_over, 2))
        moved = np.concatenate([moved, np.concatenate([cxy, surface(cxy[:, 0], cxy[:, 1])[:, None] + 1.5], 1)])
    order = rng.permutation(P1)
    moved = moved[order]
    R_true = rotation([0.3, -0.5, 0.8], angle)
    T_true = np.asarray(shift, np.float64)
    X = (moved - T_true) @ R_true.T  # (x R + T = moved)
    return Scene(X.astype(np.float32), Y.astype(np.float32), normals.astype(np.float32), R_true, T_true,
                 n_over)


def planar_scene(seed, P1, P2):
    """One tilted plane as the target (constant normals): the normal equations have rank 3 -- rotation about the
    normal and the two translations in the plane are free -- so point-to-plane must freeze as degenerate.  The source
    is a subset moved by a small motion, so that most of its rows are inliers at R_MAX."""
    rng = np.random.default_rng(seed)
    half = math.sqrt(P2 / 3000.0)
    n = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    e1 = np.cross(n, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    uv = rng.uniform(-half, half, (P2, 2))
    Y = uv[:, :1] * e1 + uv[:, 1:] * e2
    R_true, T_true = rotation([0.3, -0.5, 0.8], 0.02), np.array([0.01, -0.01, 0.01])
    X = (Y[rng.permutation(P2)[:P1]] - T_true) @ R_true.T
    return Scene(X.astype(np.float32), Y.astype(np.float32), np.broadcast_to(n, (P2, 3)).astype(np.float32), R_true,
                 T_true, P1)


def pose_error(R, T, sc):
    """(|R - R*| in the Frobenius norm, |T - T*| in the Euclidean norm)"""
    return float(np.linalg.norm(np.asarray(R, np.float64) - sc.R_true)), \
        float(np.linalg.norm(np.asarray(T, np.float64) - sc.T_true))
