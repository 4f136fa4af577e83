"""Plain numpy restatements of the operators built on the searches (csrc/covariance.hip, local_frames.hip,
points_alignment.hip), independent of the package; validated on the CPU by test_derived_ref_cpu.py and used by
test_derived_edges_gpu.py.

fp32 restatements repeat the kernel's arithmetic operation by operation (numpy float32 ufuncs are IEEE single and never
fused; the library is built with -ffp-contract=off), so the kernels are held to them bit for bit:
    cov_fp32            m = (((0 + x_0) + x_1) + ...) * inv_k;  c = (((0 + v_0 v_0^T) + v_1 v_1^T) + ...) * inv_k with
                        v_k = x_k - m and inv_k = float32(1) / float32(K), multiplied, never divided by K
    cov_backward_fp32   s = (G + G^T) * inv_k;  grad_x_k[a] = ((0 + s[a][0] v_k[0]) + s[a][1] v_k[1]) + ...
float64 evaluations state the closed forms the kernels document:
    gather_neighbourhoods       the gather rule of local_frames (zero rows for k >= lengths[n] or idx outside [0, P))
    local_frames_backward_f64   the fold of y = n x z, then grad_C = sum_{j,q} w[j][q] v_j v_q^T
    alignment_moments_f64       the moments about the pivots (row 0 of X and of Y), layout of PaSlot, long-double sums
    alignment_backward_f64      the gradient of those moments pushed to X, Y and the weights
"""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ covariance
def cov_fp32(knn):
    """knn (..., K, D) fp32 -> cov (..., D, D) fp32 in the kernel's order."""
    x = np.ascontiguousarray(knn, dtype=F32)
    K, D = x.shape[-2:]
    x = x.reshape(-1, K, D)
    inv_k = F32(1.0) / F32(K)
    m = np.zeros((x.shape[0], D), F32)
    for k in range(K):
        m = m + x[:, k]
    m = m * inv_k
    c = np.zeros((x.shape[0], D, D), F32)
    for k in range(K):
        v = x[:, k] - m
        c = c + v[:, :, None] * v[:, None, :]
    c = c * inv_k
    assert c.dtype == F32
    return c.reshape(knn.shape[:-2] + (D, D))


def cov_backward_fp32(knn, grad_cov):
    """knn (..., K, D), grad_cov (..., D, D) fp32 -> grad_knn (..., K, D) fp32 in the kernel's order."""
    x = np.ascontiguousarray(knn, dtype=F32)
    K, D = x.shape[-2:]
    x = x.reshape(-1, K, D)
    g = np.ascontiguousarray(grad_cov, dtype=F32).reshape(-1, D, D)
    inv_k = F32(1.0) / F32(K)
    m = np.zeros((x.shape[0], D), F32)
    for k in range(K):
        m = m + x[:, k]
    m = m * inv_k
    s = (g + g.transpose(0, 2, 1)) * inv_k
    out = np.zeros_like(x)
    for k in range(K):
        v = x[:, k] - m
        acc = np.zeros((x.shape[0], D), F32)
        for b in range(D):
            acc = acc + s[:, :, b] * v[:, b, None]
        out[:, k] = acc
    assert out.dtype == F32
    return out.reshape(knn.shape)


def cov_f64(knn):
    x = np.asarray(knn, np.float64)
    v = x - x.mean(-2, keepdims=True)
    return np.einsum("...ka,...kb->...ab", v, v) / x.shape[-2]


def cov_backward_f64(knn, grad_cov):
    x, g = np.asarray(knn, np.float64), np.asarray(grad_cov, np.float64)
    v = x - x.mean(-2, keepdims=True)
    return np.einsum("...ab,...kb->...ka", g + np.swapaxes(g, -1, -2), v) / x.shape[-2]


# ------------------------------------------------------------------------------------------------ local frames
def gather_neighbourhoods(points, idx, lengths):
    """points (N,P,3), idx (N,P,K) int64, lengths (N,) -> (N,P,K,3): neighbour k of row i is points[n, idx] when
    0 <= idx < P and k < lengths[n], else a zero row.  (Rows i >= lengths[n] are gathered by the same rule; the
    operator's outputs there are zero.)"""
    points, idx = np.asarray(points), np.asarray(idx)
    N, P, K = idx.shape
    out = np.zeros((N, P, K, points.shape[2]), points.dtype)
    for n in range(N):
        ok = (idx[n] >= 0) & (idx[n] < P) & (np.arange(K)[None, :] < int(lengths[n]))
        if P > 0:
            out[n] = np.where(ok[..., None], points[n][np.where(ok, idx[n], 0)], 0)
    return out


def valid_rows(lengths, P):
    return np.arange(P)[None, :] < np.asarray(lengths)[:, None]


def local_frames_backward_f64(curv, frames, g_curv, g_frames, lengths, disambiguate):
    """float64 closed form of local_frames_backward on the fp32 inputs -> (grad_cov (N,P,3,3), wabs (N,P)) with
    wabs = sum_{j,q} |w[j][q]|.  frames[..., a, j] = component a of column j.  With `disambiguate` the middle column
    is y = n x z: g_n += z x g_y, g_z += g_y x n, g_y = 0.  Then w[j][j] = g_lambda_j and, for j != q,
    w[j][q] = (v_j . g_q) / (lambda_q - lambda_j);  grad_C = sum_{j,q} w[j][q] v_j v_q^T.  Rows i >= lengths[n]: zero.
    Equal eigenvalues divide by zero (inf / nan there), as documented."""
    lam = np.asarray(curv, np.float64)
    V = np.asarray(frames, np.float64)
    gl = np.asarray(g_curv, np.float64)
    gV = np.array(g_frames, np.float64)
    if disambiguate:
        n, z, gy = V[..., :, 0], V[..., :, 2], gV[..., :, 1].copy()
        gV[..., :, 0] += np.cross(z, gy)
        gV[..., :, 2] += np.cross(gy, n)
        gV[..., :, 1] = 0.0
    dots = np.einsum("...aj,...aq->...jq", V, gV)  # v_j . g_q
    with np.errstate(divide="ignore", invalid="ignore"):
        w = dots / (lam[..., None, :] - lam[..., :, None])
    eye = np.eye(3, dtype=bool)
    w = np.where(eye, gl[..., None, :] * np.ones((3, 1)), w)
    with np.errstate(invalid="ignore"):
        grad = np.einsum("...jq,...aj,...bq->...ab", w, V, V)
        wabs = np.abs(w).sum((-1, -2))
    valid = valid_rows(lengths, lam.shape[1])
    return np.where(valid[..., None, None], grad, 0.0), np.where(valid, wabs, 0.0)


# ------------------------------------------------------------------------------------------------ alignment
def moment_slots(D):
    """name -> slice into the 3 + 4D + D*D moments (PaSlot of csrc/small_solvers.h)."""
    return {"Sw": slice(0, 1), "Sw2": slice(1, 2), "Swx": slice(2, 2 + D), "Swy": slice(2 + D, 2 + 2 * D),
            "Sw2x": slice(2 + 2 * D, 2 + 3 * D), "Sw2y": slice(2 + 3 * D, 2 + 4 * D),
            "Sxy": slice(2 + 4 * D, 2 + 4 * D + D * D), "Sxx": slice(2 + 4 * D + D * D, 3 + 4 * D + D * D)}


def _clamped_lengths(lengths, N, P):
    return np.full(N, P, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, P)


def alignment_terms(X, Y, idx, lengths, weights, n):
    """Per-row terms of cloud n's moments, float64, (len, 3 + 4D + D*D): every product is of two or three fp32 values
    widened to float64 and of differences of two such values -- what the kernel forms before it sums."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    N, P, D = X.shape
    P2 = Y.shape[1]
    L = int(_clamped_lengths(lengths, N, P)[n])
    sl = moment_slots(D)
    t = np.zeros((L, 3 + 4 * D + D * D))
    if L == 0:
        return t
    j = np.arange(L) if idx is None else np.clip(np.asarray(idx)[n, :L], 0, P2 - 1)
    px = X[n, 0]
    py = Y[n, 0] if P2 > 0 else np.zeros(D)
    x = X[n, :L] - px
    y = (Y[n, j] if P2 > 0 else np.zeros((L, D))) - py
    w = np.ones(L) if weights is None else np.asarray(weights, np.float64)[n, :L]
    w2 = w * w
    t[:, sl["Sw"]] = w[:, None]
    t[:, sl["Sw2"]] = w2[:, None]
    t[:, sl["Swx"]] = w[:, None] * x
    t[:, sl["Swy"]] = w[:, None] * y
    t[:, sl["Sw2x"]] = w2[:, None] * x
    t[:, sl["Sw2y"]] = w2[:, None] * y
    t[:, sl["Sxy"]] = ((w2[:, None] * x)[:, :, None] * y[:, None, :]).reshape(L, D * D)
    t[:, sl["Sxx"]] = ((w2[:, None] * x) * x).sum(1, keepdims=True)
    return t


def alignment_moments_f64(X, Y, idx=None, lengths=None, weights=None):
    """-> (moments (N,M) float64, abs (N,M) float64 = sum of |terms|, rows (N,) = terms per cloud); the sums run in
    long double.  idx entries are clamped to [0, P2 - 1]; lengths to [0, P]; the pivots are row 0 of X and of Y (zero
    for a cloud without rows)."""
    N, P, D = np.asarray(X).shape
    M = 3 + 4 * D + D * D
    mom, mabs = np.zeros((N, M)), np.zeros((N, M))
    rows = _clamped_lengths(lengths, N, P)
    for n in range(N):
        t = alignment_terms(X, Y, idx, lengths, weights, n).astype(np.longdouble)
        mom[n] = t.sum(0).astype(np.float64)
        mabs[n] = np.abs(t).sum(0).astype(np.float64)
    return mom, mabs, rows


def alignment_backward_f64(X, Y, lengths, weights, grad_moments):
    """float64 closed form of alignment_backward_kernel (idx = None: Y has X's shape) -> grad_X, grad_Y (N,P,D),
    grad_w (N,P): with x, y about the pivots (held constant),
    grad_x = w g_Swx + w^2 (g_Sw2x + G_xy y + 2 g_Sxx x);  grad_y = w g_Swy + w^2 (g_Sw2y + G_xy^T x);
    grad_w = g_Sw + g_Swx.x + g_Swy.y + 2 w (g_Sw2 + g_Sw2x.x + g_Sw2y.y + x^T G_xy y + g_Sxx |x|^2).
    Rows i >= lengths[n] are zero."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    g = np.asarray(grad_moments, np.float64)
    N, P, D = X.shape
    sl = moment_slots(D)
    L = _clamped_lengths(lengths, N, P)
    valid = valid_rows(L, P)
    has = (L > 0)[:, None, None]
    x = X - np.where(has, X[:, :1], 0.0) if P > 0 else X
    y = Y - np.where(has, Y[:, :1], 0.0) if P > 0 else Y
    w = np.ones((N, P)) if weights is None else np.asarray(weights, np.float64)
    w2 = w * w
    G = g[:, sl["Sxy"]].reshape(N, D, D)
    Gy = np.einsum("nab,npb->npa", G, y)
    Gx = np.einsum("nba,npb->npa", G, x)
    gsxx = g[:, sl["Sxx"]][:, :, None]
    gX = w[..., None] * g[:, None, sl["Swx"]] + w2[..., None] * (g[:, None, sl["Sw2x"]] + Gy + 2.0 * gsxx * x)
    gY = w[..., None] * g[:, None, sl["Swy"]] + w2[..., None] * (g[:, None, sl["Sw2y"]] + Gx)
    gw1 = g[:, sl["Sw"]] + (g[:, None, sl["Swx"]] * x).sum(-1) + (g[:, None, sl["Swy"]] * y).sum(-1)
    gw2 = (g[:, sl["Sw2"]] + (g[:, None, sl["Sw2x"]] * x).sum(-1) + (g[:, None, sl["Sw2y"]] * y).sum(-1)
           + (x * Gy).sum(-1) + gsxx[..., 0] * (x * x).sum(-1))
    gw = gw1 + 2.0 * w * gw2
    return (np.where(valid[..., None], gX, 0.0), np.where(valid[..., None], gY, 0.0), np.where(valid, gw, 0.0))
