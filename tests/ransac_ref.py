"""Checker for ransac_alignment (functions/ransac.py): the definition in the comment of pointops_ransac_alignment
(include/pointops_amd.h) restated in numpy, independent of the package.

Draws and selection are integers.  Everything else takes `dtype`: np.float32 reproduces the kernels' operation order
(numpy's float32 arithmetic is IEEE and unfused, as the build's -ffp-contract=off makes the kernels'), np.float64 is the
reference.  The three-pair solve and the refits are always float64 (the kernels solve in fp64 and round once).

So that no threshold decision is ever compared across precisions, the GPU suite checks in stages: the samples against
`draw_samples`; the transforms against `solve_triples` on the device's samples; the validity flags and the counts
against `hypothesis_valid` / `counts` in float32 on the device's transforms; `best` against `select` on the device's
counts; the final mask against `evaluate` in float32 on the device's final transform.

rmse bound (`rmse_bound`).  The device evaluates e = ((x0 A0k + x1 A1k) + x2 A2k) + Tk - yk in fp32 with A = fl(s R);
u = 2^-24.  Per component: A carries u, each product u more (2u on S1 = sum_j |x_j A_jk| <= sqrt(3) s max|X|), the two
sums 2u on S1, adding T u on S1 + |T|, subtracting y u on S1 + |T| + |y|: |delta_k| <= 6u (S1 + |T_k| + |y_k|)
<= 6 sqrt(3) u B with B = s max|X| + max|T| + max|Y|, and |delta|_2 <= sqrt(3) times that = 18 u B.  The rmse is the
root mean square of |e| over the inliers, so the perturbation moves it by at most max |delta|_2 (triangle inequality of
the RMS norm).  Squaring and summing d2 in fp32 costs 3u relative on d2, 1.5u on its root, the final rounding u:
2.5u rmse, and rmse <= max |e|_2 <= sqrt(3) max|e_k| <= sqrt(3) (S1 + |T_k| + |y_k|) <= 3 B, so 7.5u B.  The fp64 sum
is exact at this scale.  Together 25.5u B:  |rmse - rmse64| <= 26 * 2^-24 * (1 + s max|X| + max|T| + max|Y|).
"""
import numpy as np

THR = 0.02
U32 = 2.0 ** -24
MASK32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ integers
def mix(x):
    """lowbias32 on uint32 values held in uint64 arrays."""
    x = np.asarray(x, np.uint64) & MASK32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & MASK32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & MASK32
    x ^= x >> np.uint64(16)
    return x


def hash32(seed, n, h, j):
    """hash32(seed, n, h, j), broadcasting over n, h, j (uint64 arrays of uint32 values)."""
    seed = int(seed)
    x = mix(np.uint64(((seed & 0xFFFFFFFF) + 0x9E3779B9) & 0xFFFFFFFF))
    x = mix(x ^ np.uint64((seed >> 32) & 0xFFFFFFFF))
    x = mix(x ^ (np.asarray(n, np.uint64) & MASK32))
    x = mix(x ^ (np.asarray(h, np.uint64) & MASK32))
    return mix(x ^ (np.asarray(j, np.uint64) & MASK32))


def mulhi(a, b):
    return (np.asarray(a, np.uint64) * np.uint64(b)) >> np.uint64(32)


def draw(seed, n_global, H, M):
    """(H,3) int64 positions into the valid rows of a cloud with M >= 3 of them."""
    h = np.arange(H, dtype=np.uint64)
    i0 = mulhi(hash32(seed, n_global, h, 0), M).astype(np.int64)
    i1 = mulhi(hash32(seed, n_global, h, 1), M - 1).astype(np.int64)
    i1 += i1 >= i0
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = mulhi(hash32(seed, n_global, h, 2), M - 2).astype(np.int64)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return np.stack([i0, i1, i2], 1)


def lengths_of(lengths, N, P):
    return np.full(N, P, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, P)


def targets(corr, len1, len2, N, P1):
    """(N,P1) int64: the matched row of Y of every valid row of X, -1 for the others."""
    rows = np.arange(P1, dtype=np.int64)[None, :]
    j = np.broadcast_to(rows, (N, P1)).copy() if corr is None else np.asarray(corr, np.int64).copy()
    ok = (rows < len1[:, None]) & (j >= 0) & (j < len2[:, None])
    j[~ok] = -1
    return j


def draw_samples(tgt, H, seed, first_cloud=0):
    """(N,H,3) int64 rows of X: the drawn triples, -1 for a cloud with fewer than three valid rows."""
    N = tgt.shape[0]
    out = np.full((N, H, 3), -1, np.int64)
    for n in range(N):
        v = np.nonzero(tgt[n] >= 0)[0]
        if len(v) >= 3:
            out[n] = v[draw(seed, first_cloud + n, H, len(v))]
    return out


def select(counts):
    """best (N,) int64 from counts (N,H): the largest count >= 0, the lowest index among equals, -1 when none."""
    counts = np.asarray(counts, np.int64)
    best = counts.argmax(1)  # (the first maximum)
    best[counts.max(1) < 0] = -1
    return best


# ------------------------------------------------------------------------------------------------ triples
def gather_triples(X, Y, tgt, samples):
    """x, y (N,H,3 pairs,3) and ok (N,H): the three rows are distinct valid correspondences."""
    N, H, _ = samples.shape
    P1 = X.shape[1]
    inside = (samples >= 0) & (samples < P1)
    rows = np.where(inside, samples, 0)
    n = np.arange(N)[:, None, None]
    j = np.where(inside, tgt[n, rows], -1)
    ok = (j >= 0).all(2) & (samples[..., 0] != samples[..., 1]) & (samples[..., 0] != samples[..., 2]) \
        & (samples[..., 1] != samples[..., 2])
    x = X[n, rows]
    y = Y[n, np.maximum(j, 0)] if Y.shape[1] else np.zeros_like(x)
    return x, y, ok


def edges_ok(x, y, ratio, dtype=np.float32):
    x, y = x.astype(dtype), y.astype(dtype)
    q = dtype(ratio) * dtype(ratio)
    ok = np.ones(x.shape[:-2], bool)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        dx, dy = x[..., a, :] - x[..., b, :], y[..., a, :] - y[..., b, :]
        lx = (dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1]) + dx[..., 2] * dx[..., 2]
        ly = (dy[..., 0] * dy[..., 0] + dy[..., 1] * dy[..., 1]) + dy[..., 2] * dy[..., 2]
        ok &= (lx >= q * ly) & (ly >= q * lx)
    return ok


def hypothesis_valid(x, y, ok, ratio, estimate_scale, dtype=np.float32):
    return ok & edges_ok(x, y, ratio, dtype) if (not estimate_scale and ratio > 0) else ok.copy()


def alignment(x, y, w=None, estimate_scale=False, eps=1e-9):
    """Float64 weighted alignment without reflection of x, y (..., P, 3), w (..., P) -> R, T, s, singular values."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = np.ones(x.shape[:-1]) if w is None else np.asarray(w, np.float64)
    W = np.maximum(w.sum(-1), eps)[..., None]
    xm, ym = (w[..., None] * x).sum(-2) / W, (w[..., None] * y).sum(-2) / W
    dx, dy = (x - xm[..., None, :]) * w[..., None], (y - ym[..., None, :]) * w[..., None]
    C = np.einsum("...pa,...pb->...ab", dx, dy) / W[..., None]
    U, S, Vh = np.linalg.svd(C)
    E = np.ones(S.shape)
    E[..., -1] = np.where(np.linalg.det(U @ Vh) < 0, -1.0, 1.0)
    R = (U * E[..., None, :]) @ Vh
    s = np.ones(S.shape[:-1])
    if estimate_scale:
        s = (E * S).sum(-1) / np.maximum((dx * dx).sum((-1, -2)) / W[..., 0], eps)
    T = ym - s[..., None] * np.einsum("...a,...ab->...b", xm, R)
    return R, T, s, S


def well_determined(S, rel=1e-3):
    return S[..., 1] >= rel * S[..., 0]


# ------------------------------------------------------------------------------------------------ residuals
def residual_d2(R, T, s, x, y, dtype=np.float32):
    """d2 of rows x, y (M,3) under transforms R (...,3,3), T (...,3), s (...) -> (..., M), in the kernels' order."""
    R, T, s = np.asarray(R, dtype), np.asarray(T, dtype), np.asarray(s, dtype)
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    A = (s[..., None, None] * R)[..., None, :, :]  # (..., 1, 3, 3)
    d2 = None
    e = []
    for k in range(3):
        r = ((x[:, 0] * A[..., 0, k] + x[:, 1] * A[..., 1, k]) + x[:, 2] * A[..., 2, k]) + T[..., None, k]
        e.append(r - y[:, k])
    d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    return d2


def counts(R, T, s, valid, X, Y, tgt, thr, dtype=np.float32, block=256):
    """(N,H) int32 counts of transforms R (N,H,3,3), T, s with flags valid (N,H): -1 where invalid."""
    N, H = valid.shape
    thr2 = dtype(thr) * dtype(thr)
    out = np.full((N, H), -1, np.int32)
    for n in range(N):
        v = np.nonzero(tgt[n] >= 0)[0]
        x, y = X[n, v], Y[n, tgt[n, v]] if len(v) else np.zeros((0, 3), np.float32)
        for a in range(0, H, block):
            d2 = residual_d2(R[n, a:a + block], T[n, a:a + block], s[n, a:a + block], x, y, dtype)
            out[n, a:a + block] = (d2 <= thr2).sum(1)
        out[n, ~valid[n]] = -1
    return out


def evaluate(R, T, s, X, Y, tgt, thr, dtype=np.float32):
    """One transform per cloud -> mask (N,P1) bool, count (N,) int64, rmse (N,) float64 (sum of d2 in float64)."""
    N, P1 = tgt.shape
    thr2 = dtype(thr) * dtype(thr)
    mask = np.zeros((N, P1), bool)
    rmse = np.zeros(N)
    for n in range(N):
        v = np.nonzero(tgt[n] >= 0)[0]
        if len(v) == 0:
            continue
        d2 = residual_d2(R[n], T[n], s[n], X[n, v], Y[n, tgt[n, v]], dtype)
        inl = d2 <= thr2
        mask[n, v[inl]] = True
        rmse[n] = np.sqrt(d2[inl].astype(np.float64).sum() / max(int(inl.sum()), 1))
    return mask, mask.sum(1).astype(np.int64), rmse


def rmse64(R, T, s, X, Y, tgt, mask):
    """rmse of the given mask under the given (fp32) transform, everything in float64."""
    out = np.zeros(len(mask))
    for n in range(len(mask)):
        v = np.nonzero(mask[n])[0]
        if len(v):
            d2 = residual_d2(R[n], T[n], s[n], X[n, v], Y[n, tgt[n, v]], np.float64)
            out[n] = np.sqrt(d2.sum() / len(v))
    return out


def rmse_bound(s, T, X, Y):
    """(N,) the absolute bound of the module docstring."""
    mx = np.abs(X).reshape(len(X), -1).max(1) if X.shape[1] else np.zeros(len(X))
    my = np.abs(Y).reshape(len(Y), -1).max(1) if Y.shape[1] else np.zeros(len(Y))
    return 26.0 * U32 * (1.0 + np.abs(s) * mx + np.abs(T).max(1) + my)


def fit_mask(X, Y, tgt, mask, estimate_scale):
    """Float64 alignment of every cloud weighted by its mask (rows outside weigh 0)."""
    N = len(mask)
    n = np.arange(N)[:, None]
    Yc = Y[n, np.maximum(tgt, 0)] if Y.shape[1] else np.zeros_like(X)
    return alignment(X, Yc, mask.astype(np.float64), estimate_scale)


def refine(R, T, s, best, X, Y, tgt, thr, refine_steps, estimate_scale, dtype=np.float32):
    """Steps 7-9 from the winners' transforms (N,...): evaluate, then refit / evaluate / accept.  Returns R, T, s (in
    `dtype`), mask, count, rmse and the number of accepted refits per cloud."""
    N = len(best)
    R, T, s = np.array(R, dtype), np.array(T, dtype), np.array(s, dtype)
    none = best < 0
    R[none], T[none], s[none] = np.eye(3, dtype=dtype), 0, 1
    mask, cnt, rmse = evaluate(R, T, s, X, Y, tgt, thr, dtype)
    mask[none], cnt[none], rmse[none] = False, 0, 0.0
    stopped = none.copy()
    accepted = np.zeros(N, np.int64)
    for _ in range(refine_steps):
        Rc, Tc, sc, _ = fit_mask(X, Y, tgt, mask, estimate_scale)
        Rc, Tc, sc = Rc.astype(np.float32).astype(dtype), Tc.astype(np.float32).astype(dtype), \
            sc.astype(np.float32).astype(dtype)  # (the kernels round the fit to fp32 once)
        mc, cc, rc = evaluate(Rc, Tc, sc, X, Y, tgt, thr, dtype)
        ok = ~stopped & (cc >= cnt)
        stopped |= ~ok
        R[ok], T[ok], s[ok], mask[ok], cnt[ok], rmse[ok] = Rc[ok], Tc[ok], sc[ok], mc[ok], cc[ok], rc[ok]
        accepted += ok
    return R, T, s, mask, cnt, rmse, accepted


def run(X, Y, corr=None, len1=None, len2=None, *, thr=THR, H=256, estimate_scale=False, ratio=0.9, refine_steps=2,
        seed=0, samples=None, first_cloud=0, dtype=np.float64):
    """The whole definition; a dict of every stage."""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    N, P1, P2 = X.shape[0], X.shape[1], Y.shape[1]
    len1, len2 = lengths_of(len1, N, P1), lengths_of(len2, N, P2)
    tgt = targets(corr, len1, len2, N, P1)
    samples = draw_samples(tgt, H, seed, first_cloud) if samples is None else np.asarray(samples, np.int64)
    x, y, ok = gather_triples(X, Y, tgt, samples)
    valid = hypothesis_valid(x, y, ok, ratio, estimate_scale, dtype)
    hR, hT, hs, S = alignment(x, y, None, estimate_scale)
    hR[~valid], hT[~valid], hs[~valid] = np.eye(3), 0.0, 1.0
    h32 = [a.astype(np.float32) for a in (hR, hT, hs)]  # (one rounding, as the kernels')
    cnt = counts(*h32, valid, X, Y, tgt, thr, dtype)
    best = select(cnt)
    n = np.arange(N)
    b = np.maximum(best, 0)
    R, T, s, mask, num, rmse, accepted = refine(h32[0][n, b], h32[1][n, b], h32[2][n, b], best, X, Y, tgt, thr,
                                                refine_steps, estimate_scale, dtype)
    return dict(tgt=tgt, samples=samples, valid=valid, hyp=(hR, hT, hs), sing=S, counts=cnt, best=best, R=R, T=T, s=s,
                mask=mask, num_inliers=num, rmse=rmse, accepted=accepted)


# ------------------------------------------------------------------------------------------------ scenes
def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def scene(seed, P1, inlier_ratio, N=1, P2=None, thr=THR, lengths=False, scale=1.0):
    """One seeded scene: X uniform in the unit cube; Y = scale X R0 + T0 plus noise of norm <= 0.2 thr on a planted
    inlier set; every other valid row is matched to a uniform point of a cube twice as large; a few rows carry -1 and a
    few an index >= len2.  corr is a permutation of the rows of Y, so Y has P2 >= P1 rows.  Returns a dict with X, Y,
    corr, len1, len2 (None unless `lengths`), planted (N,P1) bool, R0 (N,3,3), T0 (N,3), scale."""
    rng = np.random.default_rng(9100 + seed)
    P2 = P1 + 7 if P2 is None else P2
    X = rng.uniform(0, 1, (N, P1, 3)).astype(np.float32)
    Y = (rng.uniform(-0.5, 1.5, (N, P2, 3)) * scale).astype(np.float32)
    corr = np.stack([rng.permutation(P2)[:P1] for _ in range(N)]).astype(np.int64)
    len1 = np.full(N, P1, np.int64)
    len2 = np.full(N, P2, np.int64)
    if lengths:
        len1 = np.maximum(P1 - rng.integers(0, max(P1 // 4, 1), N), min(P1, 3)).astype(np.int64)
        len2 = np.full(N, P2 - 3, np.int64)
    R0 = np.stack([rotation(rng) for _ in range(N)])
    T0 = rng.uniform(-1, 1, (N, 3))
    planted = np.zeros((N, P1), bool)
    for n in range(N):
        bad = rng.permutation(P1)[:max(P1 // 50, 2)]
        corr[n, bad[::2]] = -1
        corr[n, bad[1::2]] = P2 + 5  # (>= len2)
        ok = (np.arange(P1) < len1[n]) & (corr[n] >= 0) & (corr[n] < len2[n])
        v = np.nonzero(ok)[0]
        k = max(int(round(inlier_ratio * len(v))), min(3, len(v)))
        chosen = v[rng.permutation(len(v))[:k]]
        planted[n, chosen] = True
        noise = rng.standard_normal((k, 3))
        noise *= (0.2 * thr * rng.uniform(0, 1, (k, 1))) / np.linalg.norm(noise, axis=1, keepdims=True)
        Y[n, corr[n, chosen]] = (scale * (X[n, chosen].astype(np.float64) @ R0[n]) + T0[n] + noise).astype(np.float32)
        others = v[~planted[n, v]]  # an accidental near match moves out of reach (corr is injective: nobody else's)
        truth = scale * (X[n, others].astype(np.float64) @ R0[n]) + T0[n]
        near = np.linalg.norm(truth - Y[n, corr[n, others]], axis=1) < 5.0 * thr
        Y[n, corr[n, others[near]]] += np.float32(1.0)
    return dict(X=X, Y=Y, corr=corr, len1=len1 if lengths else None, len2=len2 if lengths else None, planted=planted,
                R0=R0, T0=T0, scale=scale)


def scene_margins(sc, thr=THR):
    """(largest planted distance, smallest other valid distance) under (R0, T0, scale), in units of thr."""
    X, Y = sc["X"].astype(np.float64), sc["Y"].astype(np.float64)
    N, P1 = X.shape[:2]
    tgt = targets(sc["corr"], lengths_of(sc["len1"], N, P1), lengths_of(sc["len2"], N, Y.shape[1]), N, P1)
    worst_in, best_out = 0.0, np.inf
    for n in range(N):
        v = np.nonzero(tgt[n] >= 0)[0]
        d = np.linalg.norm(sc["scale"] * (X[n, v] @ sc["R0"][n]) + sc["T0"][n] - Y[n, tgt[n, v]], axis=1)
        p = sc["planted"][n, v]
        worst_in = max(worst_in, d[p].max() if p.any() else 0.0)
        best_out = min(best_out, d[~p].min() if (~p).any() else np.inf)
    return worst_in / thr, best_out / thr


# ------------------------------------------------------------------------------------------------ the GPU suite's scenes
CHUNK = 256  # records per scoring workgroup (test_ransac_cpu.py holds it to _C_ransac.RANSAC_CHUNK)

# name -> scene() arguments, plus the run's H / estimate_scale / ratio / refine_steps; planted=False: too few
# hypotheses to promise the planted set, the stages are still compared
SCENES = {
    "p255": dict(seed=1, P1=255, inlier_ratio=0.5, H=256, refine_steps=0),
    "p256": dict(seed=2, P1=256, inlier_ratio=0.5, H=256, refine_steps=1),
    "p257": dict(seed=3, P1=257, inlier_ratio=0.5, H=256, refine_steps=3),
    "p1000": dict(seed=4, P1=1000, inlier_ratio=0.3, H=1024, N=3, lengths=True),
    "scale": dict(seed=5, P1=300, inlier_ratio=0.3, H=1024, scale=1.7, estimate_scale=True),
    "noedge": dict(seed=6, P1=300, inlier_ratio=0.5, H=256, ratio=0.0),
    "chunk-1": dict(seed=7, P1=CHUNK + 4, inlier_ratio=0.5, H=256),       # P1 // 50 = 5 rows carry no match
    "chunk": dict(seed=8, P1=CHUNK + 5, inlier_ratio=0.5, H=256),
    "chunk+1": dict(seed=9, P1=CHUNK + 6, inlier_ratio=0.5, H=256),
    "2chunk+1": dict(seed=10, P1=2 * CHUNK + 11, inlier_ratio=0.5, H=256),  # 10 rows
    "medium": dict(seed=11, P1=5000, inlier_ratio=0.2, H=1024, N=2),
    "p2047": dict(seed=16, P1=2047, inlier_ratio=0.4, H=256),  # the compaction walks 2048 rows per step
    "p2048": dict(seed=17, P1=2048, inlier_ratio=0.4, H=256),
    "p2049": dict(seed=18, P1=2049, inlier_ratio=0.4, H=256),
    # three tiles: the third (row 4096 alone, a valid pair) adds the counts of two; 81 rows without a match in those
    "p4097": dict(seed=40, P1=4097, inlier_ratio=0.4, H=256),
    # 33 tiles, and the first P1 at which the evaluation's 32 blocks walk their rows twice
    "p65537": dict(seed=60, P1=65537, inlier_ratio=0.5, H=64, refine_steps=1),
    "h1": dict(seed=12, P1=300, inlier_ratio=0.5, H=1, planted=False),
    "h63": dict(seed=13, P1=300, inlier_ratio=0.5, H=63, planted=False),
    "h64": dict(seed=14, P1=300, inlier_ratio=0.5, H=64, planted=False),
    "h65": dict(seed=15, P1=300, inlier_ratio=0.5, H=65, planted=False),
}


def make_scene(name):
    """(scene dict, keyword arguments of run() / of ransac_alignment's checker)."""
    a = dict(SCENES[name])
    a.pop("planted", None)
    kw = dict(H=a.pop("H"), estimate_scale=a.pop("estimate_scale", False), ratio=a.pop("ratio", 0.9),
              refine_steps=a.pop("refine_steps", 2), seed=100 + a["seed"], thr=THR)
    return scene(**a), kw


def rejected_refit_scene():
    """(X, Y, samples, thr): three exact pairs (the only triple), five pairs 0.8 thr off along +x and one 0.8 thr off
    along -x.  The winner (the identity) holds all nine; the least-squares refit moves about 0.36 thr towards the five
    and loses the one, so it is rejected."""
    thr = 0.05
    rng = np.random.default_rng(9300)
    X = rng.uniform(0, 1, (1, 9, 3)).astype(np.float32)
    X[0, 8] = X[0, :8].mean(0)  # the one sits at the centroid, where the refit's rotation cannot reach it
    Y = X.copy()
    Y[0, 3:8, 0] += np.float32(0.8 * thr)
    Y[0, 8, 0] -= np.float32(0.8 * thr)
    return X, Y, np.array([[[0, 1, 2]]], np.int64), thr
