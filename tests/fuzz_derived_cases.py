"""The cases of the randomised soak of the derived operators (tests/test_fuzz_derived_gpu.py), certified without a GPU by
tests/test_fuzz_derived_cpu.py.  numpy and the checkers' scene builders only: nothing of the package is imported.

One function per operator family returns the list of cases of a seed; a case is a namespace whose `what` is the dict that
reproduces it (family, seed, index, shape, lengths, kind, parameters) and is what a failing assertion prints.

POINTOPS_FUZZ_SOAK=<int> shifts every seed, as in tests/test_fuzz_small_gpu.py:
`for s in 1000 2000 ...; do POINTOPS_FUZZ_SOAK=$s pytest tests/test_fuzz_derived_gpu.py; done` draws fresh cases; offset 0
is what the suite pins and what the CPU file certifies.

Shapes.  N clouds of P rows; P is random or one of P_EDGES, every length random in 0..P or one of L_EDGES (the ends of a
64-lane wave, a 256-thread block, the 512-point grid threshold, the 1024-wide scan); one cloud is full, one is empty in
about a quarter of the cases.  Rows at or past a cloud's length hold PAD, which nothing may read."""
import math
import os
from types import SimpleNamespace

import numpy as np

import plane_ref
import ransac_ref
import registration_ref

SOAK = int(os.environ.get("POINTOPS_FUZZ_SOAK", "0"))
SEEDS = (1, 2, 3)
PAD = np.float32(9.0)
P_MAX = 1400
P_EDGES = (64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
L_EDGES = (1, 2, 63) + P_EDGES
KINDS = ("uniform", "blobs", "lattice")
STEP = 0.125  # the lattice: exact in float32, and so are its squared distances
LATTICE_RADII = (0.125, 0.126, 0.18, 0.25)  # 0.125 and 0.25 put pairs at exactly d2 == r2
NEIGHBOURS = (1.5, 4.0, 10.0)
MIN_POINTS = (1, 2, 3, 5, 8)
VOXEL_MEMBERS = (0.5, 4.0, 40.0)
CHANNELS = (None, 1, 3, 33)
VALID_EDGES = (3, 255, 256, 257, 511, 512, 513)  # valid rows of a consensus cloud: the scoring chunks of 256 and 512
HYPOTHESES = (1, 2, 64, 255, 256, 257, 600)
STAT_EDGES = (1, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 9000)  # the summation tree's chunks of 4096 rows
STAT_K1 = (2, 3, 17, 128)
DENSITIES = (0.0, 0.01, 0.5, 0.99, 1.0)
REG_EDGES = (511, 512, 513, 2047, 2048, 2049)  # the search's grid threshold, the block of 2048 partials

RADIUS_CASES, VOXEL_CASES, CONSENSUS_CASES, STAT_CASES, COMPACT_CASES, REG_CASES = 20, 20, 14, 8, 8, 10


def _rng(family, seed):
    return np.random.default_rng(1000 * family + seed + SOAK)


def shape(rng, n_max=6, p_max=P_MAX, p_edges=P_EDGES, l_edges=L_EDGES, p_min=1):
    """(N, P, lengths (N,) int64) by the rule of the module docstring."""
    N = int(rng.integers(1, n_max + 1))
    P = int(rng.choice(p_edges)) if rng.random() < 0.5 else int(rng.integers(p_min, p_max + 1))
    fit = [e for e in l_edges if e <= P]
    L = np.array([int(rng.choice(fit)) if rng.random() < 0.5 else int(rng.integers(0, P + 1)) for _ in range(N)], np.int64)
    full = int(rng.integers(0, N))
    L[full] = P
    if N > 1 and rng.random() < 0.3:
        L[(full + 1 + int(rng.integers(0, N - 1))) % N] = 0
    return N, P, L


def cloud(rng, kind, P, D):
    """(P, D) float32 in the unit cube: uniform, blobs over a uniform background, or a lattice with repeated points."""
    if kind == "uniform":
        return rng.random((P, D), dtype=np.float32)
    if kind == "blobs":
        k = int(rng.integers(2, 7))
        centres = rng.uniform(0.1, 0.9, (k, D))
        p = centres[rng.integers(0, k, P)] + rng.normal(0.0, 0.03, (P, D))
        background = rng.random(P) < 0.3
        p[background] = rng.uniform(0.0, 1.0, (int(background.sum()), D))
        return p.astype(np.float32)
    side = int(rng.choice([3, 6, 9]))
    return (rng.integers(0, side, (P, D)) * STEP).astype(np.float32)


def padded(rng, kind, N, P, D, lengths):
    pts = np.stack([cloud(rng, kind, P, D) for _ in range(N)])
    pts[np.arange(P)[None, :] >= lengths[:, None]] = PAD
    return pts


def radius_for(m, P, D):
    """The radius whose ball holds `m` of P uniform points of the unit cube."""
    return {1: m / (2.0 * P), 2: math.sqrt(m / (math.pi * P)), 3: (3.0 * m / (4.0 * math.pi * P)) ** (1.0 / 3.0)}[D]


def radius_family_cases(seed):
    """cluster_dbscan, remove_radius_outlier (min_neighbors = min_points) and, for D = 3, iss_keypoints (rs = radius):
    points (N, P, D), lengths, radius, min_points, rn."""
    rng = _rng(1, seed)
    out = []
    for i in range(RADIUS_CASES):
        N, P, L = shape(rng)
        D = int(rng.choice([1, 2, 3, 3]))
        kind = KINDS[int(rng.integers(0, 3))]
        pts = padded(rng, kind, N, P, D, L)
        m = float(rng.choice(NEIGHBOURS))
        radius = float(rng.choice(LATTICE_RADII)) if kind == "lattice" else float(np.float32(radius_for(m, P, D)))
        mp = int(rng.choice(MIN_POINTS))
        rn = float(np.float32(radius * float(rng.choice([0.6, 1.5]))))
        what = dict(family="radius", seed=seed, index=i, soak=SOAK, N=N, P=P, D=D, lengths=L.tolist(), kind=kind,
                    radius=radius, min_points=mp, rn=rn)
        out.append(SimpleNamespace(what=what, points=pts, lengths=L, radius=radius, min_points=mp, rn=rn, D=D, kind=kind))
    return out


def voxel_cases(seed):
    """voxel_downsample: points (N, P, 3), lengths, voxel size, features (N, P, C) or None, origin None / (3,) / (N, 3).
    A lattice lies on multiples of STEP with an origin on them and a voxel of STEP or 2 STEP: points exactly on faces."""
    rng = _rng(2, seed)
    out = []
    for i in range(VOXEL_CASES):
        N, P, L = shape(rng)
        kind = KINDS[int(rng.integers(0, 3))]
        pts = padded(rng, kind, N, P, 3, L)
        C = CHANNELS[int(rng.integers(0, 4))]
        feats = None
        if C is not None:
            feats = rng.normal(size=(N, P, C)).astype(np.float32)
            feats[np.arange(P)[None, :] >= L[:, None]] = PAD
        how = ("none", "one", "per-cloud")[int(rng.integers(1 if kind == "lattice" else 0, 3))]
        m = float(rng.choice(VOXEL_MEMBERS))
        if kind == "lattice":
            v = float(rng.choice([STEP, 2 * STEP]))
            draw = lambda shp: (rng.integers(-3, 4, shp) * STEP).astype(np.float32)  # noqa: E731
        else:
            v = float(np.float32((m / P) ** (1.0 / 3.0)))
            draw = lambda shp: rng.uniform(-0.5, 0.7, shp).astype(np.float32)  # noqa: E731
        origin = None if how == "none" else draw((3,) if how == "one" else (N, 3))
        what = dict(family="voxel", seed=seed, index=i, soak=SOAK, N=N, P=P, lengths=L.tolist(), kind=kind, voxel_size=v,
                    C=C, origin=None if origin is None else origin.tolist())
        out.append(SimpleNamespace(what=what, points=pts, lengths=L, voxel_size=v, features=feats, origin=origin, kind=kind))
    return out


def _consensus_shape(rng, seed, i):
    """(N, P, H, snap): each operator walks the hypothesis counts once per seed, and the valid-row edges once over two
    consecutive seeds (half of the cases are snapped)."""
    N = int(rng.integers(1, 5))
    j, s = i // 2, seed + SOAK
    H = HYPOTHESES[(j + 3 * s) % 7]
    snap = VALID_EDGES[j % 7] if (j + s) % 2 == 0 else None
    P = int(rng.integers((snap or 0) + 45, P_MAX + 1)) if rng.random() < 0.8 else int(rng.choice([2047, 2048, 2049]))
    return N, P, H, snap


def _lengths(rng, N, P):
    L = rng.integers(0, P + 1, N).astype(np.int64)
    L[int(rng.integers(0, N))] = P
    return L


def _snap(rng, valid, M):
    """`valid` (P,) bool with all but M of its set rows cleared (scattered)."""
    rows = np.flatnonzero(valid)
    keep = np.zeros_like(valid)
    keep[rng.permutation(rows)[:M]] = True
    return keep


def _plane_case(rng, seed, i):
    N, P, H, snap = _consensus_shape(rng, seed, i)
    sc = plane_ref.scene(int(rng.integers(0, 10 ** 6)), P, float(rng.choice([0.3, 0.5, 0.8])), N=N)
    X = sc["X"].copy()
    L = _lengths(rng, N, P)
    mask = rng.random((N, P)) < float(rng.choice([0.3, 0.9, 1.0]))
    if snap is not None:  # the full cloud carries the snapped count
        n = int(np.argmax(L))
        mask[n] = _snap(rng, np.ones(P, bool), snap)
    if rng.random() < 0.5:  # repeated rows: triples with a coincident pair are degenerate
        dup = rng.random((N, P)) < 0.3
        src = rng.integers(0, P, (N, P))
        X = np.where(dup[..., None], X[np.arange(N)[:, None], src], X)
    X[np.arange(P)[None, :] >= L[:, None]] = PAD
    kw = dict(thr=plane_ref.THR, H=H, refine_steps=int(rng.integers(0, 3)), seed=int(rng.integers(0, 2 ** 40)))
    what = dict(family="plane", seed=seed, index=i, soak=SOAK, N=N, P=P, lengths=L.tolist(), snap=snap,
                valid=(mask & (np.arange(P)[None, :] < L[:, None])).sum(1).tolist(), kw=kw)
    return SimpleNamespace(what=what, op="plane", X=X, lengths=L, mask=mask, kw=kw)


def _well_determined_enough(X, Y, corr, len1, len2, kw):
    """What test_ransac_gpu.check_stages takes for granted of its scenes from 100 hypotheses on: at most 1% of the valid
    hypotheses have a nearly collinear triple (their float64 solve is not comparable)."""
    if kw["H"] < 100:
        return True
    N, P1 = X.shape[:2]
    tgt = ransac_ref.targets(corr, ransac_ref.lengths_of(len1, N, P1), ransac_ref.lengths_of(len2, N, Y.shape[1]), N, P1)
    x, y, ok = ransac_ref.gather_triples(X, Y, tgt, ransac_ref.draw_samples(tgt, kw["H"], kw["seed"]))
    valid = ransac_ref.hypothesis_valid(x, y, ok, kw["ratio"], kw["estimate_scale"], np.float32)
    S = ransac_ref.alignment(x, y, None, kw["estimate_scale"])[3]
    return bool((valid & ~ransac_ref.well_determined(S)).sum() <= 0.01 * max(valid.sum(), 1))


def _ransac_case(rng, seed, i):
    N, P1, H, snap = _consensus_shape(rng, seed, i)
    while True:
        sc = ransac_ref.scene(int(rng.integers(0, 10 ** 6)), P1, float(rng.choice([0.3, 0.5, 0.8])), N=N)
        X, Y, corr = sc["X"].copy(), sc["Y"].copy(), sc["corr"].copy()
        P2 = Y.shape[1]
        len1 = _lengths(rng, N, P1)
        len2 = np.where(rng.random(N) < 0.7, P2, rng.integers(0, P2 + 1, N)).astype(np.int64)
        holes = rng.random((N, P1)) < float(rng.choice([0.0, 0.1, 0.6]))
        if snap is not None:  # the full cloud carries the snapped count: the scene's own holes leave it enough rows
            n = int(np.argmax(len1))
            holes[n], len2[n] = False, P2
        corr[holes] = -1
        if snap is not None:
            ok = (corr[n] >= 0) & (corr[n] < P2)
            corr[n, ok & ~_snap(rng, ok, snap)] = -1
        X[np.arange(P1)[None, :] >= len1[:, None]] = PAD
        Y[np.arange(P2)[None, :] >= len2[:, None]] = PAD
        kw = dict(thr=ransac_ref.THR, H=H, estimate_scale=bool(rng.random() < 0.3), ratio=float(rng.choice([0.9, 0.9, 0.0])),
                  refine_steps=int(rng.integers(0, 3)), seed=int(rng.integers(0, 2 ** 40)))
        if _well_determined_enough(X, Y, corr, len1, len2, kw):
            break
    tgt = ransac_ref.targets(corr, len1, len2, N, P1)
    what = dict(family="ransac", seed=seed, index=i, soak=SOAK, N=N, P1=P1, P2=P2, len1=len1.tolist(), len2=len2.tolist(),
                snap=snap, valid=(tgt >= 0).sum(1).tolist(), kw=kw)
    return SimpleNamespace(what=what, op="ransac", X=X, Y=Y, corr=corr, len1=len1, len2=len2, kw=kw)


def consensus_cases(seed):
    """segment_plane (even indices) and ransac_alignment (odd) on the scenes of plane_ref / ransac_ref under random
    lengths, masks and holes in `corr`."""
    rng = _rng(3, seed)
    return [(_plane_case if i % 2 == 0 else _ransac_case)(rng, seed, i) for i in range(CONSENSUS_CASES)]


def _stat_shape(rng, seed, i):
    """(N, P, lengths): three cases of four take P from STAT_EDGES in turn (two consecutive seeds meet every edge), the
    fourth a random P; the lengths are edges that fit, or random."""
    pick = lambda: int(rng.choice(STAT_EDGES)) if rng.random() < 0.6 else int(rng.integers(1, 9001))  # noqa: E731
    N = int(rng.integers(1, 6))
    P = int(rng.integers(1, 9001)) if i % 4 == 3 else STAT_EDGES[((seed + SOAK) * 6 + i - i // 4) % len(STAT_EDGES)]
    L = np.array([min(pick(), P) if rng.random() < 0.7 else int(rng.integers(0, P + 1)) for _ in range(N)], np.int64)
    L[int(rng.integers(0, N))] = P
    return N, P, L


def statistical_cases(seed):
    """The statistical filter's boundary on synthetic tables: dists (N, P, K1) float32 >= 0 with column 0 zero."""
    rng = _rng(4, seed)
    out = []
    for i in range(STAT_CASES):
        N, P, L = _stat_shape(rng, seed, i)
        K1 = int(rng.choice(STAT_K1))
        dists = (rng.random((N, P, K1), dtype=np.float32) * np.float32(rng.choice([1e-4, 1.0, 100.0]))).astype(np.float32)
        dists[..., 0] = 0.0
        dists[np.arange(P)[None, :] >= L[:, None]] = PAD
        ratio = float(rng.choice([0.0, 0.5, 1.0, 2.0]))
        what = dict(family="statistical", seed=seed, index=i, soak=SOAK, N=N, P=P, K1=K1, lengths=L.tolist(), std_ratio=ratio)
        out.append(SimpleNamespace(what=what, dists=dists, lengths=L, std_ratio=ratio))
    return out


def compact_cases(seed):
    """mask_compact: masks (N, P) bool, every cloud at a density of DENSITIES."""
    rng = _rng(5, seed)
    out = []
    for i in range(COMPACT_CASES):
        N, P, _ = _stat_shape(rng, seed, i)
        dens = [float(rng.choice(DENSITIES)) for _ in range(N)]
        mask = np.stack([rng.random(P) < d for d in dens])
        what = dict(family="compact", seed=seed, index=i, soak=SOAK, N=N, P=P, densities=dens)
        out.append(SimpleNamespace(what=what, mask=mask))
    return out


def registration_cases(seed):
    """One evaluate-only step of registration_icp: N clouds of registration_ref.scene with ragged (P1, P2), padded with
    PAD to the largest; the sizes are random or snapped around REG_EDGES."""
    rng = _rng(6, seed)
    pick = lambda lo: int(rng.choice([e for e in REG_EDGES if e >= lo])) if rng.random() < 0.6 \
        else int(rng.integers(lo, 2101))  # noqa: E731
    out = []
    for i in range(REG_CASES):
        N = int(rng.integers(1, 5))
        clutter = bool(rng.random() < 0.5)
        sizes = []
        for _ in range(N):
            a = pick(8)
            sizes.append((a, pick(a - a // 4 if clutter else a)))  # (the scene's overlap rows are rows of the target)
        scene_seed = int(rng.integers(0, 10 ** 6))
        scenes = [registration_ref.scene(scene_seed + n, a, b, clutter) for n, (a, b) in enumerate(sizes)]
        P1, P2 = max(a for a, _ in sizes), max(b for _, b in sizes)
        X, Y, Nr = (np.full((N, P, 3), PAD, np.float32) for P in (P1, P2, P2))
        for n, sc in enumerate(scenes):
            X[n, :len(sc.X)], Y[n, :len(sc.Y)], Nr[n, :len(sc.Y)] = sc.X, sc.Y, sc.normals
        estimation = ("point_to_plane", "point_to_point")[int(rng.integers(0, 2))]
        what = dict(family="registration", seed=seed, index=i, soak=SOAK, N=N, sizes=sizes, clutter=clutter,
                    scene_seed=scene_seed, estimation=estimation, r_max=registration_ref.R_MAX)
        out.append(SimpleNamespace(what=what, X=X, Y=Y, normals=Nr, len_x=np.array([a for a, _ in sizes], np.int64),
                                   len_y=np.array([b for _, b in sizes], np.int64), estimation=estimation,
                                   r_max=registration_ref.R_MAX))
    return out
