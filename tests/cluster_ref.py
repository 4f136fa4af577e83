"""Checker for cluster_dbscan (functions/cluster.py): the definition in the comment of pointops_cluster_dbscan
(include/pointops_amd.h) restated in numpy, independent of the package.  numpy alone is enough; scipy's
connected_components is used for the components when it is importable (`components_numpy` is the same thing without it,
and tests/test_cluster_cpu.py holds the two to each other).

    r2 = fl32(eps * eps);  d2(i, j) = (dx*dx + dy*dy) + dz*dz in float32, unfused (numpy's float32 arithmetic is IEEE and
    unfused, as the build's -ffp-contract=off makes the kernels');  neighbours iff d2 < r2
    core: at least min_points neighbours, itself included
    clusters: connected components of the neighbour graph on the core points, numbered by their smallest member
    border: a non-core point takes the smallest label among its core neighbours;  everything else, padding included: -1

Everything is integers and booleans: results are compared for equality, never within a tolerance.
"""
import numpy as np

try:  # optional
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:  # pragma: no cover
    connected_components = None

BLOCK = 1024  # rows of the P x P comparison formed at a time


def neighbours(p, eps):
    """(P, P) bool: d2(i, j) < r2 for the (P, D) float32 points of one cloud."""
    p = np.ascontiguousarray(p, np.float32)
    P, D = p.shape
    r2 = np.float32(eps) * np.float32(eps)
    adj = np.zeros((P, P), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, P, BLOCK):
            q = p[a:a + BLOCK]
            dx = q[:, None, 0] - p[None, :, 0]
            d = dx * dx
            for k in range(1, D):
                dk = q[:, None, k] - p[None, :, k]
                d = d + dk * dk
            adj[a:a + BLOCK] = d < r2
    return adj


def components_numpy(n, u, v):
    """(n,) int64: the smallest index of every node's component in the graph with edges (u[k], v[k]).  Min-label
    hooking with pointer jumping until nothing moves.  At the fixed point both ends of every edge carry one label, a label
    never exceeds its node's index and always names a node of the same component: it is the component's smallest index."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, u, lab[v])
        np.minimum.at(new, v, lab[u])
        new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


def components(n, u, v):
    if connected_components is None:
        return components_numpy(n, u, v)
    g = csr_matrix((np.ones(len(u), np.int8), (u, v)), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    first = np.full(comp.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(first, comp, np.arange(n, dtype=np.int64))
    return first[comp]


def dbscan_cloud(p, eps, min_points, use_scipy=True):
    """(labels (P,) int64, core (P,) bool, number of clusters) of one cloud of (P, D) float32 points."""
    P = p.shape[0]
    if P == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool), 0
    adj = neighbours(p, eps)
    core = adj.sum(1) >= min_points
    cadj = adj & core[:, None] & core[None, :]
    u, v = np.nonzero(np.triu(cadj, 1))
    root = (components if use_scipy else components_numpy)(P, u, v)  # the smallest member of a core point's cluster
    roots = np.unique(root[core])
    labels = np.full(P, -1, np.int64)
    labels[core] = np.searchsorted(roots, root[core])
    big = np.iinfo(np.int64).max
    for a in range(0, P, BLOCK):  # border points: the smallest label among the core neighbours
        rows = np.where(adj[a:a + BLOCK] & core[None, :], labels[None, :], big).min(1)
        take = ~core[a:a + BLOCK] & (rows != big)
        labels[a:a + BLOCK][take] = rows[take]
    return labels, core, int(len(roots))


def dbscan(points, lengths, eps, min_points):
    """(labels (N, P) int64, num_clusters (N,) int64, core_mask (N, P) bool) of a padded batch (N, P, D)."""
    points = np.asarray(points, np.float32)
    N, P = points.shape[:2]
    lengths = np.full(N, P, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, P)
    labels = np.full((N, P), -1, np.int64)
    core = np.zeros((N, P), bool)
    num = np.zeros(N, np.int64)
    for n in range(N):
        L = int(lengths[n])
        labels[n, :L], core[n, :L], num[n] = dbscan_cloud(points[n, :L], eps, min_points)
    return labels, num, core


# ------------------------------------------------------------------------------------------------ scenes
def random_scenes(count=40):
    """The scenes of the scikit-learn comparison: (points float64 (P, 3), eps, min_points) for seeds 0..count-1 of one
    generator."""
    rng = np.random.default_rng(0)
    out = []
    for _ in range(count):
        P = int(rng.integers(50, 700))
        k = int(rng.integers(1, 8))
        c = rng.uniform(-1, 1, (k, 3))
        p = c[rng.integers(0, k, P)] + rng.normal(0, 0.08, (P, 3))
        p[:P // 5] = rng.uniform(-1, 1, (P // 5, 3))
        eps = float(rng.choice([0.05, 0.08, 0.12]))
        min_points = int(rng.choice([1, 2, 4, 8]))
        out.append((p, eps, min_points))
    return out


def bridge_scene():
    """Two dense blobs -- rows 1..19 within 0.01 of (-0.1, 0, 0) with their outpost row 0 at the origin, rows 21..39
    within 0.01 of (0.4, 0, 0) with their outpost row 20 at (0.3, 0, 0) -- and row 40 at (0.15, 0, 0): with eps = 0.16 it
    is within eps of the two outposts only (0.15; the blobs proper are 0.24 away, the outposts 0.3 from each other), so
    it has 3 neighbours < min_points = 5 and is a border point of both clusters.  Two clusters; row 40 takes label 0.
    -> (points (41, 3) float32, eps, min_points)"""
    rng = np.random.default_rng(7)
    a = rng.uniform(-0.01, 0.01, (20, 3)) + np.array([-0.1, 0.0, 0.0])
    b = rng.uniform(-0.01, 0.01, (20, 3)) + np.array([0.4, 0.0, 0.0])
    a[0] = (0.0, 0.0, 0.0)
    b[0] = (0.3, 0.0, 0.0)
    p = np.concatenate([a, b, np.array([[0.15, 0.0, 0.0]])]).astype(np.float32)
    return p, 0.16, 5


def blobs_scene(seed, P, k=6, sigma=0.03, background=0.25, duplicates=0):
    """(P, 3) float32: k Gaussian blobs in the unit cube over a uniform background; `duplicates` rows repeat others."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.1, 0.9, (k, 3))
    p = c[rng.integers(0, k, P)] + rng.normal(0, sigma, (P, 3))
    nb = int(P * background)
    p[:nb] = rng.uniform(0, 1, (nb, 3))
    p = p[rng.permutation(P)]
    if duplicates:
        src = rng.integers(0, P, duplicates)
        dst = rng.integers(0, P, duplicates)
        p[dst] = p[src]
    return p.astype(np.float32)


def chain_scene(P, eps, order, cut=None, seed=3):
    """P points on a line, 0.9 eps apart (`cut`: the gap in front of chain position `cut` is 1.1 eps); row r of the
    result is chain position order(r): "forward", "reversed" or "shuffled".  -> (points (P, 3) float32, positions (P,))"""
    gaps = np.full(P, 0.9 * eps)
    gaps[0] = 0.0
    if cut is not None:
        gaps[cut] = 1.1 * eps
    x = np.cumsum(gaps)
    pos = np.arange(P)
    if order == "reversed":
        pos = pos[::-1].copy()
    elif order == "shuffled":
        pos = np.random.default_rng(seed).permutation(P)
    p = np.zeros((P, 3), np.float32)
    p[:, 0] = x[pos]
    p[:, 1] = 0.25
    p[:, 2] = -0.5
    return p, pos
