"""The exact grid KNN at EVERY cell size, bit for bit against the CPU oracle.

Every other GPU test runs the grid search at the one cell target its K implies (`knn_cell_target`: 0.4 K or 0.625 K
points per cell, floored at 1).  The exactness argument (header of csrc/knn_grid.hip) does not depend on the cell size,
but the capacities around it do: packed run words (2047 records, 255 with grid_big=1), the defer limit of the lane
search, the quad lanes' 1024 records, the wave sort's 2048-key chunks and 16 384-record stream, the refined cells'
descriptors and table pool, the cell cap with its halving loop, 1024 cells per dimension, the micro-bin shift, the
crowded-bin list.  POINTOPS_DEBUG=grid_c_scale=F multiplies the target; on fixed data that is the search of a cloud F
times denser (or sparser) at the tuned target, so a mismatch under the knob is a mismatch some real cloud can produce.

Matrix.  F in {1/64, 1/8, 1/2, 1, 2, 8, 64, 1e6} (K = 1: the target already sits at its floor, F >= 1 only) on the
clouds of `_CLOUDS` (ragged query counts, one target shorter than K, an empty target where N = 3):
  K = 16, L2, every cloud: every F x {default, grid_quad=1, grid_quad=0, grid_big=1, grid_refine=0} and the self-query
      (same tensor objects) with its repeat under grid_same=0;
  K = 1, 8, 32, 40 (64-slot lists, no quad pass: grid_long_box=0 and =1), 100 (wave sort), L2, on uniform, clustered,
      lattice_ties and dense_run: every F x default (K <= 32: also grid_quad=1), grid_big=1 and grid_refine=0 at
      F = 1/8, 8, 64 (K <= 64); the self-query pair on the first three;
  L1 on uniform and lattice_ties: K = 16 as above, K = 8 default and the two knobs at the three scales.
Every call goes through `_C.knn_grid_stats` (version 3 + the diagnostics; grid cache off) with the environment set once
per call, and EVERY call asserts, per cloud: the grid was used (column 4) unless the target is empty; G[d] <= 1024;
G0 G1 G2 = column 3 <= 2 ceil(P2 / c) + 64 and <= 2^22; column 3 does not grow with F; column 3 = 1 at F = 1e6.
No tolerance anywhere: indices equal, distance BITS equal.

Reach table: one test per capacity branch asserts from the diagnostics that the branch ran (and parity there).  The
shapes follow from the constants; where a first estimate from the mean occupancy c did not survive the grid's
rounding (G[d] = floor(extent / h) + 1 cells per dimension, so a cloud gets up to (x + 1)^3 cells for a target of x^3)
the shape was moved until it did -- each test's docstring has the arithmetic, DESIGN.md section 2 "Cell sizes" the
values seen on an MI355X.  One row is unreachable and asserts the opposite (test_reach_refinement_clamps).
"""
import functools

import numpy as np
import pytest

import cases
import test_gpu_parity as parity
from conftest import bits
from test_gpu_parity import G

pytestmark = pytest.mark.gpu

SCALES = (1.0 / 64, 1.0 / 8, 1.0 / 2, 1.0, 2.0, 8.0, 64.0, 1e6)
MID_SCALES = (1.0 / 8, 8.0, 64.0)  # grid_big=1, grid_refine=0
_KC = (1, 2, 4, 8, 16, 32, 64)  # list capacities of the search kernels (kGridKC)


def cell_target(K, F):
    """knn_cell_target of csrc/knn_grid.hip, in its fp32 arithmetic."""
    kc = next((k for k in _KC if k >= K), _KC[-1])
    c = np.float32(np.float32(0.4 if kc >= 8 else 0.625) * np.float32(K))
    c = np.float32(c * np.float32(F))
    return float(c) if c >= 1.0 else 1.0


def knob(F, extra=""):
    return "grid_c_scale=%r" % float(F) + ("," + extra if extra else "")


# ---------------------------------------------------------------------------------------------------------- clouds
def _third(a):
    """(2, P, D) of a two-cloud generator -> (3, P, D): the third cloud is the first one read backwards."""
    return np.concatenate([a, a[:1, ::-1]], axis=0).copy()


@functools.lru_cache(maxsize=None)
def _adversarial():
    return parity._grid_adversarial_cases()


def _from_adversarial(name, three=False):
    def make():
        p1, p2, _ = _adversarial()[name]
        return (_third(p1), _third(p2)) if three else (p1, p2)
    return make


def _uniform():
    return cases.cloud(3301, (3, 6000, 3)), cases.cloud(3302, (3, 6000, 3))


def _lattice():
    return cases.lattice(3303, 3, 3000, levels=6), cases.lattice(3304, 3, 3000, levels=6)


def _slab():
    a, b = cases.cloud(3305, (2, 6000, 3)), cases.cloud(3306, (2, 6000, 3))
    a[..., 2] *= np.float32(1e-3)
    b[..., 2] *= np.float32(1e-3)
    return a, b


def _dense_run():
    return cases.cloud(3307, (2, 512, 3)), cases.cloud(3308, (2, 24576, 3))


_CLOUDS = {
    "uniform": _uniform,                                   # N = 3, 6000 points
    "clustered": _from_adversarial("clustered", True),     # N = 3, u**6
    "half_in_cluster": _from_adversarial("half_in_cluster"),
    "lattice_ties": _lattice,                              # N = 3, 3000 points, levels=6
    "planar": _from_adversarial("planar"),
    "collinear": _from_adversarial("collinear"),
    "d2": _from_adversarial("d2"),
    "d1": _from_adversarial("d1"),
    "disjoint_far": _from_adversarial("disjoint_far"),
    "slab": _slab,
    "dense_run": _dense_run,                               # 512 queries against 24 576 points
}
_ALL_K = ("uniform", "clustered", "lattice_ties", "dense_run")
_CACHE = {}


def _cloud(name):
    if ("cloud", name) not in _CACHE:
        _CACHE["cloud", name] = _CLOUDS[name]()
    return _CACHE["cloud", name]


def _lengths(p1, p2, K):
    """Ragged query counts; the second target shorter than K; with three clouds an empty third target."""
    P1, P2 = p1.shape[1], p2.shape[1]
    if p1.shape[0] == 3:
        return np.array([P1, P1 // 3, 77]), np.array([P2, max(K - 2, 1), 0])
    return np.array([P1, P1 // 3]), np.array([P2, max(K - 2, 1)])


def _oracle(oracle, key, p1, p2, l1, l2, norm, K):
    """The oracle's answer, computed once per key and never written to."""
    if key not in _CACHE:
        i, d = oracle.knn_points_idx(p1, p2, l1, l2, norm, K)
        i.setflags(write=False)
        d.setflags(write=False)
        _CACHE[key] = (i, d)
    return _CACHE[key]


# ----------------------------------------------------------------------------------------------------- one call
def first_difference(idx, d, want_i, want_d):
    """None, or a description of the first differing (cloud, query, slot) with both values."""
    bad = (idx != want_i) | (bits(d) != bits(want_d))
    if not bad.any():
        return None
    n, q, s = (int(v) for v in np.argwhere(bad)[0])
    return (f"first difference at cloud {n}, query {q}, slot {s}: got idx {int(idx[n, q, s])} dist {float(d[n, q, s])!r}"
            f" (bits {int(bits(d)[n, q, s]):#010x}), oracle idx {int(want_i[n, q, s])} dist {float(want_d[n, q, s])!r}"
            f" (bits {int(bits(want_d)[n, q, s]):#010x}); {int(bad.any(axis=2).sum())} rows differ")


def check_geometry(st, l2, P2, K, F, what):
    """What every call's diagnostics must show whatever the cell size."""
    st = st.astype(np.int64)
    cap = 2 * int(np.ceil(float(P2) / cell_target(K, F))) + 64  # grid_cell_cap
    for n in range(st.shape[0]):
        g, ncell, used = st[n, 0:3], int(st[n, 3]), int(st[n, 4])
        assert used == (1 if l2[n] > 0 else 0), f"{what}: cloud {n} (len2 {l2[n]}) use_grid = {used}: {st[n]}"
        assert (g >= 1).all() and (g <= 1024).all(), f"{what}: cloud {n} G = {g}"
        assert int(g[0] * g[1] * g[2]) == ncell, f"{what}: cloud {n} G = {g} but {ncell} cells"
        assert ncell <= cap and ncell <= 1 << 22, f"{what}: cloud {n} has {ncell} cells, cell cap {cap}"
        if F >= 1e6:
            assert ncell == 1, f"{what}: cloud {n} has {ncell} cells (G = {g}) at F = {F}"


def run(dev, monkeypatch, t1, t2, tl1, tl2, norm, K, env):
    """One knn_grid_stats call under POINTOPS_DEBUG=env (None: unset) -> numpy (idx, dists, stats)."""
    from pytorch3d_pointops_amd import _C

    if env:
        monkeypatch.setenv("POINTOPS_DEBUG", env)  # once per call: the sizer, the entry and the diagnostics agree
    else:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    assert not _C.grid_cache_enabled()
    i, d, st = _C.knn_grid_stats(t1, t2, tl1, tl2, norm, K)
    return i.cpu().numpy(), d.cpu().numpy(), st.cpu().numpy()


class Sweep:
    """The calls of one (cloud, K, norm, query set): each against the oracle, geometry checked, cell counts per knob
    set remembered so that they can be compared across F."""

    def __init__(self, dev, monkeypatch, name, K, norm, p1, p2, l1, l2, want, same):
        self.dev, self.mp, self.name, self.K, self.norm = dev, monkeypatch, name, K, norm
        self.l2, self.P2, self.want = l2, p2.shape[1], want
        self.t2, self.tl2 = G(p2, dev), G(l2, dev)
        self.t1, self.tl1 = (self.t2, self.tl2) if same else (G(p1, dev), G(l1, dev))
        self.cells = {}  # extra knobs -> [(F, cells per cloud)]

    def call(self, F, extra=""):
        env = knob(F, extra)
        what = f"{self.name} K={self.K} norm={self.norm} F={F!r} POINTOPS_DEBUG={env}"
        i, d, st = run(self.dev, self.mp, self.t1, self.t2, self.tl1, self.tl2, self.norm, self.K, env)
        diff = first_difference(i, d, *self.want)
        assert diff is None, f"{what}: {diff}\nstats:\n{st}"
        check_geometry(st, self.l2, self.P2, self.K, F, what)
        self.cells.setdefault(extra, []).append((F, st[:, 3].copy()))
        return i, d, st

    def finish(self):
        for extra, seen in self.cells.items():
            seen.sort(key=lambda fc: fc[0])
            for (fa, ca), (fb, cb) in zip(seen, seen[1:]):
                assert (cb <= ca).all(), (f"{self.name} K={self.K} norm={self.norm} knobs '{extra}': cells per cloud grow "
                                          f"from {ca} at F={fa!r} to {cb} at F={fb!r}")


def _scales(K):
    return tuple(F for F in SCALES if K > 1 or F >= 1.0)


# ---------------------------------------------------------------------------------------------------- the matrix
def _matrix():
    ids = []
    for name in _CLOUDS:
        ids.append((name, 16, 2))
    for name in _ALL_K:
        for K in (1, 8, 32, 40, 100):
            ids.append((name, K, 2))
    for name in ("uniform", "lattice_ties"):
        ids += [(name, 16, 1), (name, 8, 1)]
    return ids


_MATRIX = _matrix()
_MATRIX_IDS = [f"{n}-k{K}-l{norm}" for n, K, norm in _MATRIX]


@pytest.mark.parametrize("name,K,norm", _MATRIX, ids=_MATRIX_IDS)
def test_cell_sizes_two_sets(dev, oracle, monkeypatch, name, K, norm):
    """p1 != p2: every F x the passes of the module docstring for this (cloud, K, norm)."""
    p1, p2 = _cloud(name)
    l1, l2 = _lengths(p1, p2, K)
    want = _oracle(oracle, ("two", name, K, norm), p1, p2, l1, l2, norm, K)
    sw = Sweep(dev, monkeypatch, name, K, norm, p1, p2, l1, l2, want, same=False)
    full = K == 16
    for F in _scales(K):
        if K == 40:
            sw.call(F, "grid_long_box=0")
            sw.call(F, "grid_long_box=1")
        else:
            sw.call(F)
        if K <= 32 and (full or norm == 2):
            sw.call(F, "grid_quad=1")
        if full:
            sw.call(F, "grid_quad=0")
    if K <= 64:  # (the wave sort of K > 64 has neither run words nor refined cells)
        for F in (_scales(K) if full else [F for F in MID_SCALES if F in _scales(K)]):
            sw.call(F, "grid_big=1")
            sw.call(F, "grid_refine=0")
    sw.finish()


_SELF = ([(n, 16, 2) for n in _CLOUDS] + [("uniform", 16, 1), ("lattice_ties", 16, 1)]
         + [(n, K, 2) for n in ("uniform", "clustered", "lattice_ties") for K in (1, 8, 32, 40, 100)])


@pytest.mark.parametrize("name,K,norm", _SELF, ids=[f"{n}-k{K}-l{norm}" for n, K, norm in _SELF])
def test_cell_sizes_self_query(dev, oracle, monkeypatch, name, K, norm):
    """The queries ARE the points (the same tensor objects: one sort) at every F, and again with grid_same=0 (two
    sorts): both equal the oracle, hence each other."""
    _, p2 = _cloud(name)
    _, l2 = _lengths(p2, p2, K)
    want = _oracle(oracle, ("self", name, K, norm), p2, p2, l2, l2, norm, K)
    sw = Sweep(dev, monkeypatch, name, K, norm, p2, p2, l2, l2, want, same=True)
    for F in _scales(K):
        i, d, st = sw.call(F)
        assert (st[:, 11] == 0).all() and (st[:, 13] == 0).all(), st  # no query sort: the point sort is the query order
        i0, d0, _ = sw.call(F, "grid_same=0")
        assert np.array_equal(i, i0) and np.array_equal(bits(d), bits(d0))
    sw.finish()


def test_control_scale_changes_nothing(dev, oracle, monkeypatch):
    """F = 1 is the run with no knob set: same diagnostics, same results."""
    for name, K in (("uniform", 16), ("half_in_cluster", 8), ("clustered", 40), ("lattice_ties", 100), ("d1", 1)):
        p1, p2 = _cloud(name)
        l1, l2 = _lengths(p1, p2, K)
        args = (G(p1, dev), G(p2, dev), G(l1, dev), G(l2, dev), 2, K)
        i0, d0, st0 = run(dev, monkeypatch, *args, None)
        i1, d1, st1 = run(dev, monkeypatch, *args, knob(1.0))
        assert np.array_equal(st0, st1), (name, K, st0, st1)
        assert np.array_equal(i0, i1) and np.array_equal(bits(d0), bits(d1)), (name, K)
        want = _oracle(oracle, ("two", name, K, 2), p1, p2, l1, l2, 2, K)
        assert first_difference(i0, d0, *want) is None, (name, K)


def test_cloud_within_one_target_is_one_cell(dev, oracle, monkeypatch):
    """No knob: a cloud of no more than `knn_cell_target` points is ONE cell (K = 16: 6.4 points per cell; clouds of 1
    to 6 points, with one, two and three extents, equal extents included; 7 points are more than one target).  The
    sizing loop of grid_setup_kernel ends with h = the largest extent e for them, and e * (1 / e) rounding to 1 gave
    that dimension a second cell for the points on the box's upper face -- two cells for most clouds, eight for a
    lattice, which is what the sweep above saw at F = 1e6 before the setup pass learnt the rule."""
    K = 16
    p2 = cases.cloud(3321, (8, 7, 3))
    p2[6] = cases.lattice(3322, 1, 7, levels=2)[0] * np.float32(4.0)  # coordinates 0 or 1: equal extents
    p2[4, :, 2] = np.float32(0.5)  # planar
    p2[5, :, 1:] = np.float32(0.5)  # collinear
    l2 = np.array([1, 2, 3, 6, 6, 6, 6, 7])
    p1 = cases.cloud(3323, (8, 40, 3))
    l1 = np.array([40, 39, 0, 40, 17, 40, 40, 40])
    i, d, st = run(dev, monkeypatch, G(p1, dev), G(p2, dev), G(l1, dev), G(l2, dev), 2, K, None)
    assert (st[:, 4] == 1).all(), st
    assert (st[:7, 3] == 1).all() and (st[:7, 0:3] == 1).all(), st
    assert st[7, 3] > 1, st
    diff = first_difference(i, d, *oracle.knn_points_idx(p1, p2, l1, l2, 2, K))
    assert diff is None, f"{diff}\nstats:\n{st}"


# ------------------------------------------------------------------------------------------------- the reach table
def _reach(dev, oracle, monkeypatch, key, p1, p2, l1, l2, norm, K, F, extra=""):
    want = _oracle(oracle, key, p1, p2, l1, l2, norm, K)
    sw = Sweep(dev, monkeypatch, key[1], K, norm, p1, p2, l1, l2, want, same=False)
    st = sw.call(F, extra)[2].astype(np.int64)
    print(f"\n{key[1]} K={K} F={F!r} {extra}: stats\n{st}")
    return st


def test_reach_run_longer_than_run_word(dev, oracle, monkeypatch):
    """A run of more than 2047 records (the packed length field) sends its query to the box search.
    K = 32, F = 64: c = 819.2.  512 queries against 20 480 uniform points: a target of 25 cells, h = 0.342, 3 cells per
    dimension, 27 cells of ~758 points; a row of three x-cells is one run of ~2275 +- 48 records, and the queries of the
    middle x-layer -- a third of them, 171 +- 11: the cubes of the outer layers are clipped to two x-cells -- list such
    rows and are deferred (column 8 above a quarter of the queries).  (With the 24 576 points of dense_run the target of
    30 cells becomes 4^3 = 64 cells of 384 points, runs of ~1150: that shape does not reach the branch, whatever its mean
    of 819 per target cell.)"""
    K, F = 32, 64.0
    p1, p2 = cases.cloud(3311, (1, 512, 3)), cases.cloud(3312, (1, 20480, 3))
    l1, l2 = np.array([512]), np.array([20480])
    st = _reach(dev, oracle, monkeypatch, ("reach", "run_word"), p1, p2, l1, l2, 2, K, F)
    assert tuple(st[0, 0:3]) == (3, 3, 3), st
    assert l2[0] // 9 > 2047  # a mean row of three x-cells (a ninth of the cloud) against the run word
    assert 512 // 4 < st[0, 8] < 512, st


def test_reach_run_longer_than_big_run_word(dev, oracle, monkeypatch):
    """grid_big=1: run words of 255 records.  uniform (6000 points), K = 16, F = 16: c = 102.4, a target of 58.6 cells,
    h = 0.2575, 4^3 = 64 cells of ~94 points: the three-cell runs of the interior queries hold ~281 records > 255
    (column 8 > 0), while without the knob nothing is deferred (runs far below 2047, cubes far below the defer limit)."""
    K, F = 16, 16.0
    p1, p2 = _cloud("uniform")
    l1, l2 = _lengths(p1, p2, K)
    key = ("two", "uniform", K, 2)
    st = _reach(dev, oracle, monkeypatch, key, p1, p2, l1, l2, 2, K, F, "grid_big=1")
    st0 = _reach(dev, oracle, monkeypatch, key, p1, p2, l1, l2, 2, K, F)
    assert tuple(st[0, 0:3]) == (4, 4, 4) and 3 * l2[0] // 64 > 255, st
    assert st[0, 8] > 0 and st0[0, 8] == 0, (st, st0)


def test_reach_cube_over_defer_limit(dev, oracle, monkeypatch):
    """half_in_cluster (K = 8), F = 1/8: c = 1 (the floor), refine threshold 64, defer limit 256; the 1e-3 cluster puts
    10 000 points into one cell, or a few, of ~0.037: those cells are refined (column 9 > 0) and every query whose
    cube holds one of them leaves the lane search for the box search (column 8 at least the cluster's queries)."""
    p1, p2, K = _adversarial()["half_in_cluster"]
    l1, l2 = _lengths(p1, p2, K)
    st = _reach(dev, oracle, monkeypatch, ("two", "half_in_cluster", K, 2), p1, p2, l1, l2, 2, K, 1.0 / 8)
    assert st[0, 9] > 0 and st[0, 8] >= p1.shape[1] // 2, st


def test_reach_quad_over_its_records(dev, oracle, monkeypatch):
    """The quad pass defers a query whose grown cube holds more than 4 x 1024 records to the box search.
    On a uniform cloud the lane pass certifies every interior query at F = 8 (the cube's faces are a whole cell of
    0.2 away, the 16th neighbour 0.086), so the quad pass gets nothing to grow there.  half_in_cluster (20 000 points,
    half of them in one cell) at the tuned cell size does: in its uniform half (3.2 points per cell, K = 16) most
    queries stay uncertified after the lane pass (column 5 > 0), their estimate grows the cube to 5 cells per
    dimension, and those within two cells of the cluster -- but not next to it, where the lane pass has already
    deferred them -- find 10 000 records in it: column 8 with grid_quad=1 exceeds column 8 with grid_quad=0, and only
    the quad kernel's over-full branch adds to it."""
    K = 16
    p1, p2 = _cloud("half_in_cluster")
    l1, l2 = _lengths(p1, p2, K)
    key = ("two", "half_in_cluster", K, 2)
    on = _reach(dev, oracle, monkeypatch, key, p1, p2, l1, l2, 2, K, 1.0, "grid_quad=1")
    off = _reach(dev, oracle, monkeypatch, key, p1, p2, l1, l2, 2, K, 1.0, "grid_quad=0")
    assert on[0, 5] > 0, on
    assert l2[0] // 2 > 4 * 1024  # the cluster alone is over the quad's limit
    assert on[0, 8] > off[0, 8], (on, off)


def test_reach_cube_under_k_points(dev, oracle, monkeypatch):
    """uniform, K = 16, F = 1/64: c = 1, 19^3 cells of 0.87 points, h = 0.055.  The 16th neighbour lies ~0.086 away,
    further than the farthest a cube's nearest face can be (1.5 h = 0.082): the lane pass certifies next to nothing
    (column 5: more than half of the queries by that argument; the control certifies most), the wave search finishes
    every one of them (column 7 as in the control: only the queries of the empty target)."""
    K = 16
    p1, p2 = _cloud("uniform")
    l1, l2 = _lengths(p1, p2, K)
    key = ("two", "uniform", K, 2)
    st = _reach(dev, oracle, monkeypatch, key, p1, p2, l1, l2, 2, K, 1.0 / 64)
    ctl = _reach(dev, oracle, monkeypatch, key, p1, p2, l1, l2, 2, K, 1.0)
    assert st[0, 5] > l1[0] // 2 and st[0, 5] > 4 * ctl[0, 5], (st, ctl)
    assert np.array_equal(st[:, 6], ctl[:, 6]) and np.array_equal(st[:, 7], ctl[:, 7]), (st, ctl)
    assert st[0, 7] == 0 and st[2, 7] == l1[2], st


@pytest.mark.parametrize("F", [2.0, 16.0])
def test_reach_wave_sort_limits(dev, oracle, monkeypatch, F):
    """K = 100 (wave sort), 256 queries against 16 800 uniform points.
    F = 2: c = 80, a target of 210 = 5.94^3 cells, 6^3 = 216 cells of 77.8 points: an interior cube holds ~2100 records,
    more than the 2048 keys of one sort, so the stream is consumed in chunks (27 len2 / cells > 2048); the queries are
    still answered by the sort (column 7 far below the query count).
    F = 16: c = 640, a target of 26.25 = 2.97^3 cells, 3^3 = 27 cells of 622 points: the cube of a query of the centre
    cell is the whole cloud, 16 800 records > the 16 384 the kernel streams, and it goes to the all-pairs list (column
    7 > 0: one query in 27, 9.5 +- 3); the clipped cubes of the other cells hold at most 18 cells and certify (their
    faces are a cell of 0.33 away, the 100th neighbour 0.11).
    (20 000 points give 7^3 cells of 58 points at F = 2: 1574 records per cube, under the limit.)"""
    K = 100
    p1, p2 = cases.cloud(3313, (1, 256, 3)), cases.cloud(3314, (1, 16800, 3))
    l1, l2 = np.array([256]), np.array([16800])
    st = _reach(dev, oracle, monkeypatch, ("reach", "wsort"), p1, p2, l1, l2, 2, K, F)
    if F == 2.0:
        assert st[0, 3] == 216 and 27 * l2[0] // st[0, 3] > 2048, st
        assert st[0, 7] < 128, st
    else:
        assert st[0, 3] == 27 and 27 * l2[0] // st[0, 3] > 16384, st
        assert 0 < st[0, 7] < 256 // 4, st


@pytest.mark.parametrize("name", ["d1", "collinear"])
def test_reach_cells_per_dimension_cap(dev, oracle, monkeypatch, name):
    """3000 points on a line at c = 1 (F = 1/64) ask for 3000 cells in one dimension: the cell edge is raised to
    extent / 1023.5 and G[0] = 1024 = kGMax."""
    p1, p2, K = _adversarial()[name]
    l1, l2 = _lengths(p1, p2, K)
    st = _reach(dev, oracle, monkeypatch, ("two", name, K, 2), p1, p2, l1, l2, 2, K, 1.0 / 64)
    assert tuple(st[0, 0:3]) == (1024, 1, 1), st


@pytest.mark.parametrize("name", ["clustered", "half_in_cluster"])
def test_reach_refinement_clamps(dev, oracle, monkeypatch, name):
    """K = 8, F = 1/64: c = 1, the smallest refine threshold (64) and the largest tables per point.  The clamps of the
    refined cells (`rdesc_cap` = P2 / 64 + 1 descriptors, `pool_cap` = 4 P2 + 64 table entries) are NOT reachable: a
    refined cell holds at least 65 points, so a cloud has at most P2 / 65 of them, and their tables sum to less than
    2.5 P2 for every c >= 1 (comment at pool_cap in csrc/grid_build.hip).  So this row asserts the opposite -- cells ARE
    refined (column 9 > 0) and their count stays inside the descriptors -- and keeps the parity check at the scale
    where both are fullest."""
    p1, p2 = _cloud(name)
    K = 8
    l1, l2 = _lengths(p1, p2, K)
    st = _reach(dev, oracle, monkeypatch, ("two", name, K, 2), p1, p2, l1, l2, 2, K, 1.0 / 64)
    assert 0 < st[0, 9] <= l2[0] // 65 < p2.shape[1] // 64 + 1, st
    off = _reach(dev, oracle, monkeypatch, ("two", name, K, 2), p1, p2, l1, l2, 2, K, 1.0 / 64, "grid_refine=0")
    assert (off[:, 9] == 0).all(), off


@pytest.mark.parametrize("F", [1.0 / 8, 8.0])
def test_reach_more_crowded_bins_than_listed(dev, oracle, monkeypatch, F):
    """The cloud of test_knn_grid_many_crowded_bins (100 clusters of 9000 points in 2e-4 cubes + 50 000 uniform points,
    K = 4) at c = 1 and c = 20: at either size every cluster is a bin of its own with more than 8192 records, 64 of
    them listed (columns 12 / 13 full resp. non-zero), the rest sorted by one workgroup each.  300 sampled queries
    against the oracle over the whole cloud."""
    from pytorch3d_pointops_amd import _C

    K = 4
    if "crowded" not in _CACHE:
        rng = np.random.default_rng(2701)
        centres = rng.random((100, 3), dtype=np.float32)
        pts = (centres[:, None, :] + rng.random((100, 9000, 3), dtype=np.float32) * np.float32(2e-4)).reshape(-1, 3)
        pts = np.concatenate([pts, rng.random((50000, 3), dtype=np.float32)])
        rng.shuffle(pts)
        q = np.concatenate([pts[::37][:20000] + np.float32(1e-5), rng.random((10000, 3), dtype=np.float32),
                            centres[:1] + rng.random((10000, 3), dtype=np.float32) * np.float32(2e-4)]).astype(np.float32)
        sel = np.arange(5, q.shape[0], q.shape[0] // 300)
        l2 = np.array([pts.shape[0]])
        want = oracle.knn_points_idx(q[None, sel], pts[None], np.array([sel.size]), l2, 2, K)
        _CACHE["crowded"] = (pts[None], q[None], sel, want)
    p2, p1, sel, want = _CACHE["crowded"]
    l1, l2 = np.array([p1.shape[1]]), np.array([p2.shape[1]])
    what = f"many crowded bins K={K} F={F!r}"
    monkeypatch.setenv("POINTOPS_DEBUG", knob(F))
    i, d, st = _C.knn_grid_stats(G(p1, dev), G(p2, dev), G(l1, dev), G(l2, dev), 2, K)
    i, d, st = i.cpu().numpy(), d.cpu().numpy(), st.cpu().numpy()
    print(f"\n{what}: stats\n{st}")
    check_geometry(st, l2, p2.shape[1], K, F, what)
    assert st[0, 10] >= 100 and st[0, 12] == 64 and st[0, 13] >= 1, st
    diff = first_difference(i[:, sel], d[:, sel], *want)
    assert diff is None, f"{what}: {diff} (query = sampled row)\nstats:\n{st}"
