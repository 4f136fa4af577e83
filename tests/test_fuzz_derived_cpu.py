"""The committed cases of tests/fuzz_derived_cases.py (offset 0) certified without a GPU, with the checkers alone: a fuzz
is only as good as its draws.

  floors      the cases hold what the soak is for -- kept and removed rows, several clusters, noise, border points, clouds
              on both sides of the 512-point grid threshold in one batch, pairs at exactly the radius, long and single
              voxels, points on voxel faces, winners and invalid slots, keypoints and salient non-keypoints
  mutations   for each mistake a kernel actually makes (`<=` at the radius, lengths ignored, self not counted, the largest
              border label, an unstable compaction, truncation for floor, the population deviation, the last best count)
              the checker with that mistake differs from the true one on at least one committed case of its operator

A floor that is missed is the generator's to mend, never the floor's."""
import numpy as np
import pytest

import cluster_ref
import filters_ref
import fuzz_derived_cases as gen
import iss_ref
import plane_ref
import ransac_ref
import voxel_ref

_CACHE = {}
_TRUE_CELLS, _TRUE_STATISTICS = voxel_ref.cloud_cells, filters_ref.statistics


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _radius_cases():
    return _once("radius", lambda: [c for s in gen.SEEDS for c in gen.radius_family_cases(s)])


def _iss_cases():
    return [c for c in _radius_cases() if c.D == 3]


def _voxel_cases():
    return _once("voxel", lambda: [c for s in gen.SEEDS for c in gen.voxel_cases(s)])


def _consensus_cases(op):
    return [c for c in _once("consensus", lambda: [c for s in gen.SEEDS for c in gen.consensus_cases(s)]) if c.op == op]


def _key(c):
    return c.what["family"], c.what["seed"], c.what["index"]


def _dbscan(c):
    return _once(("dbscan",) + _key(c), lambda: cluster_ref.dbscan(c.points, c.lengths, c.radius, c.min_points))


def _radius(c):
    return _once(("radius",) + _key(c), lambda: filters_ref.radius(c.points, c.lengths, c.radius, c.min_points))


def _iss(c):
    return _once(("iss",) + _key(c), lambda: iss_ref.iss(c.points, c.lengths, c.radius, c.rn, min_neighbors=c.min_points))


def _voxel(c):
    return _once(("voxel",) + _key(c), lambda: voxel_ref.downsample(c.points, c.lengths, c.voxel_size, c.features, c.origin))


def _consensus(c):
    if c.op == "plane":
        return _once(("plane",) + _key(c), lambda: plane_ref.run(c.X, c.lengths, c.mask, dtype=np.float32, **c.kw))
    return _once(("ransac",) + _key(c), lambda: ransac_ref.run(c.X, c.Y, c.corr, c.len1, c.len2, dtype=np.float32, **c.kw))


def _live(c):
    return np.arange(c.points.shape[1])[None, :] < c.lengths[:, None]


def _at_least(share, flags, what):
    flags = list(flags)
    assert sum(flags) >= share * len(flags), f"{what}: {sum(flags)} of {len(flags)} cases, the floor is {share:.2f}"
    print(f"{what}: {sum(flags)} of {len(flags)}")


# ------------------------------------------------------------------------------------------------ the generator itself
def test_cases_are_reproducible_and_shaped_as_the_rule_says():
    again = gen.radius_family_cases(gen.SEEDS[0])
    for a, b in zip(again, _radius_cases()):
        assert a.what == b.what and a.points.tobytes() == b.points.tobytes()
    seen_P, seen_L, empty = set(), set(), 0
    for c in _radius_cases() + _voxel_cases():
        N, P = c.points.shape[:2]
        assert 1 <= N <= 6 and 1 <= P <= gen.P_MAX and (c.lengths == P).any() and (c.lengths >= 0).all()
        assert (c.points[~_live(c)] == gen.PAD).all() and (c.points[_live(c)] != gen.PAD).all()
        seen_P.add(P)
        seen_L.update(c.lengths.tolist())
        empty += bool((c.lengths == 0).any())
    assert set(gen.P_EDGES) <= seen_P and set(gen.L_EDGES) <= seen_L
    assert 0.1 <= empty / len(_radius_cases() + _voxel_cases()) <= 0.45
    assert {c.kind for c in _radius_cases()} == set(gen.KINDS) and {c.D for c in _radius_cases()} == {1, 2, 3}
    for op in ("plane", "ransac"):
        cases = _consensus_cases(op)
        assert {c.kw["H"] for c in cases} == set(gen.HYPOTHESES)
        valid = {v for c in cases for v in c.what["valid"]}
        assert set(gen.VALID_EDGES) <= valid, (op, sorted(set(gen.VALID_EDGES) - valid))


@pytest.mark.parametrize("soak", [0, 1000, 2000])
def test_every_family_draws_its_cases_at_any_offset(monkeypatch, soak):
    """The generator itself must not fail where the GPU soak calls it: every family, every seed, shifted offsets too."""
    monkeypatch.setattr(gen, "SOAK", soak)
    for seed in gen.SEEDS:
        assert len(gen.radius_family_cases(seed)) == gen.RADIUS_CASES and len(gen.voxel_cases(seed)) == gen.VOXEL_CASES
        assert len(gen.statistical_cases(seed)) == gen.STAT_CASES and len(gen.compact_cases(seed)) == gen.COMPACT_CASES
        assert [c.op for c in gen.consensus_cases(seed)] == ["plane", "ransac"] * (gen.CONSENSUS_CASES // 2)
        for c in gen.statistical_cases(seed):
            assert (c.dists[..., 0][np.arange(c.dists.shape[1])[None, :] < c.lengths[:, None]] == 0).all()
            assert (c.dists >= 0).all() and (c.lengths == c.dists.shape[1]).any()
        for c in gen.registration_cases(seed):
            assert c.X.shape[1] == c.len_x.max() and c.Y.shape[1] == c.len_y.max() and c.normals.shape == c.Y.shape
            assert (c.X[np.arange(c.X.shape[1])[None, :] >= c.len_x[:, None]] == gen.PAD).all(), c.what
            assert c.what["soak"] == soak


def test_registration_cases_meet_their_edges():
    sizes = {v for s in gen.SEEDS for c in gen.registration_cases(s) for ab in c.what["sizes"] for v in ab}
    assert set(gen.REG_EDGES) <= sizes, sorted(set(gen.REG_EDGES) - sizes)
    stat = {v for s in gen.SEEDS for c in gen.statistical_cases(s) for v in [c.dists.shape[1]] + c.lengths.tolist()}
    assert set(gen.STAT_EDGES) <= stat, sorted(set(gen.STAT_EDGES) - stat)
    assert {c.dists.shape[2] for s in gen.SEEDS for c in gen.statistical_cases(s)} == set(gen.STAT_K1)


# ------------------------------------------------------------------------------------------------ the floors
def test_radius_filter_floor():
    def both(c):
        w, live = _radius(c), _live(c)
        return any((w["mask"][n] & live[n]).any() and (~w["mask"][n] & live[n]).any() for n in range(len(live)))
    _at_least(0.5, (both(c) for c in _radius_cases()), "radius filter: a cloud with kept and removed rows")


def test_dbscan_floors():
    cases = _radius_cases()
    _at_least(0.5, ((_dbscan(c)[1] >= 2).any() for c in cases), "dbscan: a cloud with two or more clusters")
    _at_least(0.5, (((_dbscan(c)[0] == -1) & _live(c)).any() for c in cases), "dbscan: a noise point on a live row")
    _at_least(0.25, (((_dbscan(c)[0] >= 0) & ~_dbscan(c)[2]).any() for c in cases), "dbscan: a border point")


def test_mixed_path_floor():
    def mixed(c):
        return bool((c.lengths >= 512).any() and ((c.lengths >= 2) & (c.lengths <= 511)).any())
    cases = [c for c in _radius_cases() if c.points.shape[1] >= 512]
    assert len(cases) >= 10
    _at_least(0.25, (mixed(c) for c in cases), "a cloud of 512 or more points beside one of 2 to 511")
    assert sum(mixed(c) for c in cases if c.D == 3) >= 3  # (iss_keypoints takes the D = 3 cases)


def _has_tie(c):
    r2 = np.float32(c.radius) * np.float32(c.radius)
    return any(bool((filters_ref.d2_rows(c.points[n, :L], 0, L) == r2).any()) for n, L in enumerate(c.lengths) if L > 1)


def test_ties_floor():
    ties = [c for c in _radius_cases() if c.kind == "lattice" and c.radius in (0.125, 0.25) and _has_tie(c)]
    assert len(ties) >= 3, "cluster_dbscan and remove_radius_outlier"
    assert sum(c.D == 3 for c in ties) >= 3, "iss_keypoints"
    for c in _radius_cases():  # by construction: such a lattice with two rows a step (or two) apart has one
        if c.kind == "lattice" and c.radius in (0.125, 0.25) and (c.lengths >= 64).any():
            assert c in ties, c.what


def test_voxel_floors():
    def long_and_single(c):
        w = _voxel(c)
        rows = np.arange(w["counts"].shape[1])[None, :] < w["num_voxels"][:, None]
        return bool((w["counts"] > 16).any() and ((w["counts"] == 1) & rows).any())

    def on_a_face(c):
        live = voxel_ref.live_rows(c.points, c.lengths)
        v = np.float64(np.float32(c.voxel_size))
        for n in range(len(live)):
            if not live[n].any():
                continue
            x = c.points[n, live[n]].astype(np.float64)
            o = c.points[n, live[n]].min(0).astype(np.float64) - 0.5 * v if c.origin is None else \
                c.origin.reshape(-1, 3)[n if c.origin.ndim == 2 else 0].astype(np.float64)
            q = (x - o) / v
            if (q == np.floor(q)).any():
                return True
        return False
    cases = _voxel_cases()
    assert not any(_voxel(c)["status"].any() for c in cases)
    _at_least(1 / 3, (long_and_single(c) for c in cases), "voxel: more than 16 members and exactly one")
    assert sum(on_a_face(c) for c in cases) >= 2
    assert {None if c.features is None else c.features.shape[2] for c in cases} == set(gen.CHANNELS)
    assert {None if c.origin is None else c.origin.ndim for c in cases} == {None, 1, 2}


def _invalid_slot(c):
    w = _consensus(c)
    return bool(((w["samples"] >= 0).all(-1) & ~w["valid"]).any())


def test_consensus_floors():
    cases = _consensus_cases("plane") + _consensus_cases("ransac")
    _at_least(0.5, ((_consensus(c)["best"] >= 0).any() for c in cases), "consensus: a winning hypothesis")
    _at_least(0.25, (_invalid_slot(c) for c in cases), "consensus: a drawn but invalid slot")
    for op in ("plane", "ransac"):
        assert sum(_invalid_slot(c) for c in _consensus_cases(op)) >= 2, op


def test_iss_floors():
    cases = _iss_cases()
    _at_least(1 / 3, (_iss(c)["mask"].any() for c in cases), "iss: a keypoint")
    _at_least(1 / 3, (((_iss(c)["saliency"] > 0) & ~_iss(c)["mask"]).any() for c in cases), "iss: a salient non-keypoint")


# ------------------------------------------------------------------------------------------------ the mutated checkers
def _differs(a, b):
    if isinstance(a, dict):
        return any(_differs(a[k], b[k]) for k in a if a[k] is not None)
    if isinstance(a, (tuple, list)):
        return any(_differs(x, y) for x, y in zip(a, b))
    return not np.array_equal(a, b)


def _closed_neighbours(p, eps):
    p = np.ascontiguousarray(p, np.float32)
    return filters_ref.d2_rows(p, 0, len(p)) <= np.float32(eps) * np.float32(eps)


def _closed_radius_counts(p, radius):
    return (_closed_neighbours(p, radius).sum(1) - 1).astype(np.int32)


def _largest_border_label(c):
    labels, num, core = (a.copy() for a in _dbscan(c))
    for n, L in enumerate(c.lengths):
        if L == 0:
            continue
        adj = cluster_ref.neighbours(c.points[n, :L], c.radius) & core[n, None, :L]
        rows = np.where(adj, labels[n, None, :L], -1).max(1)
        labels[n, :L] = np.where(core[n, :L], labels[n, :L], rows)
    return labels, num, core


def _unstable_compact(mask):
    index, num = filters_ref.compact(mask)
    for n, k in enumerate(num):
        index[n, :k] = index[n, :k][::-1]
    return index, num


def _truncated_cells(pts, live, v, origin):
    status, c, member = _TRUE_CELLS(pts, live, v, origin)
    if member.any():
        v64 = np.float64(np.float32(v))
        o = origin.astype(np.float64) if origin is not None else pts[live].min(0).astype(np.float64) - np.float64(0.5) * v64
        c = c.copy()
        c[live] = np.trunc((pts[live].astype(np.float64) - o) / v64).astype(np.int64)
    return status, c, member


def _population_statistics(m, length, P):
    mean, std, nf = _TRUE_STATISTICS(m, length, P)
    return mean, (std * np.sqrt((nf - 1.0) / nf) if nf >= 2 else std), nf


def _last_best(counts):
    counts = np.asarray(counts, np.int64)
    best = counts.shape[1] - 1 - counts[:, ::-1].argmax(1)
    best[counts.max(1) < 0] = -1
    return best


def _mutations(monkeypatch):
    """name -> (cases, true result of a case, mutated result of a case)"""
    def patched(module, name, value, fn):
        def run(c):
            with monkeypatch.context() as m:
                m.setattr(module, name, value(c) if getattr(value, "per_case", False) else value)
                return fn(c)
        return run

    def closed_within(q, p, radius):
        d = q[:, None, :] - p[None, :, :]
        return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) <= np.float32(radius) * np.float32(radius)

    def closed_support(c):  # the support's radius alone: the suppression keeps its `<`
        true = iss_ref.within
        return lambda q, p, radius: closed_within(q, p, radius) if radius == c.radius else true(q, p, radius)
    closed_support.per_case = True

    dbscan = lambda c, **kw: cluster_ref.dbscan(c.points, kw.get("lengths", c.lengths), c.radius,  # noqa: E731
                                                kw.get("mp", c.min_points))
    radius = lambda c, **kw: filters_ref.radius(c.points, kw.get("lengths", c.lengths), c.radius,  # noqa: E731
                                                kw.get("mn", c.min_points))
    iss = lambda c, **kw: iss_ref.iss(c.points, kw.get("lengths", c.lengths), c.radius, c.rn,  # noqa: E731
                                      min_neighbors=kw.get("mn", c.min_points))
    voxel = lambda c, **kw: voxel_ref.downsample(c.points, kw.get("lengths", c.lengths), c.voxel_size, c.features,  # noqa: E731
                                                 c.origin)
    stat = lambda c: filters_ref.statistical_from_dists(c.dists, c.lengths, c.std_ratio)  # noqa: E731
    stats = [c for s in gen.SEEDS for c in gen.statistical_cases(s)]
    compacts = [c for s in gen.SEEDS for c in gen.compact_cases(s)]
    consensus = _consensus_cases("plane") + _consensus_cases("ransac")
    R, I, V = _radius_cases(), _iss_cases(), _voxel_cases()
    return {
        "closed radius: cluster": (R, _dbscan, patched(cluster_ref, "neighbours", _closed_neighbours, dbscan)),
        "closed radius: radius filter": (R, _radius, patched(filters_ref, "radius_counts", _closed_radius_counts, radius)),
        "closed radius: iss support": (I, _iss, patched(iss_ref, "within", closed_support, iss)),
        "lengths ignored: cluster": (R, _dbscan, lambda c: dbscan(c, lengths=None)),
        "lengths ignored: radius filter": (R, _radius, lambda c: radius(c, lengths=None)),
        "lengths ignored: iss": (I, _iss, lambda c: iss(c, lengths=None)),
        "lengths ignored: voxel": (V, _voxel, lambda c: voxel(c, lengths=None)),
        "self not counted: cluster": (R, _dbscan, lambda c: dbscan(c, mp=c.min_points + 1)),
        "self counted: radius filter": (R, _radius, lambda c: radius(c, mn=c.min_points - 1)),
        "self not counted: iss": (I, _iss, lambda c: iss(c, mn=c.min_points + 1)),
        "largest border label": (R, _dbscan, _largest_border_label),
        "unstable compaction": (compacts, lambda c: filters_ref.compact(c.mask), lambda c: _unstable_compact(c.mask)),
        "truncated voxel key": (V, _voxel, patched(voxel_ref, "cloud_cells", _truncated_cells, voxel)),
        "population deviation": (stats, stat, patched(filters_ref, "statistics", _population_statistics, stat)),
        "last best count": (consensus, lambda c: ransac_ref.select(_consensus(c)["counts"]),
                            lambda c: _last_best(_consensus(c)["counts"])),
    }


MUTATIONS = ["closed radius: cluster", "closed radius: radius filter", "closed radius: iss support",
             "lengths ignored: cluster", "lengths ignored: radius filter", "lengths ignored: iss", "lengths ignored: voxel",
             "self not counted: cluster", "self counted: radius filter", "self not counted: iss", "largest border label",
             "unstable compaction", "truncated voxel key", "population deviation", "last best count"]


@pytest.mark.parametrize("name", MUTATIONS)
def test_a_mutated_checker_is_caught_by_a_committed_case(monkeypatch, name):
    table = _mutations(monkeypatch)
    assert sorted(table) == sorted(MUTATIONS)
    cases, true, mutated = table[name]
    caught = next((c for c in cases if _differs(true(c), mutated(c))), None)
    assert caught is not None, f"no committed case tells the checker from its mutation '{name}'"
    print(f"{name}: first caught by {caught.what}")
