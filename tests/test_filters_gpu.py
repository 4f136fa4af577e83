"""remove_radius_outlier, remove_statistical_outlier and mask_to_index on the GPU against the numpy checker of
tests/filters_ref.py.  Everything is compared for equality -- integers, and floating-point results bit for bit:

    radius       mask, counts, index, num_kept equal the checker; the early-exit call (no counts) gives the same mask;
                 the library's choice, POINTOPS_DEBUG=filter_grid=0 (all pairs) and =1 (a grid whatever the size) -- the
                 two forced paths each in a fresh child process -- are equal; mask equals cluster_dbscan's core_mask
    statistical  knn_points' table equals the checker's; mean_distance, stats, threshold, mask, index, num_kept equal the
                 checker's evaluation of it; two calls are byte-equal; a cloud alone equals the cloud in a batch
    compaction   mask_to_index equals the checker and keypoints_to_padded; select_rows and the Pointclouds methods
                 carry features
    contract     guarded, poisoned buffers (tests/buffers.py), short and null workspaces, empty shapes, 65 540 clouds,
                 a side stream, a captured graph
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import buffers
import filters_cases as cases
import filters_ref as ref
from conftest import ROOT
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
RADIUS_ENTRY, STAT_ENTRY = "pointops_radius_outlier", "pointops_statistical_outlier"
CASES = cases.radius_cases()
_WANT = {}


def _want_radius(name):
    if name not in _WANT:
        _WANT[name] = ref.radius(*CASES[name])
    return _WANT[name]


def _assert_equal(got, want, keys, what):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} is {a.dtype}{a.shape}, want {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))
            at = tuple(bad[0][:-1])
            raise AssertionError(f"{what}: {k} differs at {len(bad)} bytes, first at {at}: got {a[at]!r}, want {b[at]!r}")


def _guarded(monkeypatch, call, fill="ones", sibling=None, **watched):
    with buffers.contract(monkeypatch, fill, short_workspace="short" if fill == "ones" else False,
                          prototypes=PROTOS) as c:
        if sibling is not None:
            c.sibling(sibling)
        c.watch(**watched)
        out = call()
    c.assert_all_clear()
    return out, c


# ------------------------------------------------------------------------------------------------ radius
@pytest.fixture(scope="module")
def forced_paths(tmp_path_factory):
    """{knob value: the npz a fresh child process saved of every radius case under POINTOPS_DEBUG=filter_grid=value}"""
    out = {}
    for value in (0, 1):
        path = str(tmp_path_factory.mktemp("filters") / f"grid{value}.npz")
        env = dict(os.environ, POINTOPS_DEBUG=f"filter_grid={value}",
                   PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "filters_cases.py"), path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out[value] = np.load(path)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_radius_case_equals_the_checker_on_every_path(dev, monkeypatch, forced_paths, name):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    case = CASES[name]
    pts, lengths, radius, mn = case
    want = _want_radius(name)
    got, c = _guarded(monkeypatch, lambda: cases.run_case(dev, case))
    assert {(n, how) for n, _, how in c.rejections} == {(RADIUS_ENTRY, "short"), (RADIUS_ENTRY, "null")}
    assert [b.kind for b in c.buffers] == ["out"] * 4 + ["workspace"]
    _assert_equal(got, want, cases.KEYS, f"{name} [default]")
    early = cases.run_case(dev, case, want_counts=False)
    assert "counts" not in early
    _assert_equal(early, want, cases.KEYS[:3], f"{name} [default, early exit]")
    for value, saved in forced_paths.items():
        forced = {k: saved[f"{name}/{k}"] for k in cases.KEYS}
        _assert_equal(forced, want, cases.KEYS, f"{name} [filter_grid={value}]")
        _assert_equal({"mask": saved[f"{name}/mask-early"]}, want, ["mask"], f"{name} [filter_grid={value}, early exit]")
    core = f.cluster_dbscan(torch.from_numpy(pts).to(dev), radius, mn + 1, lengths=torch.from_numpy(lengths).to(dev)).core_mask
    assert np.array_equal(core.cpu().numpy(), want["mask"]), f"{name}: cluster_dbscan's core_mask"


def test_what_the_radius_cases_are_meant_to_show():
    w = _want_radius("uniform-D3-mn5")
    assert 0.5 * 700 < w["num_kept"][0] < 700 and 0 < w["num_kept"][1] <= 513 and w["num_kept"][2] == 0
    assert 8 < w["counts"][0].mean() < 22  # about 15 neighbours per radius, fewer at the faces
    assert not w["mask"][1, 513:].any() and not w["counts"][1, 513:].any()
    assert _want_radius("uniform-D3-mn0")["num_kept"].tolist() == [700, 513, 0]
    assert not _want_radius("uniform-D3-mn700")["mask"].any()
    for D in (1, 2, 3):
        o = _want_radius(f"outlier-D{D}-mn1")
        assert o["counts"][0, 7] == 0 and not o["mask"][0, 7] and o["num_kept"][0] > 350 and 7 not in o["index"][0]
        assert _want_radius(f"pair-at-radius-D{D}")["counts"].tolist() == [[0, 0]]
        assert _want_radius(f"pair-inside-D{D}")["counts"].tolist() == [[1, 1]]
        s = _want_radius(f"short-D{D}-mn0")
        assert s["num_kept"].tolist() == [1, 2, 37]
    assert _want_radius("slab-D3-mn5")["counts"][0].mean() > 3 * w["counts"][0].mean()


# ------------------------------------------------------------------------------------------------ statistical
STAT_P = 1025
STAT_LENGTHS = np.array([0, 1, 2, 255, 256, 257, 1000, 1025], np.int64)
_STAT = {}


def _stat_points():
    if "points" not in _STAT:
        _STAT["points"] = np.stack([ref.uniform_scene(300 + n, STAT_P) for n in range(len(STAT_LENGTHS))])
    return _STAT["points"]


def _stat_table(nb):
    """The checker's table of the batch, once per nb_neighbors."""
    if nb not in _STAT:
        _STAT[nb] = ref.knn_table(_stat_points(), STAT_LENGTHS, nb + 1)
    return _STAT[nb]


STAT_KEYS = ("mask", "num_kept", "index", "mean_distance", "threshold", "mean", "std")


def _stat_want(table, lengths, ratio):
    w = ref.statistical_from_dists(table, lengths, ratio)
    w["mean"], w["std"] = np.ascontiguousarray(w["stats"][:, 0]), np.ascontiguousarray(w["stats"][:, 1])
    return w


def _stat_got(r):
    return {k: getattr(r, k).cpu().numpy() for k in STAT_KEYS}


@pytest.mark.parametrize("nb", [1, 8, 127])
def test_statistical_batch_equals_the_checker_bit_for_bit(dev, monkeypatch, nb):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts, lengths = torch.from_numpy(_stat_points()).to(dev), torch.from_numpy(STAT_LENGTHS).to(dev)
    table = _stat_table(nb)
    # stage 1: the search.  Only rows below the length count; slots past it are knn_points' zero padding
    dists = f.knn_points(pts, pts, lengths, lengths, K=nb + 1).dists.cpu().numpy()
    live = np.arange(STAT_P)[None, :] < STAT_LENGTHS[:, None]
    assert np.array_equal(dists[live].view(np.int32), table[live].view(np.int32)), "knn_points' table"
    first = None
    for ratio in (0.0, 1.0, 2.0):
        r = f.remove_statistical_outlier(pts, lengths, nb_neighbors=nb, std_ratio=ratio)
        assert r.mask.dtype == torch.bool and r.mean.dtype == torch.float64 and r.threshold.dtype == torch.float32
        want = _stat_want(table, STAT_LENGTHS, ratio)
        _assert_equal(_stat_got(r), want, STAT_KEYS, f"nb {nb}, ratio {ratio}")
        again = f.remove_statistical_outlier(pts, lengths, nb_neighbors=nb, std_ratio=ratio)
        _assert_equal(_stat_got(again), _stat_got(r), STAT_KEYS, f"nb {nb}, ratio {ratio}: second call")
        if first is None:
            first = want
            assert want["num_kept"][:3].tolist() == [0, 1, 2]  # n_f = 0, 1, 2: thresholds 0, 0 and mean + 0 * std
            assert (want["num_kept"][3:] < STAT_LENGTHS[3:]).all() and (want["num_kept"][3:] > 0.3 * STAT_LENGTHS[3:]).all()
        else:
            assert (want["num_kept"] >= first["num_kept"]).all() and want["num_kept"].sum() > first["num_kept"].sum()


def test_statistical_on_three_chunks_of_the_tree(dev, monkeypatch):
    """8200 rows: three chunks of 4096, the last one short."""
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts = np.stack([ref.uniform_scene(400, 8200), ref.uniform_scene(401, 8200)])
    lengths = np.array([8200, 4097], np.int64)
    r = f.remove_statistical_outlier(torch.from_numpy(pts).to(dev), torch.from_numpy(lengths).to(dev), nb_neighbors=8,
                                     std_ratio=1.0)
    want = _stat_want(ref.knn_table(pts, lengths, 9), lengths, 1.0)
    _assert_equal(_stat_got(r), want, STAT_KEYS, "8200 rows")


@pytest.mark.parametrize("side,nb", [(8, 1), (8, 3), (10, 3)])
def test_a_lattice_keeps_every_point(dev, monkeypatch, side, nb):
    """Every point of a cubic lattice has `nb` <= 3 neighbours at exactly the step (a power of two), so every m_i is
    the step, the mean is the step, std is 0 and threshold == m_i: `<=` keeps them all, at std_ratio = 0 too."""
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts = torch.from_numpy(ref.lattice_scene(side)[None]).to(dev)
    for ratio in (0.0, 2.0):
        r = f.remove_statistical_outlier(pts, nb_neighbors=nb, std_ratio=ratio)
        assert r.num_kept.tolist() == [side ** 3] and bool(r.mask.all())
        assert r.threshold.tolist() == [0.125] and r.mean.tolist() == [0.125] and r.std.tolist() == [0.0]
        assert bool((r.mean_distance == 0.125).all())
        assert r.index[0].tolist() == list(range(side ** 3))


def test_a_cloud_alone_equals_the_cloud_in_a_batch(dev, monkeypatch):
    """The summation tree does not depend on N: the rows of cloud 2 of a batch of five are the rows of the cloud alone."""
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    P = 5000  # two chunks
    pts = np.stack([ref.uniform_scene(500 + n, P) for n in range(5)])
    lengths = np.array([P, 17, 4999, 0, 4096], np.int64)
    batch = f.remove_statistical_outlier(torch.from_numpy(pts).to(dev), torch.from_numpy(lengths).to(dev),
                                         nb_neighbors=8, std_ratio=1.0)
    for n in (0, 2, 4):
        alone = f.remove_statistical_outlier(torch.from_numpy(pts[n:n + 1]).to(dev),
                                             torch.from_numpy(lengths[n:n + 1]).to(dev), nb_neighbors=8, std_ratio=1.0)
        _assert_equal(_stat_got(alone), {k: v[n:n + 1] for k, v in _stat_got(batch).items()}, STAT_KEYS, f"cloud {n}")
    assert 0 < int(batch.num_kept[2]) < 4999


# ------------------------------------------------------------------------------------------------ compaction
def _masks(P):
    rng = np.random.default_rng(P)
    return np.stack([np.ones(P, bool), np.zeros(P, bool), np.arange(P) % 2 == 0, np.arange(P) % 2 == 1,
                     rng.uniform(size=P) < 0.5, rng.uniform(size=P) < 0.01])


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1024, 1025, 70000])
def test_mask_to_index_equals_the_checker_and_keypoints_to_padded(dev, monkeypatch, P):
    from pytorch3d_pointops_amd import functions as f

    mask = _masks(P)
    M = torch.from_numpy(mask).to(dev)
    (index, num), c = _guarded(monkeypatch, lambda: f.mask_to_index(M), mask=M)
    assert [b.kind for b in c.buffers] == ["out"] * 2 and not c.rejections  # no workspace
    want_index, want_num = ref.compact(mask)
    _assert_equal(dict(index=index.cpu().numpy(), num_kept=num.cpu().numpy()), dict(index=want_index, num_kept=want_num),
                  ("index", "num_kept"), f"P = {P}")
    idx, n = f.keypoints_to_padded(M)
    kmax = idx.shape[1]
    assert torch.equal(n, num) and torch.equal(index[:, :kmax], idx) and bool((index[:, kmax:] == -1).all())


def _featured(dev, P=700):
    pts = np.stack([ref.outlier_scene(600 + n, P) for n in range(3)])
    lengths = [700, 513, 0]
    T = lambda a, n: torch.from_numpy(np.ascontiguousarray(a[n, :lengths[n]])).to(dev)  # noqa: E731
    colors = np.random.default_rng(6).uniform(size=(3, P, 4)).astype(np.float32)
    ids = np.arange(3 * P, dtype=np.float32).reshape(3, P, 1)
    from pytorch3d_pointops_amd.structures import Pointclouds

    return Pointclouds([T(pts, n) for n in range(3)],
                       {"colors": [T(colors, n) for n in range(3)], "ids": [T(ids, n) for n in range(3)]})


@pytest.mark.parametrize("which", ["radius", "statistical"])
def test_select_rows_and_pointclouds_methods_carry_features(dev, monkeypatch, which):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pc = _featured(dev)
    if which == "radius":
        new, r = pc.remove_radius_outlier(radius=0.1, min_neighbors=3)
        direct = f.remove_radius_outlier(pc.points_padded(), pc.num_points_per_cloud(), radius=0.1, min_neighbors=3)
    else:
        new, r = pc.remove_statistical_outlier(nb_neighbors=8, std_ratio=1.0)
        direct = f.remove_statistical_outlier(pc.points_padded(), pc.num_points_per_cloud(), nb_neighbors=8, std_ratio=1.0)
    assert torch.equal(direct.mask, r.mask) and torch.equal(direct.index, r.index)
    assert new.num_points_per_cloud().tolist() == r.num_kept.tolist() and 0 < r.num_kept[0] < 700 and r.num_kept[2] == 0
    assert not bool(r.mask[0, 7])  # the far outlier goes
    sel = f.select_rows(pc.points_padded(), r.index, r.num_kept, pc.features_padded())
    one = f.select_rows(pc.points_padded(), r.index, r.num_kept, pc.get_features_padded("ids"))
    assert sel.points.shape[1] == int(r.num_kept.max()) and torch.equal(one.features, sel.features["ids"])
    assert sorted(new.feature_names()) == ["colors", "ids"]
    for n in range(3):
        keep = r.mask[n, :int(pc.num_points_per_cloud()[n])]
        k = int(r.num_kept[n])
        assert torch.equal(new.points_list()[n], pc.points_list()[n][keep])
        assert torch.equal(sel.points[n, :k], pc.points_list()[n][keep]) and not bool(sel.points[n, k:].any())
        for name in ("colors", "ids"):
            assert torch.equal(new.get_features_list(name)[n], pc.get_features_list(name)[n][keep])
            assert torch.equal(sel.features[name][n, :k], pc.get_features_list(name)[n][keep])
    assert f.select_rows(pc.points_padded(), r.index, r.num_kept).features is None


# ------------------------------------------------------------------------------------------------ contract
@pytest.mark.parametrize("fill", buffers.FILLS)
def test_statistical_entry_under_every_fill(dev, monkeypatch, fill):
    """zero / ones / stale (what a sibling call on another table with full lengths left behind): the outputs are the same
    bytes, padding rows included; the table and the lengths are untouched."""
    from pytorch3d_pointops_amd import _C_filters

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    table = _stat_table(8)
    D, L = torch.from_numpy(table).to(dev), torch.from_numpy(STAT_LENGTHS).to(dev)
    S = torch.from_numpy(np.ascontiguousarray(table[::-1])).to(dev)
    out, c = _guarded(monkeypatch, lambda: _C_filters.statistical_outlier(D, L, 1.0), fill=fill,
                      sibling=lambda: _C_filters.statistical_outlier(S, None, 1.0), dists=D, lengths=L)
    assert [b.kind for b in c.buffers] == ["out"] * 6 + ["workspace"] and c.inputs_checked >= 2
    if fill == "ones":
        assert {(n, how) for n, _, how in c.rejections} == {(STAT_ENTRY, "short"), (STAT_ENTRY, "null")}
    mask, index, num_kept, md, thr, stats = (t.cpu().numpy() for t in out)
    want = ref.statistical_from_dists(table, STAT_LENGTHS, 1.0)
    _assert_equal(dict(mask=mask, index=index, num_kept=num_kept, mean_distance=md, threshold=thr, stats=stats), want,
                  ("mask", "index", "num_kept", "mean_distance", "threshold", "stats"), f"[{fill}]")


@pytest.mark.parametrize("fill", ["zero", "stale"])
def test_radius_entry_under_the_other_fills(dev, monkeypatch, fill):
    from pytorch3d_pointops_amd import _C_filters

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    name = "outlier-D3-mn5"
    pts, lengths, radius, mn = CASES[name]
    X, L = torch.from_numpy(pts).to(dev), torch.from_numpy(lengths).to(dev)
    S = torch.from_numpy(np.ascontiguousarray(pts[::-1])).to(dev)
    out, c = _guarded(monkeypatch, lambda: _C_filters.radius_outlier(X, L, radius, mn, want_counts=True), fill=fill,
                      sibling=lambda: _C_filters.radius_outlier(S, None, radius, mn, want_counts=True), points=X,
                      lengths=L)
    assert [b.kind for b in c.buffers] == ["out"] * 4 + ["workspace"] and c.inputs_checked >= 2
    _assert_equal({k: t.cpu().numpy() for k, t in zip(cases.KEYS, out)}, _want_radius(name), cases.KEYS, f"[{fill}]")


def test_empty_batches_and_empty_clouds(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    for N, P in ((0, 5), (0, 0), (4, 0)):
        X = torch.zeros((N, P, 3), device=dev)
        r = f.remove_radius_outlier(X, radius=0.1, min_neighbors=1, return_counts=True)
        assert r.mask.shape == (N, P) and r.index.shape == (N, P) and r.counts.shape == (N, P)
        assert r.num_kept.tolist() == [0] * N
        s = f.remove_statistical_outlier(X, nb_neighbors=4)
        assert s.mask.shape == (N, P) and s.mean_distance.shape == (N, P) and s.num_kept.tolist() == [0] * N
        assert s.threshold.tolist() == [0.0] * N and s.mean.tolist() == [0.0] * N and s.std.tolist() == [0.0] * N
        index, num = f.mask_to_index(torch.zeros((N, P), dtype=torch.bool, device=dev))
        assert index.shape == (N, P) and num.tolist() == [0] * N
        sel = f.select_rows(X, r.index, r.num_kept)
        assert sel.points.shape == (N, 0, 3)


def _four_point_fold(v):
    """The documented tree for clouds of four rows: lanes 0..3 hold one row each, the fold's last two steps add lanes
    (0, 2) and (1, 3), then the two sums (every other addend is +0.0)."""
    return (v[:, 0] + v[:, 2]) + (v[:, 1] + v[:, 3])


def test_many_clouds_cross_the_slice_boundary(dev, monkeypatch):
    """65 540 clouds of 4 points go to each entry in two slices.  Every cloud is held to the definitions written out
    for four points; the first, last and boundary clouds also go through the checker."""
    from pytorch3d_pointops_amd import _C_filters
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    N, P, radius, mn, nb, ratio = 65540, 4, 0.5, 2, 2, 1.0
    pts = np.random.default_rng(77).uniform(0, 1, (N, P, 3)).astype(np.float32)
    lengths = np.random.default_rng(78).integers(0, P + 1, N).astype(np.int64)
    lengths[[0, 65534, 65535, 65536, N - 1]] = P
    X, L = torch.from_numpy(pts).to(dev), torch.from_numpy(lengths).to(dev)
    pick = [0, 1, 2, 65533, 65534, 65535, 65536, 65537, N - 2, N - 1]
    valid = np.arange(P)[None, :] < lengths[:, None]
    pair = valid[:, :, None] & valid[:, None, :]
    d = pts[:, :, None, :] - pts[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    got, c = _guarded(monkeypatch, lambda: _C_filters.radius_outlier(X, L, radius, mn, want_counts=True), points=X,
                      lengths=L)
    assert len(c.rejections) == 4  # two native calls
    got = {k: t.cpu().numpy() for k, t in zip(cases.KEYS, got)}
    counts = ((d2 < np.float32(radius) * np.float32(radius)) & pair & ~np.eye(P, dtype=bool)).sum(2).astype(np.int32)
    mask = valid & (counts >= mn)
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["mask"], mask) and 1000 < mask.sum() < valid.sum()
    index, num = ref.compact(mask)
    assert np.array_equal(got["index"], index) and np.array_equal(got["num_kept"], num)
    _assert_equal({k: v[pick] for k, v in got.items()}, ref.radius(pts[pick], lengths[pick], radius, mn), cases.KEYS,
                  "picked clouds, radius")

    r = f.remove_statistical_outlier(X, L, nb_neighbors=nb, std_ratio=ratio)
    table = np.sort(np.where(pair, d2, np.float32(np.inf)), axis=2)[..., :nb + 1]
    cnt = np.minimum(nb + 1, lengths)
    s = np.zeros((N, P))
    for k in range(nb + 1):
        s = s + np.where(k < cnt[:, None], np.sqrt(np.where(np.isfinite(table[..., k]), table[..., k], 0).astype(np.float64)), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(valid & (cnt[:, None] >= 2), s / (cnt[:, None] - 1.0), 0.0).astype(np.float32)
    nf = lengths.astype(np.float64)
    m64 = m.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(nf > 0, _four_point_fold(m64) / nf, 0.0)
        dev2 = np.where(valid, (m64 - mean[:, None]) * (m64 - mean[:, None]), 0.0)
        std = np.where(nf >= 2, np.sqrt(_four_point_fold(dev2) / (nf - 1.0)), 0.0)
    thr = (mean + np.float64(np.float32(ratio)) * std).astype(np.float32)
    smask = valid & (m <= thr[:, None])
    sindex, snum = ref.compact(smask)
    want = dict(mask=smask, num_kept=snum, index=sindex, mean_distance=m, threshold=thr, mean=mean, std=std)
    _assert_equal(_stat_got(r), want, STAT_KEYS, "every cloud, statistical")
    assert 1000 < smask.sum() < valid.sum()
    picked = _stat_want(ref.knn_table(pts[pick], lengths[pick], nb + 1), lengths[pick], ratio)
    _assert_equal({k: v[pick] for k, v in _stat_got(r).items()}, picked, STAT_KEYS, "picked clouds, statistical")

    big = torch.from_numpy(smask).to(dev)
    bi, bn = f.mask_to_index(big)
    assert np.array_equal(bi.cpu().numpy(), sindex) and np.array_equal(bn.cpu().numpy(), snum)


def test_a_side_stream_gives_the_same_bytes(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    name = "outlier-D3-mn5"
    pts, lengths, radius, mn = CASES[name]
    X, L = torch.from_numpy(pts).to(dev), torch.from_numpy(lengths).to(dev)
    table = _stat_table(8)
    SP, SL = torch.from_numpy(_stat_points()).to(dev), torch.from_numpy(STAT_LENGTHS).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        r = f.remove_radius_outlier(X, L, radius=radius, min_neighbors=mn, return_counts=True)
        s = f.remove_statistical_outlier(SP, SL, nb_neighbors=8, std_ratio=1.0)
        index, num = f.mask_to_index(s.mask)
    side.synchronize()
    _assert_equal({k: getattr(r, k).cpu().numpy() for k in cases.KEYS}, _want_radius(name), cases.KEYS, "radius")
    _assert_equal(_stat_got(s), _stat_want(table, STAT_LENGTHS, 1.0), STAT_KEYS, "statistical")
    assert torch.equal(index, s.index) and torch.equal(num, s.num_kept)


def test_graph_capture_replays_the_eager_result(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd import graphs

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts, lengths, radius, mn = CASES["outlier-D3-mn5"]
    L = torch.from_numpy(lengths).to(dev)

    def call(a):
        r = f.remove_radius_outlier(a, L, radius=radius, min_neighbors=mn, return_counts=True)
        s = f.remove_statistical_outlier(a, L, nb_neighbors=8, std_ratio=1.0)
        return tuple(r) + tuple(s) + f.mask_to_index(s.mask)

    X = torch.from_numpy(pts).to(dev)
    want = call(X)
    step = graphs.capture(call, (X.clone(),))
    assert all(torch.equal(a, b) for a, b in zip(step(), want))
    X2 = torch.from_numpy(np.ascontiguousarray(pts[::-1, ::-1])).to(dev)  # a second scene through the static input
    want2 = call(X2)
    assert not torch.equal(want2[0], want[0])
    assert all(torch.equal(a, b) for a, b in zip(step(X2), want2))
    _assert_equal({k: t.cpu().numpy() for k, t in zip(("mask", "num_kept", "index", "counts"), want2[:4])},
                  ref.radius(np.ascontiguousarray(pts[::-1, ::-1]), lengths, radius, mn), cases.KEYS, "second scene")


def test_bad_native_arguments_are_rejected_with_nothing_written(dev):
    from pytorch3d_pointops_amd import _C

    X = torch.rand(1, 8, 3, device=dev)
    D = torch.rand(1, 8, 4, device=dev)
    outs = [torch.full((1024,), 7, dtype=torch.uint8, device=dev) for _ in range(6)]
    ws = torch.zeros(max(_C._lib.pointops_radius_outlier_workspace_bytes(1, 8),
                         _C._lib.pointops_statistical_outlier_workspace_bytes(1, 8)), dtype=torch.uint8, device=dev)
    assert _C._lib.pointops_radius_outlier_workspace_bytes(65536, 8) == 0
    assert _C._lib.pointops_statistical_outlier_workspace_bytes(1, 2 ** 24 + 1) == 0
    for bad in (dict(r=0.0), dict(r=-1.0), dict(r=float("inf")), dict(r=float("nan")), dict(mn=-1), dict(D=0), dict(D=4),
                dict(N=65536), dict(P=2 ** 30), dict(N=-1)):
        a = dict(r=0.1, mn=2, N=1, P=8, D=3)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.radius_outlier("radius_outlier", dev, X, None, a["N"], a["P"], a["D"], a["r"], a["mn"], *outs[:4],
                                    ws, ws.numel())
    for bad in (dict(K1=1), dict(K1=129), dict(ratio=-0.5), dict(ratio=float("inf")), dict(ratio=float("nan")),
                dict(N=65536), dict(P=2 ** 24 + 1)):
        a = dict(ratio=1.0, N=1, P=8, K1=4)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.statistical_outlier("statistical_outlier", dev, D, None, a["N"], a["P"], a["K1"], a["ratio"],
                                         *outs, ws, ws.numel())
    for N, P in ((65536, 8), (1, 2 ** 30), (-1, 8)):
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.mask_compact("mask_compact", dev, outs[0], N, P, outs[1], outs[2])
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
