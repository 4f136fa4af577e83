"""The outlier filters without a GPU:

    native     tests/native/filter_stats_main.cpp -- csrc/filter_stats.h and nothing else of the library -- compiled with
               the hipcc and flags of pytorch3d_pointops_amd/build.py, once plain and once with the host sanitizers (UBSan
               + ASan on the host side only) as a program of its own: its m_i, statistics, threshold and mask equal
               tests/filters_ref.py bit for bit on seeded tables
    checker    filters_ref against a plain float64 evaluation (np.mean, np.std(ddof=1)); its tree against math.fsum; its
               radius mask against tests/cluster_ref.py's core mask; its compaction against np.flatnonzero
    arguments  the public functions refuse bad scalars, dtypes and shapes with ValueError, CPU tensors with RuntimeError
"""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import cluster_ref
import filters_ref as ref
from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "filter_stats_main.cpp")


def _table(seed, N, P, K1, scale=1.0):
    """(N, P, K1) float32: ascending squared distances with the row's own 0 first, as knn_points returns them."""
    rng = np.random.default_rng(seed)
    d = np.sort(rng.uniform(0.0, scale, (N, P, K1)).astype(np.float32) ** 2, axis=2)
    d[..., 0] = 0.0
    return d


def _lattice_table(N, P, K1, d2=0.015625):
    d = np.full((N, P, K1), d2, np.float32)
    d[..., 0] = 0.0
    return d


def _nonfinite_table():
    d = _table(5, 1, 300, 4)
    d[0, 17, 3] = np.inf
    d[0, 200, 2:] = np.nan
    return d


# name -> (dists, lengths or None, std_ratio)
TABLES = {
    "short-clouds": (_table(1, 4, 6, 5), [0, 1, 2, 6], 1.0),            # cnt < 2; n_f = 0, 1, 2
    "k1-above-len": (_table(2, 3, 40, 128), [3, 40, 127], 2.0),
    "around-256": (_table(3, 3, 257, 9), [255, 256, 257], 1.0),
    "two-chunks": (_table(4, 2, 5000, 3, scale=1e-3), [5000, 4097], 2.0),
    "ratio-0": (_table(6, 2, 700, 17), None, 0.0),
    "lattice": (_lattice_table(2, 1000, 7), [1000, 513], 0.0),          # all m_i equal: every row kept
    "lattice-ratio-2": (_lattice_table(1, 4100, 2, d2=0.1), None, 2.0),  # (0.1 is not a power of two: S1 / n_f rounds)
    "large-values": (_table(7, 1, 900, 31, scale=1e15), None, 1.0),
    "nonfinite": (_nonfinite_table(), None, 1.0),
    "empty": (np.zeros((2, 0, 4), np.float32), None, 1.0),
}


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "ubsan+asan"])
def program(request, tmp_path_factory):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("filter_stats") / "filter_stats")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] \
        if request.param else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    return exe


def _run_native(exe, tmp_path, dists, lengths, std_ratio):
    N, P, K1 = dists.shape
    L = np.full(N, P, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([N, P, K1], np.int64).tobytes() + np.float32(std_ratio).tobytes() + L.tobytes()
                + np.ascontiguousarray(dists, np.float32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    raw = open(dst, "rb").read()
    at = 0
    out = {}
    for key, dtype, shape in (("mean_distance", np.float32, (N, P)), ("stats", np.float64, (N, 3)),
                              ("threshold", np.float32, (N,)), ("mask", np.uint8, (N, P))):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out[key] = np.frombuffer(raw[at:at + n], dtype).reshape(shape)
        at += n
    assert at == len(raw)
    return out


@pytest.mark.parametrize("name", list(TABLES))
def test_header_arithmetic_equals_the_checker_bit_for_bit(program, tmp_path, name):
    dists, lengths, ratio = TABLES[name]
    got = _run_native(program, tmp_path, dists, lengths, ratio)
    want = ref.statistical_from_dists(dists, lengths, ratio)
    for key in ("mean_distance", "stats", "threshold"):
        assert got[key].tobytes() == want[key].tobytes(), f"{name}: {key} differs"
    assert np.array_equal(got["mask"] != 0, want["mask"]), f"{name}: mask"


def test_what_the_tables_are_meant_to_show():
    r = ref.statistical_from_dists(*TABLES["short-clouds"])
    assert r["stats"][:, 2].tolist() == [0.0, 1.0, 2.0, 6.0]
    assert r["stats"][0].tolist() == [0, 0, 0] and r["threshold"][0] == 0 and r["num_kept"][0] == 0
    assert r["mean_distance"][1, 0] == 0 and r["stats"][1].tolist() == [0, 0, 1] and r["num_kept"][1] == 1  # cnt < 2
    # two rows: std = |a - b| / sqrt(2) puts both within one std of the mean, which lies |a - b| / 2 from each
    assert r["stats"][2, 1] > 0 and r["num_kept"][2] == 2
    for name in ("lattice", "lattice-ratio-2"):
        r = ref.statistical_from_dists(*TABLES[name])
        L = ref._lengths(TABLES[name][1], *TABLES[name][0].shape[:2])
        assert r["num_kept"].tolist() == L.tolist(), name  # m_i <= threshold, not <
    r = ref.statistical_from_dists(*TABLES["ratio-0"])
    assert (0.3 * 700 < r["num_kept"]).all() and (r["num_kept"] < 0.7 * 700).all()  # the rows up to the mean
    assert (r["threshold"].astype(np.float64) == r["stats"][:, 0].astype(np.float32)).all()
    r = ref.statistical_from_dists(*TABLES["nonfinite"])
    assert r["stats"][0, 2] == 298 and not r["mask"][0, 17] and not r["mask"][0, 200] and np.isfinite(r["stats"]).all()
    assert np.isinf(r["mean_distance"][0, 17]) and np.isnan(r["mean_distance"][0, 200])


SEEDED = [(11, 3, 2000, 9, [2000, 1500, 37], 1.0), (12, 2, 5000, 17, None, 2.0), (13, 2, 900, 2, [900, 2], 0.5),
          (14, 1, 4096, 31, None, 0.0)]


@pytest.mark.parametrize("seed,N,P,K1,lengths,ratio", SEEDED)
def test_checker_equals_plain_float64(seed, N, P, K1, lengths, ratio):
    """The checker's prescribed roundings and summation order move m_i and the threshold by a few float32 ulps at
    most; a row's verdict may differ from the plain float64 one only when it lies that close to the threshold.  The
    seeds are chosen so that NO row does: the exemption hides nothing, the masks are simply equal."""
    dists = _table(seed, N, P, K1)
    got = ref.statistical_from_dists(dists, lengths, ratio)
    m, thr, mask = ref.statistical_float64(dists, lengths, ratio)
    L = ref._lengths(lengths, N, P)
    live = np.arange(P)[None, :] < L[:, None]
    near = live & (np.abs(m - thr[:, None]) <= 4 * 2.0 ** -24 * thr[:, None])
    assert int(near.sum()) == 0
    assert np.array_equal(got["mask"], mask)
    # and the quantities themselves: m_i is rounded once to float32 (2^-24 relative); moving every row by at most
    # e = 2^-24 max m moves the mean by at most e and the sample std by at most e sqrt(n / (n - 1)) <= 1.5 e; the float64
    # summations add a few 2^-53 per term, far below: 2 e bounds both
    assert (np.abs(got["mean_distance"] - m) <= 2.0 ** -24 * np.abs(m)).all()
    for n in range(N):
        rows = m[n, :L[n]]
        e = 2.0 ** -24 * rows.max()
        assert abs(got["stats"][n, 0] - rows.mean()) <= 2 * e
        if L[n] >= 2:
            assert abs(got["stats"][n, 1] - rows.std(ddof=1)) <= 2 * e


def test_tree_sum_against_fsum_and_the_order_it_documents():
    rng = np.random.default_rng(3)
    for P in (0, 1, 255, 256, 257, 4096, 4097, 10000):
        v = rng.uniform(0, 1, P)
        assert abs(ref.tree_sum(v) - math.fsum(v)) <= 2.0 ** -48 * max(math.fsum(v), 1.0)
    # the shape: rows t, t + 256, ... of a chunk are added first (one lane), then lanes t and t + 128, ...
    v = np.zeros(4096)
    v[[3, 3 + 256]] = (1.0, 2.0 ** -53)      # one lane: (0 + 1) + 2^-53 rounds back to 1 ...
    v[3 + 128] = 2.0 ** -53                  # ... and the neighbour lane's 2^-53 is lost against it as well
    assert ref.tree_sum(v) == 1.0
    v = np.zeros(4096)
    v[[3 + 128, 3 + 128 + 256]] = 2.0 ** -53  # the two small terms in ONE lane add up before they meet the 1
    v[3] = 1.0
    assert ref.tree_sum(v) == 1.0 + 2.0 ** -52
    assert ref.tree_sum(np.concatenate([v, v])) == 2.0 * (1.0 + 2.0 ** -52)  # chunks one after the other


@pytest.mark.parametrize("D", [1, 2, 3])
def test_radius_checker_equals_the_dbscan_checkers_core_mask(D):
    for seed, P, mn in ((1, 400, 0), (2, 700, 1), (3, 700, 5), (4, 300, 700)):
        p = np.stack([ref.uniform_scene(seed, P, D), ref.slab_scene(seed, P, D), ref.outlier_scene(seed, P, D)])
        lengths = np.array([P, P // 2 + 1, P])
        got = ref.radius(p, lengths, 0.1, mn)
        _, _, core = cluster_ref.dbscan(p, lengths, 0.1, mn + 1)
        assert np.array_equal(got["mask"], core)
        assert not got["mask"][2, 7] or mn == 0  # the far outlier has no neighbour
        assert got["counts"][2, 7] == 0 and (got["counts"][:, :P // 2] > 0).any()
    # a pair at exactly the radius is not a pair (0.25 - 0 = 0.25, squared 0.0625 = fl32(0.25 * 0.25))
    pair = np.zeros((1, 2, D), np.float32)
    pair[0, 1, 0] = 0.25
    assert ref.radius(pair, None, 0.25, 1)["counts"].tolist() == [[0, 0]]
    assert ref.radius(pair, None, np.nextafter(np.float32(0.25), np.float32(1)), 1)["counts"].tolist() == [[1, 1]]


def test_compaction_checker():
    rng = np.random.default_rng(5)
    mask = rng.uniform(size=(4, 300)) < np.array([0.0, 1.0, 0.5, 0.1])[:, None]
    index, num = ref.compact(mask)
    for n in range(4):
        rows = np.flatnonzero(mask[n])
        assert num[n] == len(rows) and index[n].tolist() == rows.tolist() + [-1] * (300 - len(rows))


def test_public_functions_refuse_bad_arguments():
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd.structures import Pointclouds

    X = torch.rand(2, 8, 3)
    kw = dict(radius=0.1, min_neighbors=2)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")),
                dict(radius=1e39), dict(radius="wide"), dict(min_neighbors=-1), dict(min_neighbors=2.5),
                dict(min_neighbors=float("nan")), dict(min_neighbors=None)):
        with pytest.raises(ValueError):
            f.remove_radius_outlier(X, **{**kw, **bad})
    for bad in (dict(nb_neighbors=0), dict(nb_neighbors=128), dict(nb_neighbors=1.5), dict(std_ratio=-0.5),
                dict(std_ratio=float("inf")), dict(std_ratio=float("nan")), dict(std_ratio=1e39)):
        with pytest.raises(ValueError):
            f.remove_statistical_outlier(X, **bad)
    for pts, lengths in ((torch.rand(2, 8, 4), None), (X.double(), None), (X[0], None), (X.numpy(), None),
                         (X, torch.tensor([8, 8, 8])), (X, torch.tensor([8, 8], dtype=torch.int32)), (X, [8, 8]),
                         (Pointclouds(X), torch.tensor([8, 8]))):
        with pytest.raises(ValueError):
            f.remove_radius_outlier(pts, lengths, **kw)
        with pytest.raises(ValueError):
            f.remove_statistical_outlier(pts, lengths)
    for bad in (torch.zeros(2, 3), torch.zeros(6, dtype=torch.bool), [[True]]):
        with pytest.raises(ValueError):
            f.mask_to_index(bad)
    index, num = torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    for args in ((X[0], index, num), (X, index.int(), num), (X, index[:, :4], num), (X, index, num[:1]),
                 (X, index, num.float()), (X, index, num, torch.rand(2, 7, 3)), (X, index, num, {"a": torch.rand(2, 8)})):
        with pytest.raises(ValueError):
            f.select_rows(*args)


def test_no_cpu_implementation():
    from pytorch3d_pointops_amd import _C_filters
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd.structures import Pointclouds

    X = torch.rand(2, 8, 3)
    for call in (lambda: f.remove_radius_outlier(X, radius=0.1, min_neighbors=2),
                 lambda: f.remove_statistical_outlier(X, nb_neighbors=3),
                 lambda: f.remove_statistical_outlier(torch.zeros(2, 0, 3)),
                 lambda: f.mask_to_index(torch.zeros(2, 8, dtype=torch.bool)),
                 lambda: Pointclouds(X).remove_radius_outlier(radius=0.1, min_neighbors=2),
                 lambda: Pointclouds(X).remove_statistical_outlier(),
                 lambda: _C_filters.statistical_outlier(torch.zeros(2, 8, 4), None, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert {"RadiusOutliers", "StatisticalOutliers", "remove_radius_outlier", "remove_statistical_outlier",
            "mask_to_index", "select_rows"} <= set(f.__all__)
    # select_rows is plain indexing: it runs wherever its tensors live
    mask = torch.tensor([[True, False, True, True], [False, False, False, True]])
    index, num = (torch.from_numpy(a) for a in ref.compact(mask.numpy()))
    P = torch.arange(24, dtype=torch.float32).reshape(2, 4, 3)
    sel = f.select_rows(P, index, num, {"c": P[..., :1] * 2})
    assert sel.points.shape == (2, 3, 3) and sel.lengths.tolist() == [3, 1]
    assert torch.equal(sel.points[0], P[0][mask[0]]) and torch.equal(sel.points[1, :1], P[1][mask[1]])
    assert not sel.points[1, 1:].any() and torch.equal(sel.features["c"][0], 2 * P[0][mask[0]][:, :1])
