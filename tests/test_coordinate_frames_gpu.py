"""Search kernels on signed, shifted and rescaled coordinates (frames: tests/frames.py), bit for bit.

Every other bit-exact test feeds the kernels non-negative coordinates of order one, yet the grid code branches on sign,
magnitude and exponent (ordered keys, cell_of's cast and clamps, face bounds, degenerate extents, the FLT_MAX and -1
sentinels of FPS, radius^2).  Here every operator path runs a base case in every frame:
  exact frames    idx identical to the untransformed call, dists bit-equal up to the exact factor (tests/
                  test_coordinate_frames_cpu.py proves the reference behaves so); the untransformed call itself is
                  checked against the oracle,
  inexact frames  bit-equal to the oracle on the transformed inputs, or -- beyond `_ORACLE_PAIRS` distance pairs, where
                  the oracle takes seconds -- to the brute-force family (version 0) of the library, itself pinned by
                  the oracle in every frame by the "brute" paths below.
Paths are forced with the POINTOPS_DEBUG knobs and `version` arguments of the tests named next to each, and the path
taken is asserted from the grid statistics, in every frame, where the library reports it (`_PATH_EXCEPTIONS` names the
frames whose geometry keeps the queries off a path, and why); otherwise the dispatch predicate is cited.
Bases off the 2^-24 grid (powers of uniforms) are quantised to it, so that shifts stay exact."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import cases
import frames
import test_gpu_parity as parity
from conftest import GOLDEN, bits
from test_gpu_parity import G, close

pytestmark = pytest.mark.gpu

# The untransformed call of every base is checked against the oracle up to 5e8 distance pairs (about two seconds of one
# CPU core, once per base).  The runs in inexact frames -- nine per base -- go to the oracle up to 6e7 pairs (a fraction
# of a second each) and beyond that to the library's version 0, to keep this file a minority of the suite's time;
# version 0 itself is held to the oracle in every frame by the brute_v0 and knn_wide paths (K up to 100, D = 3 included).
_ORACLE_BASE_PAIRS = 5e8
_ORACLE_PAIRS = 6e7
_CACHE = {}


def bits0(a):
    """Gradients: -0 and +0 compare equal (an exactly zero entry keeps +0 under a negation, see the CPU file)."""
    return bits(np.asarray(a, np.float32) + np.float32(0.0))


def _env(monkeypatch, knob):
    if knob:
        monkeypatch.setenv("POINTOPS_DEBUG", knob)
    else:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


_SELF_NAMES = {"ties_lattice_k16", "boundary_lattice"}  # cases.py hands the SAME array over as p1 and p2


# (path, frame) pairs whose geometry legitimately keeps the queries off the path: the test ID carries the label, the run
# asserts what happens instead (test_knn_long_lists_in_frames), and the results are still compared bit for bit.
_PATH_EXCEPTIONS = {
    # the outlier stretches the points' box a thousandfold while the cell COUNT follows the point count, so the unit
    # cube is one cell; its 30000 records are more than the wave sort streams (16384) and every query takes the
    # all-pairs list
    ("wave_sort", "outlier-1e3"): "all_pairs",
    # every query lies outside the points' box, further from it than the K-th neighbour's cube reaches: no cube
    # certifies and every query takes the all-pairs list
    ("wave_sort", "opposite_signs"): "all_pairs",
}


def _params(table, self_paths=()):
    """[(path, base, frame)] for {path: (base getter, base names)}.  Bases named "lattice" sit on a grid of 0.125 or
    coarser and also take the large integer shifts; self-queries leave out the frame that needs two clouds."""
    out = []
    for path, (_, names) in table.items():
        for name in names:
            self_query = path in self_paths or name in _SELF_NAMES
            for f in frames.frames_for(lattice="lattice" in name, self_query=self_query):
                label = _PATH_EXCEPTIONS.get((path, f.name))
                out.append(pytest.param(path, name, f, id=f"{path}{'~' + label if label else ''}-{name}-{f.name}"))
    return out


# ------------------------------------------------------------------------------------------------ knn_points
def _knn_gpu(dev, b, p1, p2, version, stats=None):
    from pytorch3d_pointops_amd import _C

    t1 = G(p1, dev)
    t2 = t1 if p2 is p1 else G(p2, dev)
    l1 = G(b["l1"], dev)
    # a self-query hands the same tensor OBJECTS over (one sort); a base with one cloud but two lengths (cases.py's
    # ties_lattice_k16) keeps both, as the test it is named after does
    l2 = l1 if (p2 is p1 and b["l2"] is b["l1"]) else G(b["l2"], dev)
    if stats == "stats":
        i, d, st = _C.knn_grid_stats(t1, t2, l1, l2, b["norm"], b["K"])
    elif stats == "counts":
        i, d, st = _C.knn_grid_fallback_counts(t1, t2, l1, l2, b["norm"], b["K"])
    else:
        i, d = _C.knn_points_idx(t1, t2, l1, l2, b["norm"], b["K"], version)
        st = None
    return i.cpu().numpy(), d.cpu().numpy(), None if st is None else st.cpu().numpy()


def _knn_want(dev, oracle, b, p1, p2, limit=_ORACLE_PAIRS):
    """The reference semantics on these inputs: the oracle, or the library's version 0 beyond `limit` pairs."""
    if float(np.sum(b["l1"] * b["l2"])) <= limit:
        return oracle.knn_points_idx(p1, p2, b["l1"], b["l2"], b["norm"], b["K"])
    assert "POINTOPS_DEBUG" not in os.environ
    i, d, _ = _knn_gpu(dev, b, p1, p2.copy() if p2 is p1 else p2, 0)
    return i, d


def _check_knn(dev, oracle, monkeypatch, path, name, b, frame, knob, version, stats=None, stat_check=None):
    what = (path, name, frame.name)

    def base():
        _env(monkeypatch, knob)
        i, d, _ = _knn_gpu(dev, b, b["p1"], b["p2"], version, stats)
        _env(monkeypatch, "")
        wi, wd = _knn_want(dev, oracle, b, b["p1"], b["p2"], _ORACLE_BASE_PAIRS)
        assert np.array_equal(i, wi) and np.array_equal(bits(d), bits(wd)), (path, name, "untransformed")
        return i, d

    bi, bd = _cached((path, name), base)
    q1, q2 = frame.apply(b["p1"], b["p2"])
    _env(monkeypatch, knob)
    i, d, st = _knn_gpu(dev, b, q1, q2, version, stats)
    _env(monkeypatch, "")
    if stat_check is not None:  # the path is asserted in EVERY frame, before the results
        print(what, "G", st[:, :3].tolist(), "ncell", st[:, 3].tolist(), "grid", st[:, 4].tolist(), "uncertified",
              st[:, 5:8].tolist(), "box", st[:, 8].tolist(), "refined", st[:, 9].tolist())
        stat_check(st, what, frame, dict(b, p1=q1, p2=q2))
    if frame.exact:
        assert np.array_equal(i, bi), what
        assert np.array_equal(bits(d), bits(bd * frame.dist_factor(b["norm"]))), what
    else:
        wi, wd = _knn_want(dev, oracle, b, q1, q2)
        assert np.array_equal(i, wi), what
        assert np.array_equal(bits(d), bits(wd)), what


def _case_base(name):
    c = cases.knn_cases()[name]
    return dict(p1=c["p1"], p2=c["p2"], l1=c["l1"], l2=c["l2"], K=c["K"], norm=c["norm"])


def _adversarial_base(name):
    """_grid_adversarial_cases of test_gpu_parity.py with the ragged lengths of test_knn_grid_adversarial."""
    def make():
        p1, p2, K = _cached("adversarial", parity._grid_adversarial_cases)[name]
        p1, p2 = frames.quantise(p1), frames.quantise(p2)
        return dict(p1=p1, p2=p2, l1=np.array([p1.shape[1], p1.shape[1] // 3]), l2=np.array([p2.shape[1], max(K - 2, 1)]),
                    K=K, norm=2)

    return _cached(("adv", name), make)


def _self_base(name):
    def make():
        b = _adversarial_base(name)
        return dict(b, p1=b["p2"], l1=b["l2"])  # (the same objects twice: a true self-query)

    return _cached(("self", name), make)


_BRUTE = {  # test_knn_versions_agree: versions 0 (LDS-transposed queries, knn_wide.hip) and 2 (register scan); the
    # wave-per-query kernel is kept out (knn_small=0) -- it has a path of its own below
    "brute_v0": (_case_base, ["ties_lattice_k16", "l1_k4"]),
    "scan_v2": (_case_base, ["ragged_k8", "l1_ties_k3"]),
}


@pytest.mark.parametrize("path,name,frame", _params(_BRUTE))
def test_knn_brute_force_in_frames(dev, oracle, monkeypatch, path, name, frame):
    _check_knn(dev, oracle, monkeypatch, path, name, _case_base(name), frame, "knn_small=0", 0 if path == "brute_v0" else 2)


_GRID = {  # test_knn_grid_alternative_passes: version 3 with the quad pass forced on / off, and the self-query
    "grid_quad": (_adversarial_base, ["clustered", "lattice_ties", "planar", "k32"]),
    "grid_lane": (_adversarial_base, ["lattice_ties", "half_in_cluster", "collinear", "k1", "d1"]),
    "grid_self": (_self_base, ["lattice_ties", "all_identical", "d2"]),
}


def _grid_used(st, what, frame, b):
    """Column 4 (use_grid): the setup pass of grid_build.hip gives every non-empty cloud with finite coordinates a grid
    -- one cell when it has no extent -- so it must be 1 for EVERY such cloud in every frame; column 3 (cells): the
    first cloud of a base with an extent must really be cut into cells."""
    assert (st[b["l2"] > 0, 4] == 1).all(), (what, st)
    extent = bool((b["p2"][0, : int(b["l2"][0])].max(0) > b["p2"][0, : int(b["l2"][0])].min(0)).any())
    assert (st[0, 3] > 1) == extent, (what, st)


@pytest.mark.parametrize("path,name,frame", _params(_GRID, self_paths=("grid_self",)))
def test_knn_grid_in_frames(dev, oracle, monkeypatch, path, name, frame):
    """Version 3 is the grid family whenever knn_check_version(3, D, K) holds (choose_version, knn.hip); the statistics
    confirm in EVERY frame that every non-empty cloud was searched through its grid and that the first cloud of a base
    with an extent was cut into more than one cell (`_grid_used`)."""
    from pytorch3d_pointops_amd import _C

    b = (_self_base if path == "grid_self" else _adversarial_base)(name)
    assert _C.knn_check_version(3, b["p1"].shape[2], b["K"])
    knob = {"grid_quad": "grid_quad=1", "grid_lane": "grid_quad=0", "grid_self": ""}[path]
    _check_knn(dev, oracle, monkeypatch, path, name, b, frame, knob, 3, stats="stats",
               stat_check=_grid_used)


def _zeros(x, rows=48):
    x[0, :rows, 0] = 0.0  # a few exact zeros: negations must carry -0.0 through this path too
    return x


def _long_base(name):
    def make():
        if name.startswith("box"):  # test_knn_grid_long_lists with grid_long_box=1
            K, norm = (40, 2) if name == "box_k40" else (64, 1)
            p1 = cases.cloud(2501, (4, 2500, 3))
            p2 = cases.cloud(2502, (4, 12000, 3))
            p2[1] = frames.quantise(p2[1] ** np.float32(3.0))  # clustered
            p2[3, :, :] = p2[3, :1, :]  # all identical: one cell, everything ties
            return dict(p1=_zeros(p1), p2=_zeros(p2), l1=np.array([2500, 2500, 900, 300]),
                        l2=np.array([12000, 7000, K - 3, 12000]), K=K, norm=norm)
        if name.startswith("refined"):  # test_knn_refined_cells_and_box_search
            K, norm = (8, 2) if name == "refined_k8" else (16, 1)
            m = 24000
            a = cases.cloud(2601, (3, 5000, 3))
            b = cases.cloud(2602, (3, m, 3))
            a[0, :2500] = a[0, :2500] * np.float32(1e-3) + np.float32(0.5)
            b[0, : m // 2] = b[0, : m // 2] * np.float32(1e-3) + np.float32(0.5)
            a[1], b[1] = frames.quantise(a[1] ** np.float32(5.0)), frames.quantise(b[1] ** np.float32(5.0))
            b[2, : m // 3] = b[2, 0]  # a third of the cloud is ONE point: every sub-cell index ties
            return dict(p1=frames.quantise(a), p2=frames.quantise(b), l1=np.array([5000, 5000, 1234]),
                        l2=np.array([m, m, m - 5]), K=K, norm=norm)
        K, norm, D = {"wsort_k100": (100, 2, 3), "wsort_k96_d2": (96, 2, 2)}[name]  # test_knn_grid_wave_sort_long_lists
        p1 = cases.cloud(3801, (4, 1500, D))
        p2 = cases.cloud(3802, (4, 30000, D))
        p2[1, :20000] = p2[1, :20000] * np.float32(3e-3) + np.float32(0.4)  # cluster: cubes with > 16384 records
        p2[2, 1::2] = p2[2, ::2]  # every point twice: ties in every list
        return dict(p1=_zeros(frames.quantise(p1)), p2=_zeros(frames.quantise(p2)), l1=np.array([1500, 1500, 1500, 40]),
                    l2=np.array([30000, 30000, 21000, K - 7]), K=K, norm=norm)

    return _cached(("long", name), make)


_LONG = {
    "box_search": (_long_base, ["box_k40"]),
    "refined_cells": (_long_base, ["refined_k8", "refined_k16_l1"]),
    "wave_sort": (_long_base, ["wsort_k100", "wsort_k96_d2"]),
}


# the path assertions of the long-list paths, from the grid statistics (also used by test_buffer_contract_gpu.py)
def _boxed(st, what, frame, fb):
    _grid_used(st, what, frame, fb)
    assert int(st[:2, 8].sum()) > 0, (what, st)  # queries handed to the box search, in every frame


def _refined(st, what, frame, fb):
    _grid_used(st, what, frame, fb)
    assert (st[:2, 9] > 0).all(), (what, st)  # refined cells: a property of the points, in every frame
    # queries deferred to the box search: those whose 3x3x3 cube is over-full.  With clouds of opposite sign every
    # query clamps into the corner cell of the points' box: that corner is where cloud 1 (u^5) is densest, while
    # cloud 0's cluster sits at the centre, out of the corner's cube -- cloud 0 defers nothing there.
    clouds = [1] if frame.name == "opposite_signs" else [0, 1]
    assert (st[clouds, 8] > 0).all(), (what, st)


def _wave_sorted(st, what, frame, fb):
    # test_knn_grid_wave_sort_long_lists: the cluster's neighbourhoods exceed what the kernel streams and end in the
    # all-pairs list (column 7 of cloud 1); every query of the uniform cloud 0 is certified by its cube (D = 3, L2:
    # the cells are sized for 3-D Euclidean balls; the planar frame's grid is rebuilt over two axes and keeps it)
    _grid_used(st, what, frame, fb)
    assert st[1, 7] > 0, (what, st)
    if ("wave_sort", frame.name) in _PATH_EXCEPTIONS:
        assert (st[:3, 7] == fb["l1"][:3]).all(), (what, st)  # what the exception claims: every query, all pairs
    elif fb["p1"].shape[2] == 3:
        assert st[0, 7] == 0, (what, st)


@pytest.mark.parametrize("path,name,frame", _params(_LONG))
def test_knn_long_lists_in_frames(dev, oracle, monkeypatch, path, name, frame):
    """box_search: K in (32, 64] with grid_long_box=1 -- statistics column 8 counts the queries handed to the box search;
    refined_cells: over-full cells are refined (column 9) and their queries deferred (column 8);
    wave_sort: 64 < K <= 128 is knn_grid_wsort.hip's range (run_grid_search, knn_grid.hip)."""
    b = _long_base(name)

    if path == "box_search":
        _check_knn(dev, oracle, monkeypatch, path, name, b, frame, "grid_long_box=1", 3, "stats", _boxed)
    elif path == "refined_cells":
        _check_knn(dev, oracle, monkeypatch, path, name, b, frame, "", 3, "stats", _refined)
    else:
        assert 64 < b["K"] <= 128
        _check_knn(dev, oracle, monkeypatch, path, name, b, frame, "", 3, "stats", _wave_sorted)


def _table_base(table, seed):
    def get(name):
        def make():
            N, P1, P2, D, K, norm, l1, l2 = table[name]
            p1, p2 = cases.cloud(seed + D, (N, P1, D)), cases.cloud(seed + 1 + D + K, (N, P2, D))
            if "lattice" in name:
                p1, p2 = cases.lattice(seed + 2, N, P1, D, levels=5), cases.lattice(seed + 3, N, P2, D, levels=5)
            if "identical" in name:
                p2[:] = np.float32(0.25)
            return dict(p1=p1, p2=p2, l1=np.array(l1), l2=np.array(l2), K=K, norm=norm)

        return _cached((seed, name), make)

    return get


_small_base = _table_base(parity._SMALL, 1900)
_wide_base = _table_base(parity._WIDE, 1700)

_SMALLP = {  # test_knn_small_batches: knn_small=1 and one query per wave / shared candidates
    "knn_small_q1": (_small_base, ["k4_long_lattice_gate_ties", "k32_long_cloud_gates"]),
    "knn_small_q2": (_small_base, ["k1_long_lattice_gate_ties_l1", "k1_l1"]),
}


@pytest.mark.parametrize("path,name,frame", _params(_SMALLP))
def test_knn_small_in_frames(dev, oracle, monkeypatch, path, name, frame):
    """knn_small=1 makes knn_small_applies() true for every D <= 8, K <= 32 batch of versions 1 / 2 (knn_small.hip)."""
    b = _small_base(name)
    assert b["p1"].shape[2] <= 8 and b["K"] <= 32
    _check_knn(dev, oracle, monkeypatch, path, name, b, frame, "knn_small=1,knn_small_q=" + path[-1], 2)


_WIDEP = {"knn_wide": (_wide_base, ["d16_k64", "d64_k20", "d3_k100"])}  # (d3_k100: version 0's long lists at D = 3)


@pytest.mark.parametrize("path,name,frame", _params(_WIDEP))
def test_knn_wide_in_frames(dev, oracle, monkeypatch, path, name, frame):
    """D > 8 or K > 32 on clouds below the grid's 4096 points leaves only version 0 (choose_version, knn.hip), whose
    plan is KnnFamily::kWide while knn_wide_supported(D, K) holds (knn_plan) -- test_knn_wide_shapes."""
    from pytorch3d_pointops_amd import _C

    b = _wide_base(name)
    assert not _C.knn_check_version(2, b["p1"].shape[2], b["K"]) and b["p2"].shape[1] < 4096
    _check_knn(dev, oracle, monkeypatch, path, name, _wide_base(name), frame, "", -1)


# ------------------------------------------------------------------------------------------------ ball_query
def _ball_base(name):
    def make():
        if name in cases.ball_query_cases():
            c = cases.ball_query_cases()[name]
            return dict(p1=c["p1"], p2=c["p2"], l1=c["l1"], l2=c["l2"], K=c["K"], radius=c["radius"])
        adv, K = name.rsplit("_k", 1)  # test_ball_query_grid_adversarial: radius 0.25 puts lattice distances ON radius^2
        b = _adversarial_base(adv)
        return dict(p1=b["p1"], p2=b["p2"], l1=b["l1"], l2=np.array([b["p2"].shape[1], 5]), K=int(K),
                    radius=0.25 if adv == "lattice_ties" else 0.06)

    return _cached(("ball", name), make)


_BALL_KNOBS = {  # test_ball_query / test_ball_query_grid_adversarial / test_fuzz_ball_query_grid_vs_scan
    "ball_scan": "ball_small=0,ball_grid=0",
    "ball_small": "ball_small=1,ball_grid=0",
    "ball_grid_staged": "ball_grid=1,ball_factor=0",
    "ball_grid_unstaged": "ball_grid=1,ball_factor=0,ball_stage=0",
    "ball_grid_storage_order": "ball_grid=1,ball_factor=0,ball_order=0",
}
_BALL = {
    "ball_scan": (_ball_base, ["boundary_lattice"]),
    "ball_small": (_ball_base, ["boundary_lattice", "ragged_r0.2"]),
    "ball_grid_staged": (_ball_base, ["lattice_ties_k4", "clustered_k20", "d2_k20"]),
    "ball_grid_unstaged": (_ball_base, ["half_in_cluster_k4"]),
    "ball_grid_storage_order": (_ball_base, ["lattice_ties_k4"]),
}


@pytest.mark.parametrize("path,name,frame", _params(_BALL))
def test_ball_query_in_frames(dev, oracle, monkeypatch, path, name, frame):
    """ball_grid=1 takes the grid for D <= 3, K <= 64 (ball_grid_candidate, ball_query.hip) and ball_factor=0 keeps the
    device from choosing the scan; hits are staged in LDS when K % 4 == 0 unless ball_stage=0 (pointops_ball_query)."""
    from pytorch3d_pointops_amd import _C

    b = _ball_base(name)
    what = (path, name, frame.name)
    if path.startswith("ball_grid"):
        assert b["p1"].shape[2] <= 3 and b["K"] <= 64 and b["K"] % 4 == 0

    def run(p1, p2, radius):
        _env(monkeypatch, _BALL_KNOBS[path])
        i, d = _C.ball_query(G(p1, dev), G(p2, dev), G(b["l1"], dev), G(b["l2"], dev), b["K"], radius)
        _env(monkeypatch, "")
        return i.cpu().numpy(), d.cpu().numpy()

    def base():
        i, d = run(b["p1"], b["p2"], b["radius"])
        wi, wd = oracle.ball_query(b["p1"], b["p2"], b["l1"], b["l2"], b["K"], b["radius"])
        assert np.array_equal(i, wi) and np.array_equal(bits(d), bits(wd)), (path, name, "untransformed")
        return i, d

    bi, bd = _cached((path, name), base)
    q1, q2 = frame.apply(b["p1"], b["p2"])
    if frame.exact:
        i, d = run(q1, q2, frame.radius(b["radius"]))
        assert np.array_equal(i, bi), what
        assert np.array_equal(bits(d), bits(bd * frame.dist_factor(2))), what
    else:
        radius = b["radius"] * frame.rscale
        i, d = run(q1, q2, radius)
        if float(np.sum(b["l1"] * b["l2"])) <= _ORACLE_PAIRS:
            wi, wd = oracle.ball_query(q1, q2, b["l1"], b["l2"], b["K"], radius)
        else:
            _env(monkeypatch, "ball_small=0,ball_grid=0")
            wi, wd = (t.cpu().numpy() for t in _C.ball_query(G(q1, dev), G(q2, dev), G(b["l1"], dev), G(b["l2"], dev),
                                                             b["K"], radius))
            _env(monkeypatch, "")
        assert np.array_equal(i, wi), what
        assert np.array_equal(bits(d), bits(wd)), what


# ------------------------------------------------------------------------------------------------ FPS
def _fps_base(name):
    def make():
        if name in cases.fps_cases():
            c = cases.fps_cases()[name]
            return dict(p1=c["points"], p2=c["points"], lengths=c["lengths"], K=c["K"], start=c["start"])
        N, P, D = {"multi_10000": (5, 10000, 3), "multi_40000": (3, 40000, 3), "multi_9000_d2": (3, 9000, 2)}[name]
        pts = cases.cloud(1400 + P, (N, P, D))  # test_fps_multi_workgroup_clusters
        pts[0, 100:200] = pts[0, 0:100]  # duplicates -> ties on the running min-distance
        pts = _zeros(pts)
        return dict(p1=pts, p2=pts, lengths=np.array([P, P // 2 + 7, min(4097, P), 5, P - 1][:N]),
                    K=np.array([64, 300, 17, 9, 128][:N]), start=np.array([0, 11, min(4096, P - 1), 4, P - 2][:N]))

    return _cached(("fps", name), make)


_FPS = {
    "fps_small": (_fps_base, ["per_cloud_k", "lattice_ties"]),  # P <= 4096: fps_single_kernel<.., 256> (fps.hip)
    "fps_clusters": (_fps_base, ["start_nonzero", "lattice_ties"]),  # fps_small=0: fps_single_kernel<.., 1024>
    "fps_multi_workgroup": (_fps_base, ["multi_10000", "multi_40000", "multi_9000_d2"]),  # P > 4096: clusters of workgroups
}


@pytest.mark.parametrize("path,name,frame", _params(_FPS, self_paths=tuple(_FPS)))
def test_sample_farthest_points_in_frames(dev, oracle, monkeypatch, path, name, frame):
    from pytorch3d_pointops_amd import _C

    b = _fps_base(name)
    P = b["p1"].shape[1]
    assert (P <= 4096) == (path != "fps_multi_workgroup")  # `P <= 16 * kFpsSmallBlock` of the launch (fps.hip)

    def run(pts):
        _env(monkeypatch, "fps_small=0" if path == "fps_clusters" else "")
        r = _C.sample_farthest_points(G(pts, dev), G(b["lengths"], dev), G(b["K"], dev), G(b["start"], dev))
        _env(monkeypatch, "")
        return r.cpu().numpy()

    def base():
        i = run(b["p1"])
        assert np.array_equal(i, oracle.sample_farthest_points(b["p1"], b["lengths"], b["K"], b["start"])), \
            (path, name, "untransformed")
        return i

    bi = _cached((path, name), base)
    q, _ = frame.apply(b["p1"])
    got = run(q)
    if frame.exact:
        assert np.array_equal(got, bi), (path, name, frame.name)
    else:
        assert np.array_equal(got, oracle.sample_farthest_points(q, b["lengths"], b["K"], b["start"])), \
            (path, name, frame.name)


# ------------------------------------------------------------------------------------------------ knn backward
def _close_rel(a, b):
    """close() of test_gpu_parity.py (1e-5 of max(1, max|b|)); gradients far below one are first brought to order one
    by an exact power of two, so that the bar keeps its meaning in the 2^-30 and 1e-18 frames (the error of a
    reordered fp32 sum is relative to the sum's terms)."""
    m = float(np.abs(b).max()) if np.asarray(b).size else 0.0
    s = 2.0 ** -np.floor(np.log2(m)) if 0.0 < m < 1.0 else 1.0
    return close(np.asarray(a, np.float64) * s, np.asarray(b, np.float64) * s)


def _bwd_base(name):
    def make():
        if name in cases.knn_backward_cases():
            return _case_base(name)
        D, norm, K = {"big_d3": (3, 2, 8), "big_d3_l1": (3, 1, 8), "big_d2": (2, 2, 3)}[name]  # test_knn_backward_modes
        N, P1, P2 = 3, 2500, 30000
        return dict(p1=cases.cloud(1500 + D, (N, P1, D)), p2=cases.cloud(1510 + D, (N, P2, D)),
                    l1=np.array([P1, 1777, 0]), l2=np.array([P2, 9001, 5]), K=K, norm=norm)

    return _cached(("bwd", name), make)


_BWD = {
    "bwd_deterministic": (_bwd_base, ["ties_lattice_k16", "l1_k4"]),
    "bwd_tiled": (_bwd_base, ["big_d3"]),
    "bwd_tiled_split3": (_bwd_base, ["big_d2"]),
    "bwd_atomic": (_bwd_base, ["big_d3_l1"]),
}


@pytest.mark.parametrize("path,name,frame", _params(_BWD))
def test_knn_backward_in_frames(dev, oracle, monkeypatch, path, name, frame):
    """deterministic=True (backward_det.hip): grad_p1 and grad_p2 bit for bit; knn_bwd_mode=tiled / atomic
    (test_knn_backward_modes): grad_p1 bit for bit, grad_p2 within close()."""
    from pytorch3d_pointops_amd import _C

    b = _bwd_base(name)
    D = b["p1"].shape[2]
    det = path == "bwd_deterministic"
    knob = {"bwd_deterministic": "", "bwd_tiled": "knn_bwd_mode=tiled", "bwd_tiled_split3": "knn_bwd_mode=tiled,knn_bwd_split=3",
            "bwd_atomic": "knn_bwd_mode=atomic"}[path]
    grad = cases.grad_for(name, (b["p1"].shape[0], b["p1"].shape[1], b["K"]))
    what = (path, name, frame.name)

    def run(p1, p2):
        args = (G(p1, dev), G(p2, dev), G(b["l1"], dev), G(b["l2"], dev))
        idx, _ = _C.knn_points_idx(*args, b["norm"], b["K"], -1)
        _env(monkeypatch, knob)
        g1, g2 = _C.knn_points_backward(*args, idx, b["norm"], G(grad, dev), deterministic=det)
        _env(monkeypatch, "")
        idx = idx.cpu().numpy()
        o1, o2 = oracle.knn_points_backward(p1, p2, b["l1"], b["l2"], idx, b["norm"], grad)
        g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
        # against the oracle's CPU loop on the same neighbour table, in this frame
        assert np.array_equal(bits(g1), bits(o1)), what
        assert np.array_equal(bits(g2), bits(o2)) if det else _close_rel(g2, o2), what
        return idx, g1, g2

    bidx, b1, b2 = _cached((path, name), lambda: run(b["p1"], b["p2"]))
    q1, q2 = frame.apply(b["p1"], b["p2"])
    idx, g1, g2 = run(q1, q2)
    if frame.exact:
        fac = frame.grad_factor(b["norm"], D)
        assert np.array_equal(idx, bidx), what
        assert np.array_equal(bits0(g1), bits0(b1 * fac)), what
        if det:
            assert np.array_equal(bits0(g2), bits0(b2 * fac)), what
        else:
            assert _close_rel(g2 / fac, b2), what  # (an exact division: +-2^k)


# ------------------------------------------------------------------------------------------------ chamfer
@pytest.mark.parametrize("frame", [f for f in frames.EXACT if f.k == 0 and not f.lattice_only], ids=repr)
def test_chamfer_pair_in_frames(dev, monkeypatch, frame):
    """The one-call bidirectional chamfer (the ragged case of test_chamfer_pair_native_vs_composed) under shifts and
    negations: the loss within 1e-5, grad_x / grad_y unchanged or negated on the negated axes within that test's 2e-5;
    the call count shows that the pair route ran."""
    import pytorch3d_pointops_amd.functions.chamfer as ch
    from test_chamfer_float64_gpu import _counting

    N, P1, P2 = 5, 700, 900
    l1, l2 = np.array([700, 1, 350, 699, 20]), np.array([900, 450, 1, 33, 899])
    x, y = cases.cloud(2101, (N, P1, 3)), cases.cloud(2102, (N, P2, 3))
    calls = _counting(monkeypatch)

    def run(x, y):
        for k in calls:
            calls[k] = 0
        tx, ty = G(x, dev).requires_grad_(True), G(y, dev).requires_grad_(True)
        loss, _ = ch.chamfer_distance(tx, ty, x_lengths=G(l1, dev), y_lengths=G(l2, dev), batch_reduction="mean",
                                      point_reduction="mean")
        loss.backward()
        assert (calls["pair"], calls["forward"], calls["composed"]) == (1, 0, 0), calls
        return float(loss.detach()), tx.grad.cpu().numpy(), ty.grad.cpu().numpy()

    base = run(x, y)
    got = run(*frame.apply(x, y))
    sign = frame.sign(3)
    assert close(got[0], base[0]), (frame.name, got[0], base[0])
    assert close(got[1] * sign, base[1], tol=2e-5) and close(got[2] * sign, base[2], tol=2e-5), frame.name


# ------------------------------------------------------------------------------------------------ full size
@pytest.mark.parametrize("frame", ["shift-0.5", "neg_all"])
def test_cfg2_cloud_digest_in_frames(dev, frame):
    """The cfg2-size cloud of tests/golden/big_meta.json as cloud - 0.5 and as -cloud: both reproduce the sha256 of idx
    and dists that the reference run pinned (test_cfg2_cloud_digest), with no new golden."""
    from pytorch3d_pointops_amd.functions import knn_points

    meta = json.load(open(os.path.join(GOLDEN, "big_meta.json")))["cfg2_cloud"]
    P, K = meta["P"], meta["K"]
    p1, p2 = frames.BY_NAME[frame].apply(cases.cloud(meta["seed1"], (1, P, 3)), cases.cloud(meta["seed2"], (1, P, 3)))
    assert (p1 < 0).any() and (p2 < 0).any()
    r = knn_points(G(p1, dev), G(p2, dev), K=K)
    idx32 = r.idx.cpu().numpy().astype(np.int32)
    assert hashlib.sha256(idx32.tobytes()).hexdigest() == meta["idx_sha256"], frame
    assert hashlib.sha256(r.dists.cpu().numpy().tobytes()).hexdigest() == meta["dists_sha256"], frame


def test_knn_huge_cloud_shifted(dev):
    """The 2 M-point clouds of test_knn_single_huge_cloud (21-bit run words) shifted by -0.5: bit-equal to the
    unshifted call."""
    from pytorch3d_pointops_amd import _C, synth

    P, K = 2_000_000, 16
    a, b = synth.uniform_f32(3601, (1, P, 3)), synth.uniform_f32(3602, (1, P, 3))
    L = torch.full((1,), P, dtype=torch.int64, device=dev)
    assert _C._lib.pointops_knn_uses_grid(1, P, P, 3, K, -1) == 1
    bi, bd = _C.knn_points_idx(G(a, dev), G(b, dev), L, L, 2, K, -1)
    sa, sb = frames.BY_NAME["shift-0.5"].apply(a, b)
    si, sd = _C.knn_points_idx(G(sa, dev), G(sb, dev), L, L, 2, K, -1)
    assert torch.equal(si, bi) and torch.equal(sd.view(torch.int32), bd.view(torch.int32))


# ------------------------------------------------------------------------------------------------ normals, registration
_DOWNSTREAM = {"centred_negated": lambda x: -(x - 0.5), "offset-1e3": lambda x: x - 1e3}


@pytest.mark.parametrize("frame", sorted(_DOWNSTREAM))
def test_normals_in_frames(dev, monkeypatch, frame):
    """test_against_float64_eigh of test_points_normals_gpu.py -- its float64 checker and its bars, computed on the
    transformed cloud -- on a centred and negated cloud and on one offset by -1e3 (no metamorphic identity: the
    neighbourhood means re-round)."""
    import test_points_normals_gpu as normals

    clouds, seen = normals._clouds, []

    def framed(*a):
        out = _DOWNSTREAM[frame](clouds(*a)).astype(np.float32)
        seen.append(out)
        return out

    monkeypatch.setattr(normals, "_clouds", framed)
    normals.test_against_float64_eigh(dev, "uniform", 16)
    assert len(seen) == 1 and (seen[0] < 0).any(), "the framed cloud did not reach the checker"


@pytest.mark.parametrize("frame", sorted(_DOWNSTREAM))
def test_registration_in_frames(dev, monkeypatch, frame):
    """test_icp_one_iteration_is_exact_composition of test_points_alignment_gpu.py (one search + one alignment against
    the float64 checker on the package's own neighbour table, its bars) with both clouds in the frame."""
    import test_points_alignment_gpu as align

    setup, seen = align._subset_setup, []

    def framed(*a, **kw):
        X, Y, lx, ly, truth = setup(*a, **kw)
        f = _DOWNSTREAM[frame]  # (the padding rows beyond lx / ly move too: they stay behind the masks)
        X, Y = f(X).float(), f(Y).float()
        seen.append((X, Y))
        return X, Y, lx, ly, truth

    monkeypatch.setattr(align, "_subset_setup", framed)
    align.test_icp_one_iteration_is_exact_composition(dev)
    assert len(seen) == 1 and bool((seen[0][0] < 0).any()) and bool((seen[0][1] < 0).any()), \
        "the framed clouds did not reach the checker"
