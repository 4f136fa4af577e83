"""CPU suite of segment_plane: the checker (tests/plane_ref.py) on hand cases, the validity tests, the sign rule and the
cone at their edges, the reachability of what the GPU suite asserts on its scenes -- computed by the checker alone --,
the argument validation of the two public functions, and the per-lane routines of csrc/plane_hypothesis.h with the
fp64 eigen core of csrc/small_solvers.h as a native host program (tests/native/plane_hypothesis_main.cpp, plain and
under the host sanitizers; nothing is loaded into Python)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import plane_ref as ref
from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "plane_hypothesis_main.cpp")


# ------------------------------------------------------------------------------------------------ hand cases
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("z, inside", [(0.25, True), (0.25 - 2.0 ** -24, True), (0.25 + 2.0 ** -23, False)],
                         ids=["on", "inside", "outside"])
def test_hand_case_threshold(z, inside, dtype):
    """The plane z = 0 from three points of it, thr = 0.25: a fourth point at height z is in at 0.25 and at
    0.25 - 2^-24, out at 0.25 + 2^-23 (all three are fp32 numbers).  Every product and sum is exact: r = z."""
    X = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, z], [0, 0, 5]]], np.float32)
    assert float(X[0, 3, 2]) == z
    samples = np.array([[[0, 1, 2], [2, 2, 1], [0, 1, 7], [0, 1, 4]]], np.int64)
    r = ref.run(X, thr=0.25, samples=samples, refine_steps=0, dtype=dtype)
    assert r["valid"].tolist() == [[True, False, False, True]]  # a repeated row, a row outside the cloud
    assert np.array_equal(r["hyp"][0, 0], np.array([0, 0, 1, 0], np.float32))
    assert not r["hyp"][0, 1].any() and not r["hyp"][0, 2].any()
    want = 4 if inside else 3
    # (the fourth triple spans y = 0, which holds its own three rows: a tie with the outside case, lost to index 0)
    assert r["counts"][0].tolist() == [want, -1, -1, 3] and r["best"][0] == 0 and r["num_inliers"][0] == want
    assert r["mask"][0].tolist() == [True, True, True, inside, False]
    assert r["rmse"][0] == pytest.approx(np.sqrt(z * z / 4) if inside else 0.0, abs=1e-9)


def test_degenerate_triples_are_invalid_and_the_cloud_gets_the_zero_plane():
    nan = np.float32(np.nan)
    collinear = np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6], [0.5, 1, 1.5]], np.float32)
    coincident = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]], np.float32)
    two_same = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]], np.float32)
    with_nan = np.array([[0, 0, 0], [1, 0, 0], [0, nan, 0], [nan, nan, nan]], np.float32)
    X = np.stack([collinear, coincident, two_same, with_nan])
    samples = np.array([[[0, 1, 2], [1, 2, 3], [0, 2, 3], [3, 2, 1]]] * 4, np.int64)
    for dtype in (np.float32, np.float64):
        r = ref.run(X, thr=0.1, samples=samples, refine_steps=2, dtype=dtype)
        assert not r["valid"].any() and (r["counts"] == -1).all() and r["best"].tolist() == [-1] * 4
        assert not r["hyp"].any() and np.isfinite(r["hyp"]).all()
        assert not r["planes"].any() and not r["mask"].any() and not r["num_inliers"].any() and not r["rmse"].any()
    # drawn from an all-collinear cloud: the same
    line = (np.arange(50, dtype=np.float32)[:, None] * np.array([1, 2, 3], np.float32))[None]
    r = ref.run(line, thr=0.1, H=64, dtype=np.float32)
    assert (r["samples"] >= 0).all() and not r["valid"].any() and r["best"][0] == -1 and not r["planes"].any()
    # the test is relative: the same triangle at 1e-15 and at 1e+15 is as valid as at 1
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    for scale in (1e-15, 1.0, 1e15):
        _, valid, _ = ref.planes_of(tri * np.float32(scale), np.array([True]))
        assert valid.all()


def test_fewer_than_three_valid_rows_draw_nothing():
    X = np.random.default_rng(0).uniform(size=(3, 6, 3)).astype(np.float32)
    mask = np.zeros((3, 6), bool)
    mask[1, :2] = True
    r = ref.run(X, np.array([6, 6, 0]), mask, H=8, dtype=np.float32)
    assert (r["samples"] == -1).all() and (r["counts"] == -1).all() and r["best"].tolist() == [-1] * 3
    assert not r["planes"].any() and not r["mask"].any()


def test_sign_rule():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)  # e1 x e2 = +z
    flipped = tri[[0, 2, 1]]                                       # e1 x e2 = -z
    for t in (tri, flipped):
        pl, valid, _ = ref.planes_of(t[None], np.array([True]))
        assert valid[0] and np.array_equal(pl[0], np.array([0, 0, 1, 0], np.float32))
    # with an axis the normal follows it, also against the largest component
    down = ref.cone_of((0.0, 0.0, -1.0), 30.0)
    for t in (tri, flipped):
        pl, valid, _ = ref.planes_of(t[None] + np.float32(2.0), np.array([True]), down)
        assert valid[0] and np.array_equal(pl[0], np.array([0, 0, -1, 2], np.float32))
    # a tie in magnitude: the lowest index decides.  Normal along +-(1, -1, 0) / sqrt 2 -> the x component is positive
    tie = np.array([[0, 0, 0], [1, 1, 0], [0, 0, 1]], np.float32)
    for t in (tie, tie[[0, 2, 1]]):
        pl, valid, _ = ref.planes_of(t[None], np.array([True]))
        assert valid[0] and pl[0, 0] > 0 and pl[0, 0] == -pl[0, 1] and pl[0, 2] == 0
    n, d = ref.orient(np.array([[-0.5, 0.5, -0.5], [0.5, -0.5, -0.5], [-0.1, -0.7, 0.7]]), np.array([1.0, 1.0, 1.0]), None)
    assert n.tolist() == [[0.5, -0.5, 0.5], [0.5, -0.5, -0.5], [0.1, 0.7, -0.7]] and d.tolist() == [-1.0, 1.0, -1.0]


def test_cone_at_exactly_the_boundary():
    """max_angle 45 degrees about z: cos^2 is the float32 square root of a half, squared in float64.  The normal of the
    triangle below is (0, -t, 1): (c.A)^2 = 1 against cos^2 (1 + t^2): in iff t^2 <= 1 / cos^2 - 1, decided in float64
    by multiplies and adds alone.  A cone of 0 degrees (cos = 1) holds exactly the axis, 90 degrees everything."""
    cone = ref.cone_of((0.0, 0.0, 2.0), 45.0)
    assert cone[0].tolist() == [0.0, 0.0, 1.0] and cone[1] == np.float32(np.sqrt(0.5))
    c2 = float(cone[1]) ** 2
    for t in (0.5, 1.0 - 2.0 ** -20, 1.0, 1.0 + 2.0 ** -20, 2.0):
        t = float(np.float32(t))
        tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, t]]], np.float32)
        _, valid, _ = ref.planes_of(tri, np.array([True]), cone)
        assert bool(valid[0]) == (1.0 >= c2 * (1.0 + t * t)), t
    flat = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    lean = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 2.0 ** -10]]], np.float32)
    exact = ref.cone_of((0.0, 0.0, 1.0), 0.0)
    assert ref.planes_of(flat, np.array([True]), exact)[1][0] and not ref.planes_of(lean, np.array([True]), exact)[1][0]
    wall = np.array([[[0, 0, 0], [1, 0, 0], [0, 0, 1]]], np.float32)
    assert ref.planes_of(wall, np.array([True]), ref.cone_of((0.0, 0.0, 1.0), 90.0))[1][0]
    assert not ref.planes_of(wall, np.array([True]), ref.cone_of((0.0, 0.0, 1.0), 89.0))[1][0]


def test_refit_is_the_least_squares_plane_and_is_rejected_when_it_loses_rows():
    X, samples, thr = ref.rejected_refit_scene()
    for dtype in (np.float32, np.float64):
        r = ref.run(X, thr=thr, samples=samples, refine_steps=3, dtype=dtype)
        assert r["accepted"].tolist() == [0] and r["num_inliers"].tolist() == [9]
        assert np.array_equal(r["planes"][0], np.array([0, 0, 1, 0], np.float32))
        fit, ok, _ = ref.fit_mask(X, r["mask"])
        d = np.abs(ref.residual(fit[0], X[0], np.float64))
        assert ok[0] and (d > thr).sum() == 1 and np.abs(d - thr).min() > 0.05 * thr
    # an accepted chain: a noisy patch is refitted to its least-squares plane
    sc, kw = ref.make_scene("p257")
    r = ref.run(sc["X"], dtype=np.float64, **kw)
    assert r["accepted"][0] >= 1
    fit, _ = ref.planted_fit(sc)
    assert np.abs(r["planes"][0] - fit[0]).max() < 1e-6


# ------------------------------------------------------------------------------------------------ reachability
def _reach(sc, kw):
    worst_in, best_out = ref.scene_margins(sc)
    assert worst_in <= 0.25 and best_out >= 4.0, (worst_in, best_out)
    r64 = ref.run(sc["X"], sc["len"], sc["mask"], dtype=np.float64, **kw)
    planted = sc["planted"].sum(1)
    n = np.arange(len(planted))
    assert np.array_equal(r64["counts"][n, r64["best"]], planted), (r64["counts"].max(1), planted)
    assert np.array_equal(r64["mask"], sc["planted"])
    r32 = ref.run(sc["X"], sc["len"], sc["mask"], dtype=np.float32, **kw)
    assert np.array_equal(r32["counts"], r64["counts"]) and np.array_equal(r32["mask"], r64["mask"])
    _, lam = ref.planted_fit(sc)
    assert (lam[:, 1] >= 0.01 * lam[:, 2]).all()  # the planted patch is no sliver: its fit is well conditioned
    return r64


@pytest.mark.parametrize("name", [k for k, v in ref.SCENES.items() if v.get("planted", True)])
def test_gpu_scene_is_reachable(name):
    """What tests/test_plane_gpu.py asserts on its scenes, established by the checker alone: planted rows lie within
    0.25 thr and every other valid row beyond 4 thr of the planted plane; the float64 winner counts exactly the planted
    set and its refined mask is the planted set; the float32 counts equal the float64 counts on every hypothesis (no
    row sits on the threshold); the planted patch has lambda_1 >= 0.01 lambda_2."""
    sc, kw = ref.make_scene(name)
    _reach(sc, kw)


def test_cone_outside_scene_loses_the_floor():
    sc, kw = ref.cone_outside_scene()
    free = ref.run(sc["X"], dtype=np.float64, **dict(kw, axis=None, max_angle_deg=None))
    assert np.array_equal(free["mask"], sc["planted"])
    for dtype in (np.float32, np.float64):
        r = ref.run(sc["X"], dtype=dtype, **kw)
        assert r["valid"].sum() < free["valid"].sum() and r["num_inliers"][0] < 0.2 * sc["planted"].sum()
        assert r["best"][0] < 0 or r["planes"][0, 2] >= np.cos(np.radians(10.0)) - 1e-6


def test_chunk_scenes_have_the_sizes_they_are_named_for():
    from pytorch3d_pointops_amd import _C_plane

    c = _C_plane.PLANE_CHUNK
    assert c == ref.CHUNK
    for name, want in (("chunk-1", c - 1), ("chunk", c), ("chunk+1", c + 1), ("2chunk+1", 2 * c + 1)):
        sc, _ = ref.make_scene(name)
        assert ref.valid_rows(sc["len"], sc["mask"], *sc["X"].shape[:2]).sum() == want, name


def planes_scene():
    """The scene of the GPU suite's segment_planes test: a floor of 1500 rows, a wall of 900, a shelf of 150 and 450
    rows of clutter well off all three; (X (1,3000,3), labels (1,3000), thr)."""
    rng = np.random.default_rng(7400)
    thr = 0.02
    parts = [(np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, 0.0]), 1500, 1.0),
             (np.array([1.0, 0.0, 0.0]), np.array([-0.6, 0.0, 0.55]), 900, 1.0),
             (np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.7, 0.8]), 150, 0.4)]
    pts, labels = [], []
    for k, (nrm, centre, count, aspect) in enumerate(parts):
        pts.append(ref.scatter_on_plane(rng, count, nrm, centre, thr, aspect=aspect))
        labels.append(np.full(count, k))
    clutter = rng.uniform(-0.45, 0.45, (450, 3)) * np.array([1.0, 1.0, 0.3]) + np.array([0.0, 0.0, 0.35])
    pts.append(clutter)
    labels.append(np.full(450, -1))
    order = rng.permutation(3000)
    return (np.concatenate(pts)[order][None].astype(np.float32), np.concatenate(labels)[order][None], thr)


def test_planes_scene_is_reachable():
    """Peeling by the checker alone: floor and wall come off in the order of their sizes with exactly their rows;
    whatever wins the third call holds fewer than 300 rows (the shelf has 150), so with min_inliers = 300 it does not
    count."""
    X, labels, thr = planes_scene()
    remaining = np.ones(labels.shape, bool)
    for k, want in enumerate((1500, 900)):
        r64 = ref.run(X, None, remaining, thr=thr, H=512, seed=40 + k, dtype=np.float64)
        r32 = ref.run(X, None, remaining, thr=thr, H=512, seed=40 + k, dtype=np.float32)
        assert np.array_equal(r64["mask"], labels == k) and r64["num_inliers"][0] == want
        assert np.array_equal(r32["mask"], r64["mask"]) and np.array_equal(r32["counts"], r64["counts"])
        remaining &= ~r64["mask"]
    for dtype in (np.float32, np.float64):
        assert ref.run(X, None, remaining, thr=thr, H=512, seed=42, dtype=dtype)["counts"].max() < 200


def test_floor_and_blobs_scene_is_reachable():
    """The end-to-end scene of the GPU suite by the two checkers alone: DBSCAN of everything is one cluster, the plane
    within 15 degrees of z holds exactly the floor, and DBSCAN of the rest is the three blobs with no noise."""
    import cluster_ref

    X, floor, eps, min_points, thr = ref.floor_and_blobs_scene()
    labels, num, _ = cluster_ref.dbscan(X, None, eps, min_points)
    assert num.tolist() == [1] and (labels >= 0).all()
    for dtype in (np.float32, np.float64):
        r = ref.run(X, thr=thr, H=256, seed=3, axis=(0, 0, 1), max_angle_deg=15.0, dtype=dtype)
        assert np.array_equal(r["mask"], floor) and r["planes"][0, 2] > 0.999
    rest = X[:, ~floor[0]]
    labels, num, _ = cluster_ref.dbscan(rest, None, eps, min_points)
    assert num.tolist() == [3] and (labels >= 0).all() and np.bincount(labels[0]).tolist() == [160] * 3


# ------------------------------------------------------------------------------------------------ the public functions
def test_exports():
    from pytorch3d_pointops_amd import functions
    from pytorch3d_pointops_amd.structures import Pointclouds

    assert {"segment_plane", "segment_planes", "PlaneSegmentation", "PlaneSet"} <= set(functions.__all__)
    assert functions.PlaneSegmentation._fields == ("planes", "inliers", "num_inliers", "rmse", "best", "counts",
                                                   "hypotheses", "samples")
    assert functions.PlaneSet._fields == ("planes", "labels", "num_inliers")
    assert callable(Pointclouds.segment_plane)


def test_validation_errors():
    from pytorch3d_pointops_amd.functions import segment_plane, segment_planes

    X = torch.rand(2, 8, 3)
    for fn, lead in ((segment_plane, ()), (segment_planes, (2,))):
        extra = dict(min_inliers=3) if lead else {}

        def call(points=X, **kw):
            a = dict(distance_threshold=0.1, **extra)
            a.update(kw)
            return fn(points, *lead, **a)

        with pytest.raises(TypeError):
            fn(X, *lead, **extra)  # distance_threshold is required
        with pytest.raises(ValueError, match=r"shape \(N, P, 3\)"):
            call(X[0])
        with pytest.raises(ValueError, match=r"shape \(N, P, 3\)"):
            call(X[..., :2])
        with pytest.raises(ValueError, match="float32"):
            call(X.double())
        with pytest.raises(ValueError, match=r"mask must be a bool tensor of shape \(N, P\)"):
            call(mask=torch.ones(2, 8))
        with pytest.raises(ValueError, match=r"mask must be a bool tensor of shape \(N, P\)"):
            call(mask=torch.ones(2, 7, dtype=torch.bool))
        with pytest.raises(ValueError, match=r"samples must be an int64 tensor of shape \(N, H, 3\)"):
            call(samples=torch.zeros(2, 4, 2, dtype=torch.int64))
        with pytest.raises(ValueError, match=r"samples must be an int64 tensor of shape \(N, H, 3\)"):
            call(samples=torch.zeros(2, 4, 3, dtype=torch.int32))
        with pytest.raises(ValueError, match="num_hypotheses"):
            call(num_hypotheses=0)
        with pytest.raises(ValueError, match="num_hypotheses"):
            call(num_hypotheses=(1 << 24) + 1)
        for bad in (-1.0, float("nan"), float("inf"), 1e39):
            with pytest.raises(ValueError, match="distance_threshold"):
                call(distance_threshold=bad)
        with pytest.raises(ValueError, match="refine_steps"):
            call(refine_steps=-1)
        with pytest.raises(ValueError, match="seed"):
            call(seed=-1)
        with pytest.raises(ValueError, match="come together"):
            call(axis=(0, 0, 1))
        with pytest.raises(ValueError, match="come together"):
            call(max_angle_deg=10.0)
        with pytest.raises(ValueError, match="axis must be three finite numbers"):
            call(axis=(0, 0, 0), max_angle_deg=10.0)
        with pytest.raises(ValueError, match="axis must be three finite numbers"):
            call(axis=(0, 1), max_angle_deg=10.0)
        with pytest.raises(ValueError, match="max_angle_deg"):
            call(axis=(0, 0, 1), max_angle_deg=91.0)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="max_planes"):
        segment_planes(X, 0, min_inliers=3, distance_threshold=0.1)
    with pytest.raises(ValueError, match="min_inliers"):
        segment_planes(X, 2, min_inliers=-1, distance_threshold=0.1)
    with pytest.raises(ValueError, match="below 2\\^63"):
        segment_planes(X, 2, min_inliers=3, distance_threshold=0.1, seed=2 ** 63 - 1)


def test_workspace_sizer_and_shape_limits():
    from pytorch3d_pointops_amd import _C

    size = _C._lib.pointops_plane_workspace_bytes
    assert size(2, 1000, 64) > 2 * 1000 * 16 and size(1, 0, 1) > 0
    assert size(2, 1000, 128) > size(2, 1000, 64) and size(4, 1000, 64) > size(2, 1000, 64)
    assert size(65536, 4, 4) == 0 and size(1, 4, 0) == 0 and size(1, 4, (1 << 24) + 1) == 0
    assert size(1, 65535 * ref.CHUNK + 1, 1) == 0


# ------------------------------------------------------------------------------------------------ native program
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_plane_routines_hold_their_bounds(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "plane_hypothesis")
    extra = ["-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] \
        if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout
