"""The numpy checker of voxel_downsample (tests/voxel_ref.py) against a second, independent restatement of the
definition: a Python dict keyed by the integer cell triple, filled row by row the way Open3D's unordered_map algorithm
works, with Python floats for the cell (IEEE doubles, one operation at a time) and fractions.Fraction for the means
(exact).  No GPU, no library call: what the GPU tests compare against is itself pinned here, case by case."""
import math
from fractions import Fraction

import numpy as np
import pytest

import voxel_ref as ref


def by_dict(points, length, v, features=None, origin=None):
    """One cloud -> (status, [(cell (x, y, z), [rows], centroid, pooled)] in voxel order)."""
    v = float(np.float32(v))
    P = len(points)
    live = [i for i in range(min(max(int(length), 0), P)) if all(math.isfinite(float(c)) for c in points[i])]
    if not live:
        return 0, []
    mn = [min(np.float32(points[i][a]) for i in live) for a in range(3)]
    mx = [max(np.float32(points[i][a]) for i in live) for a in range(3)]
    o = [float(np.float32(origin[a])) if origin is not None else float(mn[a]) - 0.5 * v for a in range(3)]
    if not all(math.isfinite(x) for x in o):
        return 1, []  # (cells of infinite magnitude, or NaN, which fails every "fits" comparison)
    cell = lambda x, a: math.floor((float(x) - o[a]) / v)  # noqa: E731  (a Python int: no range to fall out of)
    for a in range(3):
        c_lo, c_hi = cell(mn[a], a), cell(mx[a], a)
        if c_hi - c_lo >= 2 ** 21 or abs(c_lo) >= 2 ** 31 or abs(c_hi) >= 2 ** 31:
            return 1, []
    voxels = {}
    for i in live:  # ascending row index
        voxels.setdefault(tuple(cell(points[i][a], a) for a in range(3)), []).append(i)
    out = []
    for key in sorted(voxels, key=lambda k: (k[2], k[1], k[0])):
        rows = voxels[key]
        mean = lambda vals: float(sum((Fraction(float(x)) for x in vals), Fraction(0)) / len(vals))  # noqa: E731
        centroid = [mean([points[i][a] for i in rows]) for a in range(3)]
        pooled = None if features is None else [mean([features[i][k] for i in rows]) for k in range(features.shape[1])]
        out.append((key, rows, centroid, pooled))
    return 0, out


def check(points, lengths, v, features=None, origin=None):
    """Both restatements agree on every output of every cloud; returns the checker's result."""
    points = np.asarray(points, np.float32)
    if points.ndim == 2:
        points = points[None]
        features = None if features is None else np.asarray(features, np.float32)[None]
    N, P = points.shape[:2]
    got = ref.downsample(points, lengths, v, features, origin)
    for n in range(N):
        o = None if origin is None else np.asarray(origin, np.float32).reshape(-1, 3)[n if np.ndim(origin) == 2 else 0]
        status, voxels = by_dict(points[n], P if lengths is None else lengths[n], v,
                                 None if features is None else features[n], o)
        V = len(voxels)
        assert got["status"][n] == status and got["num_voxels"][n] == V
        inverse = np.full(P, -1, np.int64)
        for r, (key, rows, centroid, pooled) in enumerate(voxels):
            inverse[rows] = r
            assert got["counts"][n, r] == len(rows) and got["first_index"][n, r] == rows[0]
            assert got["coords"][n, r].tolist() == list(key)
            # fsum / n and the exact quotient rounded once differ by the division's half ulp at most
            assert np.allclose(got["centroids"][n, r], centroid, rtol=2.0 ** -52, atol=0.0)
            if pooled is not None:
                assert np.allclose(got["pooled"][n, r], pooled, rtol=2.0 ** -52, atol=0.0)
        assert np.array_equal(got["inverse"][n], inverse)
        assert not got["counts"][n, V:].any() and (got["first_index"][n, V:] == -1).all()
        assert not got["coords"][n, V:].any() and not got["centroids"][n, V:].any()
    return got


def test_a_single_point():
    got = check([[0.3, -0.2, 7.0]], None, 0.5)
    assert got["num_voxels"].tolist() == [1] and got["coords"][0, 0].tolist() == [0, 0, 0]  # (the default origin)
    assert got["centroids"][0, 0].tolist() == [float(np.float32(x)) for x in (0.3, -0.2, 7.0)]


def test_all_points_in_one_voxel_and_one_point_per_voxel():
    pts = ref.blobs(1, 200)
    feats = np.random.default_rng(2).normal(size=(200, 3)).astype(np.float32)
    got = check(pts, None, 100.0, feats)
    assert got["num_voxels"].tolist() == [1] and got["counts"][0, 0] == 200 and not got["inverse"].any()
    got = check(pts, None, 1e-6, feats)
    assert got["num_voxels"].tolist() == [200] and (got["counts"][0] == 1).all()
    assert np.array_equal(got["centroids"][0][got["inverse"][0]], pts.astype(np.float64))  # a point is its own mean
    assert sorted(got["inverse"][0].tolist()) == list(range(200))


def test_a_point_on_a_face_goes_to_the_upper_cell():
    v = 0.25
    pts = np.array([[0.0, 0.0, 0.0], [0.25, 0.5, 0.75], [0.2499999, 0.5, 0.75], [-0.25, -0.0, 1.0], [1.0, 1.0, 1.0]],
                   np.float32)
    got = check(pts, None, v, origin=np.zeros(3, np.float32))
    want = {0: (0, 0, 0), 1: (1, 2, 3), 2: (0, 2, 3), 3: (-1, 0, 4), 4: (4, 4, 4)}
    for row, cell in want.items():
        assert got["coords"][0, got["inverse"][0, row]].tolist() == list(cell)


def test_negative_coordinates_with_an_explicit_origin_and_the_default_rule():
    pts = (ref.blobs(3, 300) - np.float32(0.5)) * np.float32(4.0)
    got = check(pts, None, 0.3, origin=np.array([0.1, -0.2, 0.3], np.float32))
    assert (got["coords"][0, : got["num_voxels"][0]] < 0).any() and (got["coords"][0] > 0).any()
    # the default rule: the lowest cell of every axis is 0, the smallest point sits half a voxel inside it
    got = check(np.stack([pts, pts + np.float32(10.0)]), [300, 250], 0.3)
    for n in range(2):
        assert got["coords"][n, : got["num_voxels"][n]].min(0).tolist() == [0, 0, 0]
    # and one origin per cloud
    check(np.stack([pts, pts]), None, 0.3, origin=np.array([[0, 0, 0], [0.15, 0.15, 0.15]], np.float32))


def test_duplicated_points_and_non_finite_rows():
    base = ref.blobs(4, 50)
    pts = np.concatenate([base, base, base[:7]])
    got = check(pts, None, 0.05)
    assert got["counts"][0].sum() == 107 and (got["counts"][0, : got["num_voxels"][0]] >= 2).all()
    pts = ref.blobs(5, 40)
    pts[3, 1], pts[11, 0], pts[12, 2], pts[39] = np.nan, np.inf, -np.inf, np.nan
    got = check(np.stack([pts, np.full_like(pts, np.nan)]), [40, 40], 0.1)
    assert (got["inverse"][0, [3, 11, 12, 39]] == -1).all() and (np.delete(got["inverse"][0], [3, 11, 12, 39]) >= 0).all()
    assert got["num_voxels"][1] == 0 and got["status"].tolist() == [0, 0]  # no live row: empty, not refused
    check(pts, [0], 0.1)
    check(pts, [-3], 0.1)
    check(pts, [1000], 0.1)


def test_the_extent_rule_at_its_edge_in_python_integers():
    z = np.zeros(3, np.float32)
    near = np.array([[0.5, 0.5, 0.5], [2.0 ** 21 - 0.5, 0.5, 0.5]], np.float32)  # cells 0 and 2^21 - 1
    far = np.array([[0.5, 0.5, 0.5], [2.0 ** 21 + 0.5, 0.5, 0.5]], np.float32)   # cells 0 and 2^21
    assert math.floor(float(near[1, 0])) == 2 ** 21 - 1 and math.floor(float(far[1, 0])) == 2 ** 21
    got = check(near, None, 1.0, origin=z)
    assert got["status"].tolist() == [0] and got["coords"][0, 1].tolist() == [2 ** 21 - 1, 0, 0]
    got = check(far, None, 1.0, origin=z)
    assert got["status"].tolist() == [1] and got["num_voxels"].tolist() == [0] and (got["inverse"] == -1).all()
    # the magnitude rule: |c| = 2^31 - 1 passes, 2^31 does not.  x = 2^31 - 256 is a float32 number; the origin moves
    # x - o (exact in float64) to 2^31 - 0.5 or to 2^31
    pts = np.array([[2.0 ** 31 - 256, 0.5, 0.5], [2.0 ** 31 - 1280, 0.5, 0.5]], np.float32)
    assert float(pts[0, 0]) == 2 ** 31 - 256
    origin = lambda x: np.array([x, 0, 0], np.float32)  # noqa: E731
    got = check(pts, None, 1.0, origin=origin(-255.5))
    assert got["status"].tolist() == [0] and got["coords"][0, 1, 0] == 2 ** 31 - 1
    assert check(pts, None, 1.0, origin=origin(-256.0))["status"].tolist() == [1]
    got = check(-pts, None, 1.0, origin=origin(255.0))
    assert got["status"].tolist() == [0] and got["coords"][0, 0, 0] == -(2 ** 31 - 1)
    assert check(-pts, None, 1.0, origin=origin(255.5))["status"].tolist() == [1]
    # a far outlier between clean clouds, and a non-finite origin
    clean = ref.blobs(6, 30)
    out = clean.copy()
    out[7] = 1e30
    got = check(np.stack([clean, out, clean]), None, 1e-3)
    assert got["status"].tolist() == [0, 1, 0] and np.array_equal(got["inverse"][0], got["inverse"][2])
    assert check(clean, None, 0.1, origin=np.array([0, np.nan, 0], np.float32))["status"].tolist() == [1]
    assert check(np.array([[3.4e38, 0, 0], [-3.4e38, 0, 0]], np.float32), None, 1e-45)["status"].tolist() == [1]


def test_the_voxel_order_is_z_then_y_then_x():
    pts = np.array([[2.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 0.5, 1.5], [0.5, 0.5, 0.5]], np.float32)
    got = check(pts, None, 1.0, origin=np.zeros(3, np.float32))
    assert got["coords"][0].tolist() == [[0, 0, 0], [2, 0, 0], [0, 1, 0], [1, 0, 1]]
    assert got["inverse"][0].tolist() == [1, 2, 3, 0]
    by_xyz = sorted(range(4), key=lambda i: tuple(pts[i]))
    assert [int(got["inverse"][0, i]) for i in by_xyz] != [0, 1, 2, 3]  # sorting by (x, y, z) numbers them otherwise


@pytest.mark.parametrize("seed", range(4))
def test_random_ragged_batches_with_features(seed):
    rng = np.random.default_rng(seed)
    pts = np.stack([ref.blobs(10 * seed + n, 257) for n in range(3)])
    feats = rng.normal(size=(3, 257, 5)).astype(np.float32)
    got = check(pts, [257, 100, 0], [0.02, 0.07, 0.3, 5.0][seed], feats)
    m = ref.exact_means(pts, got["inverse"], got["num_voxels"])
    assert np.array_equal(m, got["centroids"])
    assert (ref.mean_bound(pts, got["inverse"], got["counts"], m)[got["counts"] > 0] > 0).all()
