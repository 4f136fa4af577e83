"""voxel_downsample on the GPU against the numpy checker of tests/voxel_ref.py, stage by stage, so that no stage hides
another:

    integers   num_voxels, status, inverse, counts, first_index, coords EQUAL the checker's (the definition fixes them)
    means      centroids and pooled features within the derived bound of the exact mean m of the members the DEVICE's own
               inverse names:  |out - m| <= 2^-24 |m| + n 2^-52 max_j |x_j|  -- one rounding to float32, plus twice the
               worst case of a float64 sum of n float32 terms in any order with the float64 division.  The largest excess
               over the first term alone is printed (on an MI355X it is never positive on any scene: the float64 sums are
               far inside the second term).
    fill       rows at or past V hold exactly the fill values; the guard bands around every buffer are untouched
    paths      every output is byte-equal between POINTOPS_DEBUG=voxel_long=0, =1 and the default, and between two calls

Every native call goes through the guarded, poisoned buffers of tests/buffers.py (fill 0xFF, short and null workspaces
tried first).  The checker's result of a scene is computed once."""
import numpy as np
import pytest
import torch

import buffers
import voxel_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
MODES = {"default": None, "lane": "voxel_long=0", "wave": "voxel_long=1"}
KEYS = ("num_voxels", "status", "inverse", "counts", "first_index", "coords", "centroids", "pooled")
INTS = KEYS[:6]
ENTRY = "pointops_voxel_downsample"


def _feats(seed, N, P, C):
    return None if C is None else np.random.default_rng(seed).normal(size=(N, P, C)).astype(np.float32)


def _ragged(P, seed, C):
    """N = 3 clouds of P rows with lengths (0, 1, P)."""
    return np.stack([ref.blobs(seed + n, P) for n in range(3)]), np.array([0, 1, P], np.int64), _feats(seed, 3, P, C)


def _s(points, lengths, v, features=None, origin=None):
    return np.ascontiguousarray(points, np.float32), lengths, v, features, origin


def _frame(shift, scale):
    p = ref.blobs(50, 1000).astype(np.float64)
    return (p * scale + np.asarray(shift, np.float64)).astype(np.float32)[None]


def _faces():
    k = np.random.default_rng(5).integers(-8, 9, (2, 500, 3))
    return (k * 0.25).astype(np.float32)  # exact multiples of v = 0.25


def _nonfinite():
    p = np.stack([ref.blobs(80 + n, 300) for n in range(3)])
    p[1, 5, 0], p[1, 17, 2], p[2, 9, 1], p[2, 299] = np.nan, np.inf, np.inf, np.nan
    p[0, :, :] = np.nan  # a cloud without a live row
    return p


def _refusal():
    p = np.stack([ref.blobs(90 + n, 200) for n in range(3)])
    p[1, 77, 1] = 1e30
    return p


# name -> () -> (points (N, P, 3) float32, lengths or None, v, features or None, origin or None)
SCENES = {}
for _i, _P in enumerate((1, 63, 64, 65, 1000)):
    _C = (None, 1, 3, 33, 0)[_i]
    SCENES[f"ragged-{_P}"] = lambda P=_P, C=_C: _s(*_ragged(P, 10, C)[:2], 0.1, _ragged(P, 10, C)[2])
    SCENES[f"full-{_P}"] = lambda P=_P, C=_C: _s(_ragged(P, 20, C)[0], None, 0.1, _ragged(P, 20, C)[2])
SCENES.update({
    "channels-33": lambda: _s(*_ragged(1000, 30, 33)[:2], 0.15, _ragged(1000, 30, 33)[2]),
    "one-voxel-4096": lambda: _s(ref.blobs(40, 4096)[None], None, 100.0, _feats(41, 1, 4096, 3)),
    "one-voxel-ragged": lambda: _s(np.stack([ref.blobs(42 + n, 1100) for n in range(2)]), np.array([1025, 17], np.int64),
                                   50.0, _feats(43, 2, 1100, 1)),
    "tiny-voxels": lambda: _s(*_ragged(1000, 10, None)[:2], 1e-6, _feats(44, 3, 1000, 3)),
    "faces": lambda: _s(_faces(), None, 0.25, None, np.zeros(3, np.float32)),
    "origin-per-cloud": lambda: _s(np.stack([ref.blobs(45, 500)] * 2), None, 0.1, _feats(46, 2, 500, 1),
                                   np.array([[0.0, 0.0, 0.0], [0.05, -0.33, 7.0]], np.float32)),
    "translated": lambda: _s(_frame((1000.0, -1000.0, 500.0), 1.0), None, 0.1, _feats(47, 1, 1000, 3)),
    "scaled": lambda: _s(_frame((0.0, 0.0, 0.0), 1e-3), None, 1e-4),
    "identical": lambda: _s(np.full((1, 700, 3), 0.375, np.float32), None, 0.05, _feats(48, 1, 700, 3)),
    "nonfinite": lambda: _s(_nonfinite(), None, 0.1, _feats(49, 3, 300, 3)),
    "refusal": lambda: _s(_refusal(), None, 1e-3, _feats(51, 3, 200, 3)),
    "mid": lambda: _s(np.stack([ref.blobs(60 + n, 8192, k=12, sigma=0.05) for n in range(2)]), None, 0.04,
                      _feats(52, 2, 8192, 3)),
})
_BUILT, _WANT = {}, {}


def _scene(name):
    if name not in _BUILT:
        _BUILT[name] = SCENES[name]()
    return _BUILT[name]


def _want(name):
    if name not in _WANT:
        _WANT[name] = ref.downsample(*_scene(name))
    return _WANT[name]


def _set_mode(monkeypatch, mode):
    if MODES[mode] is None:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    else:
        monkeypatch.setenv("POINTOPS_DEBUG", MODES[mode])


def _t(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _native(dev, monkeypatch, scene, fill="ones", sibling_points=None):
    """The boundary call under the buffer contract -> ({key: numpy or None}, the contract)."""
    from pytorch3d_pointops_amd import _C_voxel

    pts, lengths, v, feats, origin = scene
    P, Lt, F, O = _t(dev, pts), _t(dev, lengths), _t(dev, feats), _t(dev, origin)
    with buffers.contract(monkeypatch, fill, short_workspace="short" if fill == "ones" else False,
                          prototypes=PROTOS) as c:
        if sibling_points is not None:
            S = _t(dev, sibling_points)
            full = torch.full((len(pts),), pts.shape[1], dtype=torch.int64, device=dev)
            c.sibling(lambda: _C_voxel.voxel_downsample(S, full, v, F, O))
        c.watch(points=P, lengths=Lt, features=F, origin=O)
        out = _C_voxel.voxel_downsample(P, Lt, v, F, O)
    c.assert_all_clear()
    num, status, inverse, counts, first, coords, centroids, pooled = out
    assert num.dtype == torch.int64 and status.dtype == torch.int32 and centroids.dtype == torch.float32
    assert all(t.dtype == torch.int64 for t in (inverse, counts, first, coords))
    assert (pooled is None) == (feats is None)
    return dict(zip(KEYS, (None if t is None else t.cpu().numpy() for t in out))), c


def _check_stages(got, scene, want, what):
    pts, lengths, v, feats, origin = scene
    N, P = pts.shape[:2]
    for k in INTS:  # stage 1: the integers, exactly
        bad = np.argwhere(got[k] != want[k])
        assert got[k].shape == want[k].shape and not len(bad), (
            f"{what}: {k} differs at {len(bad)} places, first {bad[0].tolist()}: got {got[k][tuple(bad[0])]}, "
            f"want {want[k][tuple(bad[0])]}")
    worst = float("-inf")  # (negative: every mean is closer to m than one float32 rounding allows)
    for k, values in (("centroids", pts), ("pooled", feats)):  # stage 2: the means, from the device's own assignment
        if values is None:
            continue
        assert got[k].shape == values.shape and got[k].dtype == np.float32
        m = ref.exact_means(values, got["inverse"], got["num_voxels"])
        bound = ref.mean_bound(values, got["inverse"], got["counts"], m)
        err = np.abs(got[k].astype(np.float64) - m)
        rounding = 2.0 ** -24 * np.abs(m)
        worst = max(worst, float((err - rounding).max()) if err.size else worst)
        assert (err <= bound).all(), (f"{what}: {k} off by {float((err - bound).max()):.3e} beyond the bound at "
                                      f"{np.argwhere(err > bound)[0].tolist()}")
        # stage 3: the fill of the rows at or past V, bit for bit (+0.0)
        pad = np.arange(P)[None, :] >= got["num_voxels"][:, None]
        assert not got[k].view(np.int32)[pad].any(), f"{what}: {k} padding rows"
    print(f"{what}: largest excess of |out - m| over 2^-24 |m|: {worst:.3e}")


def _assert_bit_equal(a, b, what):
    for k in KEYS:
        if a[k] is None:
            assert b[k] is None
        else:
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} is not bit-equal"


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_on_every_path_equals_the_checker_stage_by_stage(dev, monkeypatch, name):
    scene = _scene(name)
    first = None
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        got, c = _native(dev, monkeypatch, scene)
        assert {(n, how) for n, _, how in c.rejections} == {(ENTRY, "short"), (ENTRY, "null")}
        assert [b.kind for b in c.buffers] == ["out"] * (7 + (scene[3] is not None)) + ["workspace"]
        if first is None:
            first = got
            _check_stages(got, scene, _want(name), f"{name} [{mode}]")
        else:
            _assert_bit_equal(got, first, f"{name} [{mode}] against [default]")
    again, _ = _native(dev, monkeypatch, scene)
    _assert_bit_equal(again, first, f"{name}: a second call")


def test_what_the_scenes_are_meant_to_show(dev, monkeypatch):
    """The results have the features the scene names promise (the comparison above is only as good as its scenes)."""
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    run = lambda name: _native(dev, monkeypatch, _scene(name))[0]  # noqa: E731
    got = run("ragged-1000")
    assert got["num_voxels"][:2].tolist() == [0, 1] and 50 < got["num_voxels"][2] < 1000
    assert got["counts"][2].max() > 16 and (got["counts"][2, : got["num_voxels"][2]] == 1).any()  # both reductions
    one = run("one-voxel-4096")
    assert one["num_voxels"].tolist() == [1] and one["counts"][0, 0] == 4096 and not one["inverse"].any()
    rag = run("one-voxel-ragged")
    assert rag["num_voxels"].tolist() == [1, 1] and rag["counts"][:, 0].tolist() == [1025, 17]
    tiny = run("tiny-voxels")
    assert tiny["num_voxels"].tolist() == [0, 1, 1000] and (tiny["counts"][2] == 1).all()
    faces = run("faces")
    pts = _scene("faces")[0]
    cells = np.take_along_axis(faces["coords"], faces["inverse"][..., None].repeat(3, 2), 1)
    assert np.array_equal(cells, np.rint(pts.astype(np.float64) / 0.25).astype(np.int64))  # a face: the upper cell
    per = run("origin-per-cloud")
    assert not np.array_equal(per["coords"][0], per["coords"][1]) and (per["coords"][1, :, 2] < -60).any()
    ident = run("identical")
    assert ident["num_voxels"].tolist() == [1] and ident["centroids"][0, 0].tolist() == [0.375] * 3
    nf = run("nonfinite")
    assert nf["num_voxels"][0] == 0 and (nf["inverse"][0] == -1).all() and nf["status"].tolist() == [0, 0, 0]
    for n, i in ((1, 5), (1, 17), (2, 9), (2, 299)):
        assert nf["inverse"][n, i] == -1
    assert (nf["inverse"][1] >= 0).sum() == 298 and (nf["inverse"][2] >= 0).sum() == 298
    # the frames: the same cloud shrunk keeps its voxel structure (the voxel size scales with the frame) up to the
    # points that rounding moves across a face
    base = ref.downsample(ref.blobs(50, 1000)[None], None, 0.1)
    assert abs(int(run("scaled")["num_voxels"][0]) - int(base["num_voxels"][0])) <= 0.02 * base["num_voxels"][0]
    assert abs(int(run("translated")["num_voxels"][0]) - int(base["num_voxels"][0])) <= 0.1 * base["num_voxels"][0]


def test_a_refused_cloud_leaves_its_neighbours_alone(dev, monkeypatch):
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts, lengths, v, feats, origin = _scene("refusal")
    got, _ = _native(dev, monkeypatch, _scene("refusal"))
    assert got["status"].tolist() == [0, 1, 0] and got["num_voxels"][1] == 0 and (got["inverse"][1] == -1).all()
    assert not got["counts"][1].any() and (got["first_index"][1] == -1).all() and not got["centroids"][1].any()
    for n in (0, 2):
        alone, _ = _native(dev, monkeypatch, (pts[n:n + 1], None, v, feats[n:n + 1], None))
        for k in KEYS:
            assert got[k][n].tobytes() == alone[k][0].tobytes(), (n, k)


def test_many_clouds_cross_the_slice_boundary(dev, monkeypatch):
    """65 600 clouds of 4 points go to the entry in two slices.  Every output of EVERY cloud equals the definition
    written out for four points; the first, last and boundary clouds also go through the checker."""
    N, P, v = 65600, 4, 0.25
    pts = np.random.default_rng(77).uniform(0, 1, (N, P, 3)).astype(np.float32)
    lengths = np.random.default_rng(78).integers(0, P + 1, N).astype(np.int64)
    lengths[[0, 65534, 65535, 65536, N - 1]] = P
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    got, c = _native(dev, monkeypatch, (pts, lengths, v, None, None))
    assert len(c.rejections) == 4  # two native calls
    pick = [0, 1, 2, 65533, 65534, 65535, 65536, 65537, N - 2, N - 1]
    sub = (pts[pick], lengths[pick], v, None, None)
    _check_stages({k: None if a is None else a[pick] for k, a in got.items()}, sub, ref.downsample(*sub), "picked clouds")
    live = np.arange(P)[None, :] < lengths[:, None]
    x = pts.astype(np.float64)
    mn = np.where(live[..., None], pts, np.float32(np.inf)).min(1)  # float32
    o = mn.astype(np.float64) - 0.5 * np.float64(np.float32(v))
    with np.errstate(invalid="ignore"):
        cell = np.floor((x - o[:, None, :]) / np.float64(np.float32(v)))
    cell = np.where(live[..., None], cell, 0).astype(np.int64)
    code = (cell[..., 2] * 1000 + cell[..., 1]) * 1000 + cell[..., 0]  # (z, y, x) order; cells are in [0, 5)
    same = (code[:, :, None] == code[:, None, :]) & live[:, :, None] & live[:, None, :]  # [n, i, j]
    earlier = np.tril(np.ones((P, P), bool), -1)[None]  # j < i
    is_first = live & ~(same & earlier).any(2)
    less = (code[:, None, :] < code[:, :, None]) & is_first[:, None, :]  # first occurrences j below i's cell
    inverse = np.where(live, less.sum(2), -1)
    assert np.array_equal(got["inverse"], inverse)
    assert np.array_equal(got["num_voxels"], is_first.sum(1)) and not got["status"].any()
    count_of_row = same.sum(2)
    sums = (same[..., None] * x[:, None, :, :]).sum(2)  # exact: four float32 terms of [0, 1) in float64
    n_idx, i_idx = np.nonzero(is_first)
    r_idx = inverse[n_idx, i_idx]
    counts = np.zeros((N, P), np.int64)
    first = np.full((N, P), -1, np.int64)
    coords = np.zeros((N, P, 3), np.int64)
    mean = np.zeros((N, P, 3), np.float64)
    counts[n_idx, r_idx] = count_of_row[n_idx, i_idx]
    first[n_idx, r_idx] = i_idx
    coords[n_idx, r_idx] = cell[n_idx, i_idx]
    mean[n_idx, r_idx] = sums[n_idx, i_idx] / count_of_row[n_idx, i_idx][:, None]
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["first_index"], first)
    assert np.array_equal(got["coords"], coords)
    biggest = np.zeros((N, P, 3), np.float64)
    biggest[n_idx, r_idx] = np.where(same[..., None], np.abs(x)[:, None, :, :], 0.0).max(2)[n_idx, i_idx]
    err = np.abs(got["centroids"].astype(np.float64) - mean)
    assert (err <= 2.0 ** -24 * np.abs(mean) + counts[..., None] * 2.0 ** -52 * biggest).all()
    assert (counts > 1).sum() > 1000 and (is_first.sum(1) > 1).sum() > 1000


def _public(dev, name, **kw):
    from pytorch3d_pointops_amd import functions as f

    pts, lengths, v, feats, origin = _scene(name)
    return f.voxel_downsample(_t(dev, pts), _t(dev, lengths), voxel_size=v, features=_t(dev, feats),
                              origin=_t(dev, origin), **kw)


def _public_dict(r):
    return dict(num_voxels=r.num_voxels, status=r.status, inverse=r.inverse, counts=r.counts,
                first_index=r.first_index, coords=r.coords, centroids=r.points, pooled=r.features)


@pytest.mark.parametrize("name", ["ragged-65", "channels-33", "origin-per-cloud"])
def test_public_call_dict_features_and_pointclouds_route(dev, monkeypatch, name):
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd.structures import Pointclouds

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts, lengths, v, feats, origin = _scene(name)
    want, _ = _native(dev, monkeypatch, _scene(name))
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=PROTOS) as c:
        r = _public(dev, name)
    c.assert_guards_intact()
    assert isinstance(r, f.VoxelDownsample)
    for k, t in _public_dict(r).items():
        assert t.cpu().numpy().tobytes() == want[k].tobytes(), k
    # a dict of features is concatenated for the one call and split again; the widths come back
    C = feats.shape[2]
    halves = {"a": _t(dev, feats[..., : C // 2]), "b": _t(dev, feats[..., C // 2:])}
    d = f.voxel_downsample(_t(dev, pts), _t(dev, lengths), voxel_size=v, features=halves, origin=_t(dev, origin))
    assert sorted(d.features) == ["a", "b"] and d.features["a"].shape[2] == C // 2
    assert torch.equal(torch.cat([d.features["a"], d.features["b"]], 2), r.features) and torch.equal(d.points, r.points)
    if origin is not None:
        return
    # the Pointclouds route: every feature pooled, lists rebuilt
    L = np.full(len(pts), pts.shape[1]) if lengths is None else lengths
    pc = Pointclouds([_t(dev, pts[n, : L[n]]) for n in range(len(pts))],
                     {"a": [halves["a"][n, : L[n]] for n in range(len(pts))],
                      "b": [halves["b"][n, : L[n]] for n in range(len(pts))]})
    small = pc.voxel_downsample(v)
    assert isinstance(small, Pointclouds) and small.num_points_per_cloud().tolist() == want["num_voxels"].tolist()
    for n, V in enumerate(want["num_voxels"]):
        assert small.points_list()[n].cpu().numpy().tobytes() == want["centroids"][n, :V].tobytes()
        got_f = torch.cat([small.features_list()["a"][n], small.features_list()["b"][n]], 1)
        assert got_f.cpu().numpy().tobytes() == want["pooled"][n, :V].tobytes()
    r2 = f.voxel_downsample(pc, voxel_size=v)
    assert torch.equal(r2.inverse, r.inverse) and sorted(r2.features) == ["a", "b"]


def test_voxels_to_padded_against_numpy_and_check_raises(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    r = _public(dev, "ragged-1000")
    p = f.voxels_to_padded(r, check=True)
    V = r.num_voxels.cpu().numpy()
    vmax = int(V.max())
    assert p.points.shape == (3, vmax, 3) and p.features.shape == (3, vmax, 0) and p.coords.shape == (3, vmax, 3)
    assert p.counts.shape == (3, vmax) and p.first_index.shape == (3, vmax) and p.inverse.shape == (3, 1000)
    for a, b in ((p.points, r.points), (p.counts, r.counts), (p.first_index, r.first_index), (p.coords, r.coords)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()[:, :vmax])
    assert torch.equal(p.num_voxels, r.num_voxels) and torch.equal(p.inverse, r.inverse)
    bad = _public(dev, "refusal")
    assert f.voxels_to_padded(bad).status.tolist() == [0, 1, 0]
    with pytest.raises(RuntimeError, match="refused"):
        f.voxels_to_padded(bad, check=True)
    from pytorch3d_pointops_amd.structures import Pointclouds
    with pytest.raises(RuntimeError, match="refused"):
        Pointclouds(_t(dev, _scene("refusal")[0])).voxel_downsample(1e-3, check=True)
    with pytest.raises(ValueError):
        f.voxels_to_padded(r.points)


def test_empty_batch_and_empty_clouds(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    for shape in ((0, 5, 3), (0, 0, 3), (4, 0, 3)):
        r = f.voxel_downsample(torch.zeros(shape, device=dev), voxel_size=0.1)
        assert r.points.shape == shape and r.inverse.shape == shape[:2] and r.coords.shape == shape
        assert r.num_voxels.tolist() == [0] * shape[0] and r.status.tolist() == [0] * shape[0] and r.features is None
        assert f.voxels_to_padded(r).points.shape == (shape[0], 0, 3)


def test_a_side_stream_gives_the_same_bytes(dev, monkeypatch):
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    scene = _scene("mid")
    first, _ = _native(dev, monkeypatch, scene)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other, _ = _native(dev, monkeypatch, scene)
    side.synchronize()
    _assert_bit_equal(other, first, "side stream")


@pytest.mark.parametrize("name", ["mid", "ragged-65"])
def test_graph_capture_replays_the_eager_result(dev, monkeypatch, name):
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd import graphs

    pts, lengths, v, feats, origin = _scene(name)
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    Lt, F = _t(dev, lengths), _t(dev, feats)

    def call(a):
        r = f.voxel_downsample(a, Lt, voxel_size=v, features=F)
        return r.points, r.features, r.num_voxels, r.inverse, r.counts, r.first_index, r.coords, r.status

    P = _t(dev, pts)
    want = call(P)
    step = graphs.capture(call, (P.clone(),))
    assert all(torch.equal(a, b) for a, b in zip(step(), want))
    P2 = _t(dev, pts[::-1, ::-1])  # a second scene through the static input
    want2 = call(P2)
    assert not torch.equal(want2[3], want[3])
    assert all(torch.equal(a, b) for a, b in zip(step(P2), want2))
    if name != "mid":  # (the checker's pass over 2 x 8192 points is paid once, by the scene test)
        scene2 = (np.ascontiguousarray(pts[::-1, ::-1]), lengths, v, feats, origin)
        got2 = dict(zip(("centroids", "pooled", "num_voxels", "inverse", "counts", "first_index", "coords", "status"),
                        (t.cpu().numpy() for t in want2)))
        _check_stages(got2, scene2, ref.downsample(*scene2), "second scene")


_BASELINE = {}


@pytest.mark.parametrize("fill", buffers.FILLS)
@pytest.mark.parametrize("name", ["ragged-1000", "ragged-65"])
def test_buffer_contract_under_every_fill(dev, monkeypatch, name, fill):
    """zero / ones / stale (what a sibling call on other points with full lengths left behind): the outputs are the
    same bytes, padding rows included."""
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    scene = _scene(name)
    got, c = _native(dev, monkeypatch, scene, fill=fill, sibling_points=np.ascontiguousarray(scene[0][::-1]))
    assert c.inputs_checked >= 2
    _check_stages(got, scene, _want(name), f"{name} [{fill}]")
    key = _BASELINE.setdefault(name, c.output_bytes())
    for (n1, a), (_, b) in zip(c.output_bytes(), key):
        assert np.array_equal(a, b), (fill, n1)


def test_bad_arguments_are_rejected_with_nothing_written(dev):
    from pytorch3d_pointops_amd import _C
    from pytorch3d_pointops_amd import functions as f

    X = torch.rand(1, 8, 3, device=dev)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39, "x"):
        with pytest.raises(ValueError):
            f.voxel_downsample(X, voxel_size=bad)
    for kw in (dict(points=torch.rand(1, 8, 2, device=dev)), dict(points=X.double()), dict(points=X[0]),
               dict(lengths=torch.tensor([8, 8], device=dev)), dict(lengths=torch.tensor([8], dtype=torch.int32, device=dev)),
               dict(lengths=[8]), dict(features=torch.rand(1, 7, 3, device=dev)), dict(features=X.double()),
               dict(features={"a": X[0]}), dict(features=torch.rand(1, 8, 1025, device=dev)),
               dict(origin=torch.zeros(2, 3, device=dev)), dict(origin=torch.zeros(3, dtype=torch.float64, device=dev)),
               dict(origin=[0.0, 0.0, 0.0])):
        with pytest.raises(ValueError):
            f.voxel_downsample(**{**dict(points=X, voxel_size=0.1), **kw})
    sizer = _C._lib.pointops_voxel_workspace_bytes
    assert sizer(1, 2 ** 24 + 1, 0) == 0 and sizer(65536, 8, 0) == 0 and sizer(1, 8, 1025) == 0 and sizer(1, 8, 3) > 0
    outs = [torch.full((1024,), 7, dtype=torch.uint8, device=dev) for _ in range(8)]
    feats = torch.rand(1, 8, 3, device=dev)
    ws = torch.zeros(sizer(1, 8, 3), dtype=torch.uint8, device=dev)
    for bad in (dict(v=0.0), dict(v=-1.0), dict(v=float("nan")), dict(v=float("inf")), dict(P=2 ** 24 + 1),
                dict(N=65536), dict(N=-1), dict(C=1025), dict(C=-1), dict(feats=None)):
        a = dict(v=0.1, N=1, P=8, C=3, feats=feats)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.voxel_downsample("voxel_downsample", dev, X, None, a["feats"], None, 0, a["N"], a["P"], a["C"],
                                      a["v"], *outs, ws, ws.numel())
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)


def test_gradients_equal_the_float64_composition(dev, monkeypatch):
    """(points w1).sum() + (features w2).sum() at 2 x 65 points, C = 3: the gradients equal those of the float64 torch
    composition (index_add over the device's inverse, then a divide) within 2^-23 relative -- the one float32 division
    of the backward is 2^-24 -- and are exactly 0 on the rows of no voxel; two backward calls are byte-equal."""
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    N, P, C, v = 2, 65, 3, 0.15
    pts = np.stack([ref.blobs(70 + n, P) for n in range(N)])
    pts[1, 7, 0], pts[1, 30] = np.nan, np.inf
    lengths = torch.tensor([P, 50], device=dev)
    feats = _feats(71, N, P, C)
    rng = np.random.default_rng(72)
    w1, w2 = (torch.from_numpy(rng.normal(size=(N, P, k)).astype(np.float32)).to(dev) for k in (3, C))

    def grads():
        X, F = _t(dev, pts).requires_grad_(True), _t(dev, feats).requires_grad_(True)
        r = f.voxel_downsample(X, lengths, voxel_size=v, features=F)
        assert r.points.requires_grad and r.features.requires_grad and not r.inverse.requires_grad
        ((r.points * w1).sum() + (r.features * w2).sum()).backward()
        return X.grad, F.grad, r

    gx, gf, r = grads()
    gx2, gf2, _ = grads()
    assert gx.cpu().numpy().tobytes() == gx2.cpu().numpy().tobytes() and gf.cpu().numpy().tobytes() == gf2.cpu().numpy().tobytes()
    member = r.inverse >= 0
    assert int(member.sum()) == P + 50 - 2 and int(r.num_voxels.min()) > 3 and int(r.counts.max()) > 1
    assert not gx[~member].any() and not gf[~member].any()  # exactly 0, NaN and inf rows included
    idx = r.inverse.clamp(min=0)
    for g, vals, w in ((gx, pts, w1), (gf, feats, w2)):
        x64 = torch.nan_to_num(_t(dev, vals).double(), nan=0.0, posinf=0.0, neginf=0.0).requires_grad_(True)
        K = x64.shape[2]
        sums = torch.zeros(N, P, K, dtype=torch.float64, device=dev)
        cnt = torch.zeros(N, P, dtype=torch.float64, device=dev)
        for n in range(N):
            sums[n] = sums[n].index_add(0, idx[n][member[n]], x64[n][member[n]])
            cnt[n] = cnt[n].index_add(0, idx[n][member[n]], torch.ones(int(member[n].sum()), dtype=torch.float64, device=dev))
        mean = sums / cnt.clamp(min=1)[..., None]
        (mean * w.double()).sum().backward()
        want = x64.grad
        err = (g.double() - want).abs()
        assert bool((err <= 2.0 ** -23 * want.abs()).all()), float((err / want.abs().clamp(min=1e-300)).max())
        assert bool((want[member] != 0).all())
