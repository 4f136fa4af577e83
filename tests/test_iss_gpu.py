"""iss_keypoints on the GPU against the numpy checker of tests/iss_ref.py, stage by stage, so that no stage's rounding
hides another's error:

    moments       equal to iss_ref.moments                                  (integers: no tolerance)
    eigenvalues   within 2^-23 |l_ref| + 2^-40 l2_ref of numpy's eigvalsh of the checker's C: the rounding to float32 is
                  2^-24 relative, the rest is the backward error of two float64 solvers (a few 2^-53 l2 each) with room
    saliency      equal to iss_ref.decide(the DEVICE's eigenvalues)         (float32 comparisons: no tolerance)
    mask          equal to iss_ref.nms(the DEVICE's saliency)
    num_keypoints equal to the mask's row sums

Every call goes through the guarded, poisoned buffers of tests/buffers.py (fill 0xFF, short and null workspaces tried
first).  Each scene runs three ways -- as the library chooses (grids from 512 points per cloud on), with
POINTOPS_DEBUG=iss_grid=0 (all pairs) and iss_grid=1 (a grid whatever the size) -- and the three are bit-equal in every
output, moments included.  The checker's result of a scene is computed once."""
import numpy as np
import pytest
import torch

import buffers
import iss_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
MODES = {"default": None, "allpairs": "iss_grid=0", "grid": "iss_grid=1"}
KEYS = ("mask", "saliency", "eigenvalues", "moments")
ENTRY = "pointops_iss_keypoints"


def _ragged(P, seed):
    """N = 3 clouds of P rows with lengths (0, 1, P)."""
    return np.stack([ref.blobs_scene(seed + n, P) for n in range(3)]), np.array([0, 1, P], np.int64)


def _radii(P):
    return (0.08, 0.05, 5) if P >= 1000 else (0.25, 0.15, 3)


def _nonfinite():
    import test_cluster_gpu

    return test_cluster_gpu._nonfinite()


def _frame(shift, scale):
    p = ref.blobs_scene(50, 1000).astype(np.float64)
    return (p * scale + np.asarray(shift, np.float64)).astype(np.float32)[None]


def _s(points, lengths, rs, rn, mn=5, g21=0.975, g32=0.975):
    return points, lengths, rs, rn, g21, g32, mn


# name -> () -> (points (N, P, 3) float32, lengths or None, rs, rn, gamma_21, gamma_32, min_neighbors)
SCENES = {}
for _P in (1, 63, 64, 65, 1000):
    SCENES[f"ragged-{_P}"] = lambda P=_P: _s(*_ragged(P, 10), *_radii(P))
    SCENES[f"full-{_P}"] = lambda P=_P: _s(_ragged(P, 20)[0], None, *_radii(P))
SCENES.update({
    "rn-above-rs": lambda: _s(*_ragged(1000, 10), 0.05, 0.08),
    "one-cell": lambda: _s(*_ragged(1000, 10), 10.0, 10.0),
    "tiny-radii": lambda: _s(*_ragged(1000, 10), 1e-6, 1e-6, 0),
    "min-neighbors-0": lambda: _s(*_ragged(1000, 10), 0.08, 0.05, 0),
    "min-neighbors-high": lambda: _s(*_ragged(1000, 10), 0.08, 0.05, 5000),
    "gamma-1": lambda: _s(*_ragged(1000, 10), 0.08, 0.05, 5, 1.0, 1.0),
    "gamma-1e-3": lambda: _s(*_ragged(1000, 10), 0.08, 0.05, 5, 1e-3, 1e-3),
    "identical": lambda: _s(np.full((1, 700, 3), 0.375, np.float32), None, 0.05, 0.05),
    "doubled": lambda: _s(ref.doubled(ref.blobs_scene(71, 500))[None], None, 0.08, 0.05, 2),
    "tilted-plane": lambda: _s(ref.tilted_plane()[None], None, 0.08, 0.05, 0),
    "cube-corner": lambda: _s(ref.cube_corner()[None], None, 0.13, 0.11, 4),
    "translated": lambda: _s(_frame((1000.0, -1000.0, 500.0), 1.0), None, 0.08, 0.05),
    "scaled": lambda: _s(_frame((0.0, 0.0, 0.0), 1e-3), None, 0.08e-3, 0.05e-3),
    "nonfinite": lambda: _s(_nonfinite(), None, 0.08, 0.05),
    "mid": lambda: _s(np.stack([ref.blobs_scene(60 + n, 8192, k=12, sigma=0.05) for n in range(2)]), None, 0.06, 0.04),
})
_BUILT, _WANT = {}, {}


def _scene(name):
    if name not in _BUILT:
        pts, lengths, *rest = SCENES[name]()
        _BUILT[name] = (np.ascontiguousarray(pts, np.float32), lengths, *rest)
    return _BUILT[name]


def _want(name):
    """The checker's moments, C and float64 eigenvalues of a scene (the later stages are checked from the device's own
    values)."""
    if name not in _WANT:
        pts, lengths, rs = _scene(name)[:3]
        mom = ref.moments(pts, lengths, rs)
        C = ref.covariance(mom, rs)
        _WANT[name] = dict(moments=mom, C=C, eig64=ref.eigenvalues64(C))
    return _WANT[name]


def _set_mode(monkeypatch, mode):
    if MODES[mode] is None:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    else:
        monkeypatch.setenv("POINTOPS_DEBUG", MODES[mode])


def _guarded(monkeypatch, call, fill="ones", sibling=None, **watched):
    """`call()` under the buffer contract; -> (the tuple it returns, the contract)."""
    with buffers.contract(monkeypatch, fill, short_workspace="short" if fill == "ones" else False,
                          prototypes=PROTOS) as c:
        if sibling is not None:
            c.sibling(sibling)
        c.watch(**watched)
        out = call()
    c.assert_all_clear()
    return out, c


def _native(dev, monkeypatch, scene, fill="ones", sibling_points=None):
    """The boundary call with the diagnostic moments -> ({key: numpy}, the contract)."""
    from pytorch3d_pointops_amd import _C_iss

    pts, lengths, rs, rn, g21, g32, mn = scene
    P = torch.from_numpy(pts).to(dev)
    Lt = None if lengths is None else torch.from_numpy(lengths).to(dev)
    sibling = None
    if sibling_points is not None:
        S = torch.from_numpy(sibling_points).to(dev)
        full = torch.full((len(pts),), pts.shape[1], dtype=torch.int64, device=dev)
        sibling = lambda: _C_iss.iss_keypoints(S, full, rs, rn, g21, g32, mn, want_moments=True)  # noqa: E731
    out, c = _guarded(monkeypatch, lambda: _C_iss.iss_keypoints(P, Lt, rs, rn, g21, g32, mn, want_moments=True),
                      fill=fill, sibling=sibling, points=P, lengths=Lt)
    mask, sal, eig, mom = out
    assert mask.dtype == torch.bool and sal.dtype == torch.float32 and eig.dtype == torch.float32
    assert mom.dtype == torch.int64 and mom.shape == pts.shape[:2] + (10,)
    return dict(zip(KEYS, (t.cpu().numpy() for t in out))), c


def _check_stages(got, name, scene, what):
    pts, lengths, rs, rn, g21, g32, mn = scene
    want = _want(name) if name is not None else None
    if want is None:
        mom = ref.moments(pts, lengths, rs)
        C = ref.covariance(mom, rs)
        want = dict(moments=mom, C=C, eig64=ref.eigenvalues64(C))
    N, P = pts.shape[:2]
    L = np.full(N, P) if lengths is None else np.clip(lengths, 0, P)
    live = np.arange(P)[None, :] < L[:, None]
    bad = np.argwhere(got["moments"] != want["moments"])
    assert not len(bad), (f"{what}: moments differ at {len(bad)} places, first {bad[0].tolist()}: got "
                          f"{got['moments'][tuple(bad[0])]}, want {want['moments'][tuple(bad[0])]}")
    e64 = np.where(live[..., None], want["eig64"], 0.0)
    tol = 2.0 ** -23 * np.abs(e64) + 2.0 ** -40 * e64[..., 2:3]
    err = np.abs(got["eigenvalues"].astype(np.float64) - e64)
    worst = float((err - tol).max()) if err.size else 0.0
    print(f"{what}: eigenvalues: max |got - ref| = {float(err.max()) if err.size else 0.0:.3e}, "
          f"max excess over the bound = {worst:.3e}")
    assert (err <= tol).all(), f"{what}: eigenvalues off by {worst:.3e} beyond the bound at {np.argwhere(err > tol)[0]}"
    assert not got["eigenvalues"][~live].any() and not got["saliency"][~live].any() and not got["mask"][~live].any()
    sal = np.where(live, ref.decide(got["eigenvalues"], g21, g32), np.float32(0))
    assert np.array_equal(got["saliency"].view(np.int32), sal.view(np.int32)), f"{what}: saliency"
    mask = ref.nms(got["saliency"], pts, lengths, rn, mn)
    bad = np.argwhere(got["mask"] != mask)
    assert not len(bad), f"{what}: mask differs at {len(bad)} places, first {bad[0].tolist()}"


def _assert_bit_equal(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} is not bit-equal"


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_in_three_modes_equals_the_checker_stage_by_stage(dev, monkeypatch, name):
    scene = _scene(name)
    first = None
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        got, c = _native(dev, monkeypatch, scene)
        assert {(n, how) for n, _, how in c.rejections} == {(ENTRY, "short"), (ENTRY, "null")}
        assert [b.kind for b in c.buffers] == ["out"] * 4 + ["workspace"]
        if first is None:
            first = got
            _check_stages(got, name, scene, f"{name} [{mode}]")
        else:
            _assert_bit_equal(got, first, f"{name} [{mode}] against [default]")


def test_what_the_scenes_are_meant_to_show(dev, monkeypatch):
    """The results have the features the scene names promise (the comparison above is only as good as its scenes)."""
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    run = lambda name: _native(dev, monkeypatch, _scene(name))[0]  # noqa: E731
    got = run("ragged-1000")
    assert got["mask"][2].sum() >= 3 and (got["saliency"][2] > 0).sum() > got["mask"][2].sum()
    assert got["moments"][1, 0].tolist() == [1] + [0] * 9 and not got["mask"][:2].any()
    one = run("one-cell")
    assert (one["moments"][2, :, 0] == 1000).all() and one["mask"].sum(1).tolist() == [0, 0, 1]
    tiny = run("tiny-radii")
    assert (tiny["moments"][2, :, 0] == 1).all() and not tiny["saliency"].any() and not tiny["mask"].any()
    assert run("min-neighbors-0")["mask"].sum() >= got["mask"].sum() and not run("min-neighbors-high")["mask"].any()
    assert not run("gamma-1e-3")["saliency"].any()
    assert (run("gamma-1")["saliency"] > 0).sum() > (got["saliency"] > 0).sum()
    ident = run("identical")
    assert (ident["moments"][0, :, 0] == 700).all() and not ident["moments"][0, :, 1:].any() and not ident["mask"].any()
    dbl = run("doubled")
    assert dbl["mask"][0, :500].sum() > 0 and not dbl["mask"][0, 500:].any()
    assert np.array_equal(dbl["saliency"][0, :500], dbl["saliency"][0, 500:])
    assert not run("tilted-plane")["saliency"].any()
    assert np.flatnonzero(run("cube-corner")["mask"][0]).tolist() == [0]
    nf = run("nonfinite")
    for n, i in ((1, 5), (1, 17), (2, 9)):
        assert nf["moments"][n, i, 0] == 0 and not nf["eigenvalues"][n, i].any() and not nf["mask"][n, i]
    assert nf["mask"].sum(1).min() >= 1
    # the frames: the same cloud moved / shrunk keeps its support counts (the radius scales with the frame)
    base = ref.moments(ref.blobs_scene(50, 1000)[None], None, 0.08)[0, :, 0]
    assert (run("scaled")["moments"][0, :, 0] == base).mean() > 0.99
    assert (run("translated")["moments"][0, :, 0] == base).mean() > 0.95  # (coordinates rounded to 2^-14)


@pytest.mark.parametrize("mode", ["default", "grid"])
def test_many_clouds_cross_the_slice_boundary(dev, monkeypatch, mode):
    """65 600 clouds of 4 points go to the entry in two slices.  Moments, saliency and mask of EVERY cloud equal the
    definition written out for four points; the first, last and boundary clouds also go through the checker."""
    N, P = 65600, 4
    rs, rn, g21, g32, mn = 0.7, 0.5, 0.975, 0.975, 2
    pts = np.random.default_rng(77).uniform(0, 1, (N, P, 3)).astype(np.float32)
    lengths = np.random.default_rng(78).integers(0, P + 1, N).astype(np.int64)
    lengths[[0, 65534, 65535, 65536, N - 1]] = P
    _set_mode(monkeypatch, mode)
    got, c = _native(dev, monkeypatch, (pts, lengths, rs, rn, g21, g32, mn))
    assert len(c.rejections) == 4  # two native calls
    pick = [0, 1, 2, 65533, 65534, 65535, 65536, 65537, N - 2, N - 1]
    _check_stages({k: v[pick] for k, v in got.items()}, None, (pts[pick], lengths[pick], rs, rn, g21, g32, mn),
                  f"picked clouds [{mode}]")
    valid = np.arange(P)[None, :] < lengths[:, None]
    pair = valid[:, :, None] & valid[:, None, :]
    d = pts[:, :, None, :] - pts[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    hit = (d2 < np.float32(rs) * np.float32(rs)) & pair
    q = np.rint((pts[:, None, :, :].astype(np.float64) - pts[:, :, None, :].astype(np.float64)) * ref.scale(rs))
    q = np.where(hit[..., None], q, 0.0).astype(np.int64)
    mom = np.concatenate([hit.sum(2)[..., None], q.sum(2)] +
                         [(q[..., u] * q[..., v]).sum(2)[..., None] for u, v in ref.PAIRS], axis=2)
    assert np.array_equal(got["moments"], mom)
    sal = np.where(valid, ref.decide(got["eigenvalues"], g21, g32), np.float32(0))
    assert np.array_equal(got["saliency"], sal) and (sal > 0).sum() > 1000
    near = (d2 < np.float32(rn) * np.float32(rn)) & pair
    idx = np.arange(P)
    beats = (sal[:, None, :] > sal[:, :, None]) | ((sal[:, None, :] == sal[:, :, None]) & (idx[None, None, :] < idx[None, :, None]))
    mask = (sal > 0) & (near.sum(2) >= mn) & ~(near & beats).any(2)
    assert np.array_equal(got["mask"], mask) and mask.sum() > 1000


def _public(dev, name, via="tensor"):
    from pytorch3d_pointops_amd import functions as f

    pts, lengths, rs, rn, g21, g32, mn = _scene(name)
    kw = dict(salient_radius=rs, non_max_radius=rn, gamma_21=g21, gamma_32=g32, min_neighbors=mn)
    P = torch.from_numpy(pts).to(dev)
    if via == "pointclouds":
        from pytorch3d_pointops_amd.structures import Pointclouds

        L = np.full(len(pts), pts.shape[1]) if lengths is None else lengths
        return Pointclouds([P[n, :int(L[n])] for n in range(len(pts))]).iss_keypoints(**kw)
    return f.iss_keypoints(P, None if lengths is None else torch.from_numpy(lengths).to(dev), **kw)


@pytest.mark.parametrize("name", ["ragged-65", "ragged-1000"])
def test_public_call_and_pointclouds_route(dev, monkeypatch, name):
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    want, _ = _native(dev, monkeypatch, _scene(name))
    for via in ("tensor", "pointclouds"):
        with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=PROTOS) as c:
            r = _public(dev, name, via)
        c.assert_guards_intact()
        kinds = [b.kind for b in c.buffers]  # (no moments unless asked for; a Pointclouds pads through the seam too)
        assert kinds.count("workspace") == 1 and kinds.count("out") == 3 + (via == "pointclouds"), kinds
        assert r.mask.dtype == torch.bool and r.num_keypoints.dtype == torch.int64
        for k in KEYS[:3]:
            assert getattr(r, k).cpu().numpy().tobytes() == want[k].tobytes(), (via, k)
        assert np.array_equal(r.num_keypoints.cpu().numpy(), want["mask"].sum(1))


def test_two_runs_and_a_side_stream_are_bit_equal(dev, monkeypatch):
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    scene = _scene("mid")
    first, _ = _native(dev, monkeypatch, scene)
    again, _ = _native(dev, monkeypatch, scene)
    _assert_bit_equal(again, first, "second run")
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

    pts, lengths, rs, rn, g21, g32, mn = _scene(name)
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    Lt = None if lengths is None else torch.from_numpy(lengths).to(dev)
    call = lambda a: tuple(f.iss_keypoints(a, Lt, salient_radius=rs, non_max_radius=rn, min_neighbors=mn))  # noqa: E731
    P = torch.from_numpy(pts).to(dev)
    want = call(P)
    step = graphs.capture(call, (P.clone(),))
    assert all(torch.equal(a, b) for a, b in zip(step(), want))
    P2 = torch.from_numpy(np.ascontiguousarray(pts[::-1, ::-1])).to(dev)  # a second scene through the static input
    want2 = call(P2)
    assert not torch.equal(want2[1], want[1])
    assert all(torch.equal(a, b) for a, b in zip(step(P2), want2))
    if name != "mid":  # (the checker's pass over 2 x 8192 points is paid once, by the scene test)
        got2 = dict(zip(KEYS[:3], (t.cpu().numpy() for t in want2)))
        got2["moments"] = ref.moments(pts[::-1, ::-1], lengths, rs)  # (the public call has none: the stage is vacuous)
        _check_stages(got2, None, (np.ascontiguousarray(pts[::-1, ::-1]), lengths, rs, rn, g21, g32, mn), "second scene")


_BASELINE = {}


@pytest.mark.parametrize("fill", buffers.FILLS)
@pytest.mark.parametrize("name", ["ragged-1000", "ragged-65"])
def test_buffer_contract_under_every_fill(dev, monkeypatch, name, fill):
    """zero / ones / stale (what a sibling call on other points with full lengths left behind): the outputs are the
    same bytes, padding rows included."""
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    scene = _scene(name)
    got, c = _native(dev, monkeypatch, scene, fill=fill, sibling_points=np.ascontiguousarray(scene[0][::-1]))
    assert [b.kind for b in c.buffers] == ["out"] * 4 + ["workspace"] and c.inputs_checked >= 2
    _check_stages(got, name, scene, f"{name} [{fill}]")
    key = _BASELINE.setdefault(name, c.output_bytes())
    for (n1, a), (_, b) in zip(c.output_bytes(), key):
        assert np.array_equal(a, b), (fill, n1)


def test_empty_batch_and_empty_clouds(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    kw = dict(salient_radius=0.1, non_max_radius=0.1)
    for shape in ((0, 5, 3), (0, 0, 3), (4, 0, 3)):
        r = f.iss_keypoints(torch.zeros(shape, device=dev), **kw)
        assert r.mask.shape == shape[:2] and r.eigenvalues.shape == shape and r.num_keypoints.tolist() == [0] * shape[0]


def test_keypoints_to_padded_and_cloud_resolution_against_numpy(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    r = _public(dev, "ragged-1000")
    idx, num = f.keypoints_to_padded(r.mask)
    mask = r.mask.cpu().numpy()
    assert torch.equal(num, r.num_keypoints) and idx.dtype == torch.int64 and idx.shape == (3, int(mask.sum(1).max()))
    for n in range(3):
        rows = np.flatnonzero(mask[n])
        assert idx[n].tolist() == rows.tolist() + [-1] * (idx.shape[1] - len(rows))
    idx0, num0 = f.keypoints_to_padded(torch.zeros((2, 7), dtype=torch.bool, device=dev))
    assert idx0.shape == (2, 0) and num0.tolist() == [0, 0]
    pts, lengths = _scene("ragged-1000")[:2]
    res = f.cloud_resolution(torch.from_numpy(pts).to(dev), torch.from_numpy(lengths).to(dev)).cpu().numpy()
    p = pts[2].astype(np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(2))
    np.fill_diagonal(d, np.inf)
    assert res.dtype == np.float32 and res[:2].tolist() == [0.0, 0.0]
    assert abs(res[2] - d.min(1).mean()) <= 1e-5 * d.min(1).mean()  # (float32 distances and a float32 mean of 1000 terms)


def test_bad_arguments_are_rejected_with_nothing_written(dev):
    from pytorch3d_pointops_amd import _C
    from pytorch3d_pointops_amd import functions as f

    X = torch.rand(1, 8, 3, device=dev)
    kw = dict(salient_radius=0.1, non_max_radius=0.1)
    for bad in (dict(salient_radius=0.0), dict(salient_radius=-1.0), dict(non_max_radius=float("inf")),
                dict(non_max_radius=float("nan")), dict(salient_radius=1e39), dict(gamma_21=0.0),
                dict(gamma_32=float("nan")), dict(min_neighbors=-1), dict(min_neighbors=2.5)):
        with pytest.raises(ValueError):
            f.iss_keypoints(X, **{**kw, **bad})
    for pts, lengths in ((torch.rand(1, 8, 2, device=dev), None), (X.double(), None), (X[0], None),
                         (X, torch.tensor([8, 8], device=dev)), (X, torch.tensor([8], dtype=torch.int32, device=dev)),
                         (X, [8])):
        with pytest.raises(ValueError):
            f.iss_keypoints(pts, lengths, **kw)
    with pytest.raises(ValueError):
        f.keypoints_to_padded(torch.zeros(2, 3, device=dev))
    outs = [torch.full((256,), 7, dtype=torch.uint8, device=dev) for _ in range(4)]
    ws = torch.zeros(_C._lib.pointops_iss_workspace_bytes(1, 8), dtype=torch.uint8, device=dev)
    assert _C._lib.pointops_iss_workspace_bytes(1, 2 ** 24 + 1) == 0
    for bad in (dict(rs=0.0), dict(rs=-1.0), dict(rn=float("inf")), dict(rn=float("nan")), dict(rn=0.0), dict(g21=0.0),
                dict(g32=float("nan")), dict(mn=-1), dict(P=2 ** 24 + 1), dict(N=65536)):
        a = dict(rs=0.1, rn=0.1, g21=0.975, g32=0.975, mn=5, N=1, P=8)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.iss_keypoints("iss_keypoints", dev, X, None, a["N"], a["P"], a["rs"], a["rn"], a["g21"], a["g32"],
                                   a["mn"], *outs, ws, ws.numel())
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
