"""smooth_mls on the GPU against the numpy checker of tests/mls_ref.py, stage by stage, so that no stage's rounding hides
another's error:

    moments        equal to the checker's                                     (integers: no tolerance)
    num_neighbors  equal to the checker's
    status         equal to the checker's (the scenes keep l1 / l2 far from 2^-20: ~1e-17 on a line, > 1e-3 elsewhere)
    curvature      within 2^-23 |c| + 2^-40 of the checker's float64 quotient: the rounding to float32 is 2^-24 relative,
                   the rest is the backward error of two float64 eigensolvers (a few 2^-53 l2 each) with room
    normals        unit vectors within 2^-22; on WELL-CONDITIONED rows (l1 - l0 >= 0.05 l2) equal to the checker's
                   sign-fixed eigh vector within 2^-24 + 1e-12 per component: the rounding to float32 (2^-24 of a
                   component of at most 1), the Jacobi's stopping rule (off-diagonal mass <= 1e-15 |diag|, so an angle
                   of at most 1e-15 * sqrt(3) l2 / (0.05 l2) = 3.5e-14) and the float64 roundings of both solvers
                   (about 100 * 2^-53 l2 over the same gap: 2.2e-13)
    points         within |h| 2^-22 + 1/2 ulp of fl32(x + (delta . n^) n^), evaluated in float64 from the checker's delta
                   and the DEVICE's returned float32 normal n^.  The definition moves the point along n^ itself, not
                   along the float64 eigenvector it is the rounding of: delta has a part ALONG the surface of up to 4500
                   times |h| in these scenes (a support at the rim of a cloud is one-sided), and with the unrounded
                   vector that part times the rounding of n^, |delta| 2^-24, would exceed the bound on a few rows (9 of
                   1800 components of the sphere, by a factor of up to 1.98, when measured that way).
    rows of status 1 and 2: the input point's bits, normal 0, curvature 0; padding rows: 0

Every call goes through the guarded, poisoned buffers of tests/buffers.py (fill 0xFF, short and null workspaces tried
first).  Each scene runs three ways -- as the library chooses (grids from 512 points per cloud on), with
POINTOPS_DEBUG=mls_grid=0 (all pairs) and mls_grid=1 (a grid whatever the size) -- and the three are bit-equal in every
output, moments included.  The checker's result of a scene is computed once."""
import numpy as np
import pytest
import torch

import buffers
import mls_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
MODES = {"default": None, "allpairs": "mls_grid=0", "grid": "mls_grid=1"}
KEYS = ("points", "normals", "curvature", "num_neighbors", "status", "moments")
ENTRY = "pointops_mls_smooth"


def _plane(P, seed, r=0.15):
    return ref.noisy_plane(P, seed=seed)[None], None, r


def _ragged():
    """N = 4 clouds of 600 rows with lengths (0, 1, 2, 600)."""
    return np.stack([ref.noisy_plane(600, seed=30 + n) for n in range(4)]), np.array([0, 1, 2, 600], np.int64), 0.15


def _one_empty():
    """N = 3 with one empty cloud between a full and a half-full one."""
    pts = np.stack([ref.noisy_sphere(600, seed=40), ref.noisy_sphere(600, seed=41), ref.noisy_sphere(600, seed=42)])
    return pts, np.array([600, 0, 300], np.int64), 0.3


def _isolated():
    far = np.array([[10.0 * (k + 1)] * 3 for k in range(5)], np.float32)
    return np.concatenate([ref.noisy_plane(595, seed=50), far])[None], None, 0.15


def _nan_row():
    p = ref.noisy_plane(600, seed=51).copy()
    p[7] = np.nan
    p[300, 1] = np.inf
    return p[None], None, 0.15


# name -> () -> (points (N, P, 3) float32, lengths or None, radius)
SCENES = {f"plane-{P}": (lambda P=P: _plane(P, P)) for P in (511, 512, 513, 768, 769, 1023)}
SCENES.update({
    "sphere": lambda: (ref.noisy_sphere()[None], None, 0.3),
    "ragged-0-1-2": _ragged,
    "one-empty": _one_empty,
    "doubled": lambda: (ref.doubled(ref.noisy_plane(300, seed=52))[None], None, 0.15),
    "collinear": lambda: (ref.collinear()[None], None, 0.1),
    "isolated": _isolated,
    "nan-row": _nan_row,
    "radius-above-cloud": lambda: _plane(520, 53, 5.0),
    "radius-power-of-two": lambda: _plane(600, 54, 0.25),
    "shifted-1000": lambda: ((ref.noisy_plane(600, seed=55).astype(np.float64) + 1000.0).astype(np.float32)[None], None,
                             0.15),
})
_BUILT, _WANT = {}, {}
MIN_NEIGHBORS = 3


def _scene(name):
    if name not in _BUILT:
        pts, lengths, r = SCENES[name]()
        _BUILT[name] = (np.ascontiguousarray(pts, np.float32), lengths, r)
    return _BUILT[name]


def _want(name, iterations=1):
    if (name, iterations) not in _WANT:
        pts, lengths, r = _scene(name)
        _WANT[name, iterations] = ref.smooth(pts, lengths, r, MIN_NEIGHBORS, iterations)
    return _WANT[name, iterations]


def _set_mode(monkeypatch, mode):
    if MODES[mode] is None:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    else:
        monkeypatch.setenv("POINTOPS_DEBUG", MODES[mode])


def _native(dev, monkeypatch, scene, iterations=1, fill="ones"):
    """The boundary call with the diagnostic moments, under the buffer contract -> ({key: numpy}, the contract)."""
    from pytorch3d_pointops_amd import _C_mls

    pts, lengths, r = scene
    P = torch.from_numpy(pts).to(dev)
    Lt = None if lengths is None else torch.from_numpy(lengths).to(dev)
    with buffers.contract(monkeypatch, fill, short_workspace="short", prototypes=PROTOS) as c:
        c.watch(points=P, lengths=Lt)
        out = _C_mls.mls_smooth(P, Lt, r, MIN_NEIGHBORS, iterations, want_moments=True)
    c.assert_all_clear()
    dtypes = [t.dtype for t in out]
    assert dtypes == [torch.float32, torch.float32, torch.float32, torch.int64, torch.uint8, torch.int64], dtypes
    assert out[5].shape == pts.shape[:2] + (10,) and out[0].shape == pts.shape
    return dict(zip(KEYS, (t.cpu().numpy() for t in out))), c


def _ulp(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _points_error(got, want, pts):
    """(|points - b|, |h|, b) with b = fl32(x + (delta . n^) n^), evaluated in float64 from the checker's delta and the
    device's normal; the error is 0 outside the rows of status 0."""
    nh = got["normals"].astype(np.float64)
    d = want["delta"]
    h = (d[..., 0] * nh[..., 0] + d[..., 1] * nh[..., 1]) + d[..., 2] * nh[..., 2]
    ok = want["live"] & (want["status"] == 0)
    with np.errstate(invalid="ignore"):  # (non-finite rows are never smoothed)
        b = (pts.astype(np.float64) + h[..., None] * nh).astype(np.float32)
        err = np.where(ok[..., None], np.abs(got["points"].astype(np.float64) - b.astype(np.float64)), 0.0)
    return err, np.abs(h), b


def _check_stages(got, want, pts, what):
    live = want["live"]
    for k in ("moments", "num_neighbors", "status"):
        bad = np.argwhere(got[k] != want[k])
        assert not len(bad), (f"{what}: {k} differs at {len(bad)} places, first {bad[0].tolist()}: got "
                              f"{got[k][tuple(bad[0])]}, want {want[k][tuple(bad[0])]}")
    ok = live & (want["status"] == 0)
    # rows that are not smoothed: the point's own bits, zeros elsewhere; padding: zeros
    keep = live & ~ok
    assert np.array_equal(got["points"].view(np.int32)[keep], pts.view(np.int32)[keep]), f"{what}: unsmoothed rows moved"
    assert not got["points"][~live].any() and not got["normals"][~ok].any() and not got["curvature"][~ok].any()
    e = want["eig"]
    with np.errstate(invalid="ignore", divide="ignore"):
        c64 = np.where(ok, e[..., 0] / ((e[..., 0] + e[..., 1]) + e[..., 2]), 0.0)
    cerr = np.abs(got["curvature"].astype(np.float64) - c64)
    ctol = 2.0 ** -23 * np.abs(c64) + 2.0 ** -40
    print(f"{what}: curvature: max |got - ref| = {float(cerr.max()) if cerr.size else 0.0:.3e}, "
          f"max excess = {float((cerr - ctol).max()) if cerr.size else 0.0:.3e}")
    assert (cerr <= ctol).all(), f"{what}: curvature beyond its bound at {np.argwhere(cerr > ctol)[0]}"
    nrm = np.linalg.norm(got["normals"].astype(np.float64), axis=-1)
    assert (np.abs(nrm - 1.0)[ok] <= 2.0 ** -22).all(), f"{what}: normals are not unit vectors"
    well = want["well"] & ok
    nerr = np.abs(got["normals"].astype(np.float64) - want["n"]).max(-1)
    print(f"{what}: {int(ok.sum())} smoothed rows, {int(well.sum())} well conditioned; normals: max |got - ref| = "
          f"{float(nerr[well].max()) if well.any() else 0.0:.3e} (bound {2.0 ** -24 + 1e-12:.3e})")
    assert (nerr[well] <= 2.0 ** -24 + 1e-12).all(), f"{what}: normals differ from the checker's on well-conditioned rows"
    perr, hn, b32 = _points_error(got, want, pts)
    ptol = (hn * 2.0 ** -22)[..., None] + 0.5 * _ulp(np.where(ok[..., None], b32, 1))
    print(f"{what}: points: max |got - b| / bound = {float((perr / ptol)[ok].max()) if ok.any() else 0.0:.3f}")
    assert (perr <= ptol)[ok].all(), f"{what}: points beyond their bound at {np.argwhere((perr > ptol) & ok[..., None])[0]}"


def _assert_bit_equal(a, b, what, keys=KEYS):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} is not bit-equal"


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_in_three_modes_equals_the_checker_stage_by_stage(dev, monkeypatch, name):
    scene = _scene(name)
    first = None
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        got, c = _native(dev, monkeypatch, scene)
        assert {(n, how) for n, _, how in c.rejections} == {(ENTRY, "short"), (ENTRY, "null")}
        assert [b.kind for b in c.buffers] == ["out"] * 6 + ["workspace"]
        if first is None:
            first = got
            _check_stages(got, _want(name), scene[0], f"{name} [{mode}]")
        else:
            _assert_bit_equal(got, first, f"{name} [{mode}] against [default]")


@pytest.mark.parametrize("name", ["sphere", "plane-1023"])
def test_points_within_the_bound_of_the_feature_request(dev, monkeypatch, name):
    """|points - fl32(x + (delta . n^) n^)| <= |h| 2^-22 + 1/2 ulp, delta the checker's, n^ the device's normal, as the
    feature request states it, on every smoothed row.

    The returned point is the returned normal's own projection (this file's docstring): both sides evaluate the same
    float64 expression of the same float32 vector, so the figures printed are those of delta alone.  (_check_stages
    holds every scene to the same bound; this test names it.)"""
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts = _scene(name)[0]
    got, _ = _native(dev, monkeypatch, _scene(name))
    want = _want(name)
    nh = got["normals"].astype(np.float64)
    d = want["delta"]
    h = (d[..., 0] * nh[..., 0] + d[..., 1] * nh[..., 1]) + d[..., 2] * nh[..., 2]
    b = (pts.astype(np.float64) + h[..., None] * nh).astype(np.float32)
    ok = want["live"] & (want["status"] == 0)
    err = np.abs(got["points"].astype(np.float64) - b.astype(np.float64))
    tol = np.abs(h)[..., None] * 2.0 ** -22 + 0.5 * _ulp(b)
    miss = (err > tol) & ok[..., None]
    print(f"{name}: {int(miss.sum())} of {3 * int(ok.sum())} components beyond |h| 2^-22 + 1/2 ulp, worst factor "
          f"{float((err / tol)[ok].max()):.3f}")
    assert not miss.any()


def test_what_the_scenes_are_meant_to_show(dev, monkeypatch):
    """The results have the features the scene names promise (the comparison above is only as good as its scenes)."""
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    run = lambda name: _native(dev, monkeypatch, _scene(name))[0]  # noqa: E731
    rms = lambda z: float(np.sqrt((z.astype(np.float64) ** 2).mean()))  # noqa: E731
    plane = run("plane-1023")
    assert (plane["status"] == 0).all() and rms(plane["points"][0, :, 2]) < 0.5 * rms(_scene("plane-1023")[0][0, :, 2])
    assert (plane["normals"][0, :, 2] > 0.9).all() and plane["num_neighbors"].min() >= 10
    sph = run("sphere")
    before = np.abs(np.linalg.norm(_scene("sphere")[0][0].astype(np.float64), axis=1) - 1.0)
    after = np.abs(np.linalg.norm(sph["points"][0].astype(np.float64), axis=1) - 1.0)
    assert rms(after) < 0.8 * rms(before) and (sph["curvature"] >= 0).all() and sph["curvature"].max() < 1 / 3
    rag = run("ragged-0-1-2")
    assert rag["status"][1, 0] == 1 and rag["num_neighbors"][1, 0] == 1 and rag["moments"][1, 0].tolist() == [4096] + [0] * 9
    assert rag["status"][2, :2].tolist() == [1, 1] and (rag["status"][3] == 0).mean() > 0.99
    assert not rag["moments"][0].any() and not rag["points"][0].any()
    dbl = run("doubled")
    for k in ("points", "normals", "curvature"):
        assert np.array_equal(dbl[k][0, :300], dbl[k][0, 300:]), k
    assert (dbl["num_neighbors"] % 2 == 0).all()
    col = run("collinear")
    assert (col["status"] == 2).all() and np.array_equal(col["points"], _scene("collinear")[0])
    iso = run("isolated")
    assert iso["status"][0, 595:].tolist() == [1] * 5 and (iso["status"][0, :595] == 0).all()
    nan = run("nan-row")
    assert nan["status"][0, 7] == 1 and nan["num_neighbors"][0, 7] == 0 and np.isnan(nan["points"][0, 7]).all()
    assert nan["status"][0, 300] == 1 and np.isposinf(nan["points"][0, 300, 1]) and (nan["status"][0] == 0).sum() >= 590
    big = run("radius-above-cloud")
    assert (big["num_neighbors"] == 520).all() and (big["status"] == 0).all()
    assert ref.exponent(0.25) == -2 and ref.exponent(np.nextafter(np.float32(0.25), np.float32(1))) == -1
    assert (run("radius-power-of-two")["status"] == 0).all()
    base = ref.smooth(ref.noisy_plane(600, seed=55)[None], None, 0.15)["num_neighbors"]
    assert (run("shifted-1000")["num_neighbors"] == base).mean() > 0.9  # (coordinates rounded to 2^-14)


def test_two_calls_and_a_ragged_batch_are_bit_equal(dev, monkeypatch):
    """Twice the same call; and every cloud alone, at its own length, against its rows inside the ragged batch."""
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    for name in ("one-empty", "ragged-0-1-2"):
        pts, lengths, r = _scene(name)
        first, _ = _native(dev, monkeypatch, (pts, lengths, r))
        again, _ = _native(dev, monkeypatch, (pts, lengths, r))
        _assert_bit_equal(again, first, f"{name}: second call")
        for n, ln in enumerate(lengths):
            if ln == 0:
                continue
            alone, _ = _native(dev, monkeypatch, (np.ascontiguousarray(pts[n:n + 1, :ln]), None, r))
            for k in KEYS:
                assert alone[k][0].tobytes() == first[k][n, :ln].tobytes(), f"{name}: cloud {n} alone: {k}"


@pytest.mark.parametrize("name", ["plane-511", "plane-769"])
def test_a_row_permutation_permutes_the_outputs(dev, monkeypatch, name):
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts, lengths, r = _scene(name)
    perm = np.random.default_rng(9).permutation(pts.shape[1])
    first, _ = _native(dev, monkeypatch, (pts, lengths, r))
    moved, _ = _native(dev, monkeypatch, (np.ascontiguousarray(pts[:, perm]), lengths, r))
    for k in KEYS:
        assert moved[k].tobytes() == np.ascontiguousarray(first[k][:, perm]).tobytes(), k


@pytest.mark.parametrize("name", ["plane-513", "one-empty", "plane-511"])
def test_two_iterations_are_two_calls(dev, monkeypatch, name):
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts, lengths, r = _scene(name)
    one, _ = _native(dev, monkeypatch, (pts, lengths, r))
    two_calls, _ = _native(dev, monkeypatch, (one["points"], lengths, r))
    for iterations, chain in ((2, two_calls), (3, _native(dev, monkeypatch, (two_calls["points"], lengths, r))[0])):
        got, c = _native(dev, monkeypatch, (pts, lengths, r), iterations=iterations)
        assert [b.kind for b in c.buffers] == ["out"] * 6 + ["workspace"]
        _assert_bit_equal(got, chain, f"{name}: iterations={iterations} against {iterations} calls")
    # the second pass against the checker's pass over the DEVICE's first-pass points (the checker's own differ from
    # them in last bits, which a support at the radius would turn into another moment)
    _check_stages(two_calls, ref.smooth_once(one["points"], lengths, r, MIN_NEIGHBORS), one["points"], f"{name}: second pass")


def _public(dev, name, via="tensor", **kw):
    from pytorch3d_pointops_amd import functions as f

    pts, lengths, r = _scene(name)
    P = torch.from_numpy(pts).to(dev)
    if via == "pointclouds":
        from pytorch3d_pointops_amd.structures import Pointclouds

        L = np.full(len(pts), pts.shape[1]) if lengths is None else lengths
        return Pointclouds([P[n, :int(L[n])] for n in range(len(pts))]).smooth_mls(radius=r, **kw)
    return f.smooth_mls(P, None if lengths is None else torch.from_numpy(lengths).to(dev), radius=r, **kw)


def test_public_call_and_pointclouds_route(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    assert {"smooth_mls", "MLSSmoothing"} <= set(f.__all__)
    want, _ = _native(dev, monkeypatch, _scene("one-empty"))
    for via in ("tensor", "pointclouds"):
        r = _public(dev, "one-empty", via)
        assert isinstance(r, f.MLSSmoothing) and r._fields == KEYS[:5]
        assert r.num_neighbors.dtype == torch.int64 and r.status.dtype == torch.uint8
        for k in KEYS[:5]:
            assert getattr(r, k).cpu().numpy().tobytes() == want[k].tobytes(), (via, k)
    r, mom = _public(dev, "one-empty", return_moments=True, min_neighbors=MIN_NEIGHBORS)
    assert mom.cpu().numpy().tobytes() == want["moments"].tobytes() and torch.equal(r.status.cpu(), torch.from_numpy(want["status"]))
    high = _public(dev, "one-empty", min_neighbors=10 ** 6)
    live = _want("one-empty")["live"]
    assert (high.status.cpu().numpy()[live] == 1).all() and torch.equal(
        high.points.cpu(), torch.from_numpy(np.where(live[..., None], _scene("one-empty")[0], np.float32(0))))


def test_graph_capture_of_two_iterations_replays_the_eager_bytes(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd import graphs

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    pts, lengths, r = _scene("one-empty")
    Lt = torch.from_numpy(lengths).to(dev)
    call = lambda a: tuple(f.smooth_mls(a, Lt, radius=r, iterations=2))  # noqa: E731
    P = torch.from_numpy(pts).to(dev)
    want = [t.clone() for t in call(P)]
    step = graphs.capture(call, (P.clone(),))
    for replay in range(2):
        got = step()
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got, want)), replay


def test_empty_batch_and_empty_clouds(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    for shape in ((0, 5, 3), (0, 0, 3), (4, 0, 3)):
        for iterations in (1, 2):
            r = f.smooth_mls(torch.zeros(shape, device=dev), radius=0.1, iterations=iterations)
            assert r.points.shape == shape and r.normals.shape == shape and r.status.shape == shape[:2]


def test_bad_arguments_are_rejected_with_nothing_written(dev):
    from pytorch3d_pointops_amd import _C
    from pytorch3d_pointops_amd import functions as f

    X = torch.rand(1, 8, 3, device=dev)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")),
                dict(radius=1e39), dict(radius=0.1, min_neighbors=-1), dict(radius=0.1, min_neighbors=2.5),
                dict(radius=0.1, iterations=0), dict(radius=0.1, iterations=1.5)):
        with pytest.raises(ValueError):
            f.smooth_mls(X, **bad)
    for pts, lengths in ((torch.rand(1, 8, 2, device=dev), None), (X.double(), None), (X[0], None),
                         (X, torch.tensor([8, 8], device=dev)), (X, torch.tensor([8], dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            f.smooth_mls(pts, lengths, radius=0.1)
    with pytest.raises(ValueError, match="2\\^20"):
        f.smooth_mls(torch.zeros(1, 2 ** 20 + 1, 3, device=dev), radius=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f.smooth_mls(torch.rand(1, 8, 3), radius=0.1)
    outs = [torch.full((1024,), 7, dtype=torch.uint8, device=dev) for _ in range(6)]
    ws = torch.zeros(_C._lib.pointops_mls_workspace_bytes(1, 8, 2), dtype=torch.uint8, device=dev)
    assert _C._lib.pointops_mls_workspace_bytes(1, 2 ** 20 + 1, 1) == 0 and _C._lib.pointops_mls_workspace_bytes(1, 8, 0) == 0
    for bad in (dict(r=0.0), dict(r=-1.0), dict(r=float("inf")), dict(r=float("nan")), dict(mn=-1), dict(it=0),
                dict(it=65537), dict(P=2 ** 20 + 1), dict(N=65536)):
        a = dict(r=0.1, mn=3, it=2, N=1, P=8)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.mls_smooth("mls_smooth", dev, X, None, a["N"], a["P"], a["r"], a["mn"], a["it"], *outs, ws,
                                ws.numel())
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
