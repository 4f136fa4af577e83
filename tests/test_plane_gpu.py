"""GPU suite of segment_plane / segment_planes against the numpy checker tests/plane_ref.py, in stages, so that no
threshold decision is compared across precisions:

  1  drawn samples                bit-equal to the checker's integers
  2  hypothesis planes            validity flags bit-equal to the float64 checker on the DEVICE's samples; planes within one
                                  fp32 ulp of the float64 plane rounded once; invalid slots hold zeros
  3  counts                       bit-equal to the float32 checker on the DEVICE's planes, -1 for invalid slots
  4  best                         exact from the DEVICE's counts
  5  final mask, num_inliers      bit-equal to the float32 evaluation of the DEVICE's final plane; rmse against float64
                                  within plane_ref.rmse_bound; on scenes with margins also the refinement chain
  6  planted sets                 the mask is the planted set, the plane is the float64 eigh fit of that set

What stage 6 asserts is established on the CPU by test_plane_cpu.py::test_gpu_scene_is_reachable."""
import numpy as np
import pytest
import torch

import buffers
import plane_ref as ref
import ransac_ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
_RUNS = {}
_RMSE_WORST = [0.0, 0.0]  # (largest |rmse - rmse64|, its bound)
NAMES = "planes mask num_inliers rmse best counts hyp samples".split()


def _api():
    from pytorch3d_pointops_amd import functions

    return functions


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _call(dev, X, lengths=None, mask=None, *, thr=ref.THR, H=256, refine_steps=2, seed=0, samples=None, axis=None,
          max_angle_deg=None, hypotheses=True):
    """segment_plane on numpy inputs through the boundary (lengths as a tensor: the boundary takes them)."""
    from pytorch3d_pointops_amd import _C_plane

    cone = ref.cone_of(axis, max_angle_deg)
    out = _C_plane.segment_plane(_t(X, dev), _t(lengths, dev), _t(mask, dev), _t(samples, dev),
                                 H if samples is None else samples.shape[1], seed, float(np.float32(thr)),
                                 None if cone is None else [float(v) for v in cone[0]],
                                 None if cone is None else float(cone[1]), refine_steps, want_hypotheses=hypotheses)
    return {k: _np(v) for k, v in zip(NAMES, out)}


def _bars(X):
    return 1e-5, 1e-5 * (1.0 + (np.abs(X).max() if X.size else 0.0))


def check_stages(got, X, lengths, mask, kw, given_samples=None, first_cloud=0, chain=False):
    """Stages 1-5 of the module docstring on one result."""
    N, P = X.shape[:2]
    H = got["counts"].shape[1]
    thr = kw["thr"]
    cone = ref.cone_of(kw.get("axis"), kw.get("max_angle_deg"))
    rows = ref.valid_rows(lengths, mask, N, P)
    # 1
    want_samples = given_samples if given_samples is not None else ref.draw_samples(rows, H, kw["seed"], first_cloud)
    assert np.array_equal(got["samples"], want_samples)
    # 2
    p, ok = ref.gather_triples(X, rows, got["samples"])
    pl32, valid, pl64 = ref.planes_of(p, ok, cone)
    assert np.array_equal(got["counts"] >= 0, valid)
    assert not got["hyp"][~valid].any() and np.isfinite(got["hyp"]).all()
    assert (np.abs(got["hyp"].astype(np.float64) - pl32.astype(np.float64)) <= ref.ulp32(pl64)).all()
    # 3
    want_counts = ref.counts(got["hyp"], valid, X, rows, thr, np.float32)
    assert np.array_equal(got["counts"], want_counts)
    # 4
    best = ransac_ref.select(got["counts"])
    assert np.array_equal(got["best"], best)
    # 5
    m, num, _ = ref.evaluate(got["planes"], X, rows, thr, np.float32)
    none = best < 0
    m[none], num[none] = False, 0
    assert np.array_equal(got["mask"], m) and np.array_equal(got["num_inliers"], num)
    assert not got["planes"][none].any() and not got["rmse"][none].any()
    err = np.abs(got["rmse"] - ref.rmse64(got["planes"], X, got["mask"]))
    bound = ref.rmse_bound(got["planes"], X, thr)
    if N:
        k = int(np.argmax(err / bound))
        if err[k] > _RMSE_WORST[0]:
            _RMSE_WORST[:] = [float(err[k]), float(bound[k])]
        print(f"rmse: largest |device - float64| = {err.max():.3e} (bound {bound[k]:.3e})")
    assert (err <= bound).all()
    if chain:  # the refinement from the device's winner: fits in float64, decisions in float32
        n, b = np.arange(N), np.maximum(best, 0)
        planes, cmask, cnum, _, accepted = ref.refine(got["hyp"][n, b], best, X, rows, thr, kw["refine_steps"], cone,
                                                      np.float32)
        assert np.array_equal(got["mask"], cmask) and np.array_equal(got["num_inliers"], cnum)
        bar_n, bar_d = _bars(X)
        assert np.abs(got["planes"][:, :3] - planes[:, :3]).max() <= bar_n
        assert np.abs(got["planes"][:, 3] - planes[:, 3]).max() <= bar_d
        return accepted
    return None


def _scene_run(dev, name):
    if name not in _RUNS:
        sc, kw = ref.make_scene(name)
        _RUNS[name] = (sc, kw, _call(dev, sc["X"], sc["len"], sc["mask"], **kw))
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("name", list(ref.SCENES))
def test_scene_in_stages(dev, name):
    sc, kw, got = _scene_run(dev, name)
    planted = ref.SCENES[name].get("planted", True)
    check_stages(got, sc["X"], sc["len"], sc["mask"], kw, chain=planted)
    if not planted:
        return
    # 6
    assert np.array_equal(got["mask"], sc["planted"])
    assert np.array_equal(got["num_inliers"], sc["planted"].sum(1))
    if kw["refine_steps"] > 0:  # the final plane is the float64 least-squares plane of the planted set
        fit, lam = ref.planted_fit(sc, ref.cone_of(kw["axis"], kw["max_angle_deg"]))
        assert (lam[:, 1] >= 0.01 * lam[:, 2]).all()
        bar_n, bar_d = _bars(sc["X"])
        assert np.abs(got["planes"][:, :3] - fit[:, :3]).max() <= bar_n
        assert np.abs(got["planes"][:, 3] - fit[:, 3]).max() <= bar_d
    # every planted row within thr of the device's plane, in float64, and the planted normal recovered: a plane that
    # holds a patch of extent 1 x 1 (its rows at most 0.1 thr off the planted plane) within thr leans by at most
    # asin(2.2 thr / 0.9) < 0.13 (thr <= 0.05) from it once the patch spans 0.9, and 1 - cos 0.13 < 0.009
    for n in range(len(sc["X"])):
        r = ref.residual(got["planes"][n], sc["X"][n, sc["planted"][n]], np.float64)
        assert np.abs(r).max() <= kw["thr"] * (1.0 + 1e-3)
        assert abs(float(got["planes"][n, :3].astype(np.float64) @ sc["normal"][n])) >= 1.0 - 0.009


def test_cone_outside_throws_the_floor_out(dev):
    sc, kw = ref.cone_outside_scene()
    got = _call(dev, sc["X"], **kw)
    check_stages(got, sc["X"], None, None, kw, chain=False)
    free = _call(dev, sc["X"], **dict(kw, axis=None, max_angle_deg=None))
    assert np.array_equal(free["mask"], sc["planted"])
    assert (got["counts"] >= 0).sum() < (free["counts"] >= 0).sum()
    assert got["num_inliers"][0] < 0.2 * sc["planted"].sum()
    assert got["best"][0] < 0 or got["planes"][0, 2] >= np.cos(np.radians(10.0)) - 1e-6


def test_axis_turns_the_normal(dev):
    """The same floor with the axis up and down: the same rows, the plane negated."""
    sc, kw = ref.make_scene("cone-in")
    up = _scene_run(dev, "cone-in")[2]
    down_kw = dict(kw, axis=(0.0, 0.0, -1.0))
    down = _call(dev, sc["X"], **down_kw)
    check_stages(down, sc["X"], None, None, down_kw, chain=True)
    assert np.array_equal(up["mask"], down["mask"]) and up["planes"][0, 2] > 0 > down["planes"][0, 2]
    assert np.array_equal(up["planes"], -down["planes"])


def test_small_clouds_beside_a_normal_one(dev):
    """M = 0, 1, 2, 3 valid rows through the mask, a zero-length cloud, a ragged one and a normal cloud in one batch."""
    sc = ref.scene(41, 64, 0.6, N=7)
    X = sc["X"]
    lengths = np.full(7, 64, np.int64)
    mask = np.ones((7, 64), bool)
    for n, M in enumerate((0, 1, 2, 3)):
        mask[n] = False
        mask[n, np.nonzero(sc["planted"][n])[0][:M]] = True
    lengths[4] = 0
    lengths[5] = 40
    kw = dict(thr=ref.THR, H=64, refine_steps=2, seed=5)
    got = _call(dev, X, lengths, mask, **kw)
    check_stages(got, X, lengths, mask, kw, chain=True)
    assert got["best"][[0, 1, 2, 4]].tolist() == [-1] * 4 and (got["samples"][[0, 1, 2, 4]] == -1).all()
    assert got["best"][3] >= 0 and got["num_inliers"][3] == 3
    assert not got["mask"][5, 40:].any() and got["num_inliers"][5] >= 10 and got["num_inliers"][6] >= 20
    off = _call(dev, X, lengths, np.zeros((7, 64), bool), **kw)  # mask all false
    check_stages(off, X, lengths, np.zeros((7, 64), bool), kw)
    assert (off["best"] == -1).all() and not off["mask"].any() and not off["planes"].any()


def test_given_samples(dev):
    """The caller's triples: an invalid row, a duplicated row, a masked row and an all-invalid cloud give counts of -1
    and the zero plane; nothing is drawn."""
    sc = ref.scene(42, 100, 0.5, N=2)
    X = sc["X"]
    p = np.nonzero(sc["planted"][0])[0]
    mask = np.ones((2, 100), bool)
    mask[0, p[9]] = False
    samples = np.array([[[p[0], p[1], p[2]], [p[3], -1, p[4]], [p[5], p[5], p[6]], [p[7], p[8], 100], [p[2], p[1], p[0]],
                         [p[0], p[9], p[1]]], [[100, 101, 102]] * 6], np.int64)
    kw = dict(thr=ref.THR, refine_steps=1, seed=0)
    got = _call(dev, X, None, mask, samples=samples, **kw)
    check_stages(got, X, None, mask, kw, given_samples=samples)
    assert (got["counts"][0] >= 0).tolist() == [True, False, False, False, True, False]
    assert (got["counts"][1] == -1).all() and got["best"].tolist() == [0, -1]
    assert not got["mask"][1].any() and got["num_inliers"][1] == 0 and got["num_inliers"][0] >= 3
    assert not got["mask"][0, p[9]]


def test_hand_case_and_degenerate_clouds_are_exact(dev):
    """tests/test_plane_cpu.py's hand case on the device: the threshold on both sides, to the bit; collinear, coincident
    and NaN triples and an all-collinear cloud give the zero plane."""
    X = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0], [0, 0, 5]]] * 3, np.float32)
    for n, z in enumerate((0.25, 0.25 - 2.0 ** -24, 0.25 + 2.0 ** -23)):
        X[n, 3, 2] = np.float32(z)
    samples = np.array([[[0, 1, 2], [2, 2, 1], [0, 1, 7], [0, 1, 4]]] * 3, np.int64)
    got = _call(dev, X, thr=0.25, samples=samples, refine_steps=0)
    assert np.array_equal(got["hyp"][:, 0], np.array([[0, 0, 1, 0]] * 3, np.float32))
    assert got["counts"].tolist() == [[4, -1, -1, 3], [4, -1, -1, 3], [3, -1, -1, 3]]
    assert got["best"].tolist() == [0, 0, 0] and got["num_inliers"].tolist() == [4, 4, 3]
    assert got["mask"].tolist() == [[True, True, True, True, False]] * 2 + [[True, True, True, False, False]]
    nan = np.float32(np.nan)
    D = np.stack([np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6], [0.5, 1, 1.5]], np.float32),
                  np.ones((4, 3), np.float32),
                  np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]], np.float32),
                  np.array([[0, 0, 0], [1, 0, 0], [0, nan, 0], [nan, nan, nan]], np.float32)])
    ds = np.array([[[0, 1, 2], [1, 2, 3], [0, 2, 3], [3, 2, 1]]] * 4, np.int64)
    kw = dict(thr=0.1, refine_steps=2, seed=0)
    bad = _call(dev, D, samples=ds, **kw)
    check_stages(bad, D, None, None, kw, given_samples=ds)
    assert (bad["counts"] == -1).all() and (bad["best"] == -1).all() and not bad["planes"].any()
    line = (np.arange(50, dtype=np.float32)[:, None] * np.array([1, 2, 3], np.float32))[None]
    kw = dict(thr=0.1, H=64, refine_steps=2, seed=0)
    drawn = _call(dev, line, **kw)
    check_stages(drawn, line, None, None, kw)
    assert (drawn["samples"] >= 0).all() and (drawn["counts"] == -1).all() and drawn["best"][0] == -1


def test_rejected_refinement_keeps_the_winner(dev):
    X, samples, thr = ref.rejected_refit_scene()
    kw = dict(thr=thr, refine_steps=3, seed=0)
    got = _call(dev, X, samples=samples, **kw)
    accepted = check_stages(got, X, None, None, kw, given_samples=samples, chain=True)
    assert accepted.tolist() == [0] and got["num_inliers"].tolist() == [9]
    assert np.array_equal(got["planes"], got["hyp"][:, 0])
    free = _call(dev, X, samples=samples, **dict(kw, refine_steps=0))
    for k in ("planes", "mask", "num_inliers", "rmse"):
        assert np.array_equal(got[k], free[k]), k


@pytest.mark.parametrize("steps", [0, 1, 2, 3])
def test_refits_follow_the_chain(dev, steps):
    sc, kw = ref.make_scene("p1000")
    kw = dict(kw, refine_steps=steps, H=256)
    got = _call(dev, sc["X"], sc["len"], sc["mask"], **kw)
    accepted = check_stages(got, sc["X"], sc["len"], sc["mask"], kw, chain=True)
    assert (accepted <= steps).all() and (steps == 0 or accepted.min() >= 1)


def test_empty_batch_and_empty_clouds(dev):
    """N == 0 launches nothing; P == 0 is the zero result, fully written."""
    for N, P in ((0, 5), (2, 0), (0, 0)):
        X = np.ones((N, P, 3), np.float32)
        got = _call(dev, X, H=5, refine_steps=1)
        assert got["mask"].shape == (N, P) and got["counts"].shape == (N, 5) and got["samples"].shape == (N, 5, 3)
        assert not got["mask"].any() and (got["best"] == -1).all() and (got["counts"] == -1).all()
        assert (got["samples"] == -1).all() and not got["num_inliers"].any() and not got["rmse"].any()
        assert not got["planes"].any() and not got["hyp"].any()
    samples = np.zeros((2, 3, 3), np.int64)
    got = _call(dev, np.ones((2, 0, 3), np.float32), samples=samples)
    assert (got["counts"] == -1).all() and np.array_equal(got["samples"], samples) and not got["planes"].any()


def test_public_function_and_pointclouds(dev):
    """The public wrapper: a namedtuple of tensors that never require grad, None without return_hypotheses, lengths
    from Pointclouds equal to the padded call through the boundary; Pointclouds.segment_plane forwards."""
    from pytorch3d_pointops_amd.structures import Pointclouds

    f = _api()
    sc, kw, got = _scene_run(dev, "p1000")
    X = _t(sc["X"], dev).requires_grad_(True)
    pc = Pointclouds([X[n, :int(sc["len"][n])].detach() for n in range(3)])
    P = int(sc["len"].max())
    args = dict(distance_threshold=kw["thr"], num_hypotheses=kw["H"], seed=kw["seed"], refine_steps=kw["refine_steps"])
    sol = f.segment_plane(pc, return_hypotheses=True, **args)
    assert isinstance(sol, f.PlaneSegmentation)
    assert sol.inliers.dtype == torch.bool and sol.num_inliers.dtype == torch.int64 and sol.best.dtype == torch.int64
    assert sol.counts.dtype == torch.int32 and sol.samples.dtype == torch.int64 and sol.hypotheses.shape == (3, kw["H"], 4)
    assert np.array_equal(_np(sol.inliers), got["mask"][:, :P]) and np.array_equal(_np(sol.planes), got["planes"])
    assert np.array_equal(_np(sol.best), got["best"]) and np.array_equal(_np(sol.samples), got["samples"])
    method = pc.segment_plane(**args)
    assert torch.equal(method.planes, sol.planes) and torch.equal(method.inliers, sol.inliers)
    plain = f.segment_plane(X[:1], distance_threshold=kw["thr"], num_hypotheses=64)
    assert plain.counts is None and plain.hypotheses is None and plain.samples is None
    assert not any(t.requires_grad for t in plain[:5])


# ------------------------------------------------------------------------------------------------ determinism, streams
def _solve(f, X, kw, mask=None):
    r = f.segment_plane(X, distance_threshold=kw["thr"], num_hypotheses=kw["H"], seed=kw["seed"],
                        refine_steps=kw["refine_steps"], mask=mask, axis=kw.get("axis"),
                        max_angle_deg=kw.get("max_angle_deg"), return_hypotheses=True)
    return tuple(r)


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def test_two_runs_are_bit_equal_and_a_side_stream_too(dev):
    sc, kw = ref.make_scene("2chunk+1")
    X, mask = _t(sc["X"], dev), _t(sc["mask"], dev)
    first = _solve(_api(), X, kw, mask)
    assert _same(first, _solve(_api(), X, kw, mask))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = _solve(_api(), X, kw, mask)
    side.synchronize()
    assert _same(first, other)


@pytest.mark.parametrize("knobs", ["plane_lds=1", "plane_lds=0", "plane_hpl=1", "plane_hpl=2", "plane_lds=0,plane_hpl=1",
                                   "plane_lds=0,plane_hpl=2"])
@pytest.mark.parametrize("name", ["chunk-1", "2chunk+1", "h65", "p1000"])
def test_scoring_variants_change_nothing(dev, monkeypatch, name, knobs):
    """POINTOPS_DEBUG=plane_lds=1 sends the records through an LDS tile, plane_lds=0 through the scalar path, and
    plane_hpl sets the hypotheses per lane: every output is bit-equal to the default's, whichever form that is."""
    sc, kw, want = _scene_run(dev, name)
    monkeypatch.setenv("POINTOPS_DEBUG", knobs)
    got = _call(dev, sc["X"], sc["len"], sc["mask"], **kw)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_graph_capture_replays_the_eager_result(dev):
    from pytorch3d_pointops_amd import graphs

    sc, kw = ref.make_scene("chunk+1")
    X, mask = _t(sc["X"], dev), _t(sc["mask"], dev)
    want = _solve(_api(), X, kw, mask)
    x = X.clone()
    step = graphs.capture(lambda a: _solve(_api(), a, kw, mask), (x,))
    assert _same(step(), want)
    sc2 = ref.scene(51, sc["X"].shape[1], 0.5)  # other points through the static input, the same mask
    X2 = _t(sc2["X"], dev)
    assert _same(step(X2), _solve(_api(), X2, kw, mask))


# ------------------------------------------------------------------------------------------------ buffer contract
_BASELINE = {}


def _under_contract(monkeypatch, dev, fill):
    sc, kw = ref.make_scene("p257")
    sib = ref.scene(52, 257, 0.5)
    X, S = _t(sc["X"], dev), _t(sib["X"], dev)
    short = "short" if fill == "ones" else False
    with buffers.contract(monkeypatch, fill, short_workspace=short, prototypes=PROTOS) as c:
        c.sibling(lambda: _solve(_api(), S, kw))
        c.watch(X=X)
        out = _solve(_api(), X, kw)
    c.assert_all_clear()
    assert [b.kind for b in c.buffers] == ["out"] * 8 + ["workspace"] and c.inputs_checked >= 1
    if short:
        assert {(n, how) for n, _, how in c.rejections} == {("pointops_segment_plane", "short"),
                                                            ("pointops_segment_plane", "null")}
    _, _, got = _scene_run(dev, "p257")
    assert np.array_equal(_np(out[1]), got["mask"]) and np.array_equal(_np(out[5]), got["counts"])
    return c.output_bytes()


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_buffer_contract(monkeypatch, dev, fill):
    got = _under_contract(monkeypatch, dev, fill)
    if "zero" not in _BASELINE:
        _BASELINE["zero"] = got if fill == "zero" else _under_contract(monkeypatch, dev, "zero")
    want = _BASELINE["zero"]
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert np.array_equal(a, b), (fill, name)


def test_bad_shapes_are_rejected_with_nothing_written(dev):
    from pytorch3d_pointops_amd import _C, _C_plane

    X = torch.rand(1, 8, 3, device=dev)
    with pytest.raises(RuntimeError, match="segment_plane"):
        _C_plane.segment_plane(X, None, torch.ones(1, 7, dtype=torch.bool, device=dev), None, 4, 0, 0.1, None, None, 1)
    with pytest.raises(RuntimeError, match="segment_plane"):
        _C_plane.segment_plane(X[..., :2], None, None, None, 4, 0, 0.1, None, None, 1)
    outs = [torch.full((64,), 7, dtype=torch.uint8, device=dev) for _ in range(5)]
    ws = torch.zeros(_C._lib.pointops_plane_workspace_bytes(1, 8, 4), dtype=torch.uint8, device=dev)
    for bad in (dict(H=0), dict(thr=-1.0), dict(thr=float("inf")), dict(refine=-1), dict(first=-1),
                dict(axis=(0.0, 0.0, 2.0)), dict(cosm=1.5), dict(cosm=-0.5)):
        a = dict(H=4, thr=0.1, refine=1, first=0, axis=(0.0, 0.0, 1.0), cosm=0.5)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.segment_plane("segment_plane", dev, X, None, None, None, 1, 8, a["H"], 0, a["first"], a["thr"], 1,
                                   *a["axis"], a["cosm"], a["refine"], *outs, None, None, None, ws, ws.numel())
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ big batch
def test_batch_of_65537_clouds_draws_by_the_global_index(dev):
    """One batch over the entry's limit goes in slices; clouds 0, 65 534, 65 535 and 65 536 equal the checker run on
    each alone with its index in the batch as first_cloud."""
    N, P, H = 65537, 8, 8
    rng = np.random.default_rng(7500)
    X = rng.uniform(0, 1, (N, P, 3)).astype(np.float32)
    X[:, :6, 2] = np.float32(0.5)  # six rows on z = 0.5, two well off it
    X[:, 6:, 2] = np.float32(0.5) + rng.choice([-1.0, 1.0], (N, 2)).astype(np.float32) * np.float32(0.25)
    kw = dict(thr=ref.THR, H=H, refine_steps=1, seed=77)
    got = _call(dev, X, **kw)
    for n in (0, 65534, 65535, 65536):
        one = {k: v[n:n + 1] for k, v in got.items()}
        check_stages(one, X[n:n + 1], None, None, kw, first_cloud=n)
    assert (got["best"] >= 0).all() and (got["num_inliers"] >= 3).all()
    assert not np.array_equal(got["samples"][0], got["samples"][65535])  # (a restart at 0 would repeat cloud 0's draws)


# ------------------------------------------------------------------------------------------------ several planes, end to end
def test_segment_planes_peels_floor_and_wall(dev):
    """Floor, wall, shelf and clutter (test_plane_cpu.py::planes_scene, reachable there): labels equal the planted ones,
    the planes come in the order of their sizes, and the third plane, below min_inliers, is reported as zeros."""
    from test_plane_cpu import planes_scene

    f = _api()
    Xn, labels, thr = planes_scene()
    X = _t(Xn, dev)
    out = f.segment_planes(X, 3, min_inliers=300, distance_threshold=thr, num_hypotheses=512, seed=40)
    assert isinstance(out, f.PlaneSet) and out.planes.shape == (1, 3, 4) and out.labels.dtype == torch.int64
    want = np.where(labels <= 1, labels, -1)
    assert np.array_equal(_np(out.labels), want)
    assert _np(out.num_inliers).tolist() == [[1500, 900, 0]] and not _np(out.planes)[0, 2].any()
    planes = _np(out.planes)[0].astype(np.float64)
    assert abs(planes[0, 2]) >= 1.0 - 1e-4 and abs(planes[0, 3]) <= 1e-3                 # z = 0
    assert abs(planes[1, 0]) >= 1.0 - 1e-4 and abs(abs(planes[1, 3]) - 0.6) <= 1e-3      # x = -0.6
    # call k is segment_plane with seed + k on what is left
    first = f.segment_plane(X, distance_threshold=thr, num_hypotheses=512, seed=40)
    second = f.segment_plane(X, distance_threshold=thr, num_hypotheses=512, seed=41, mask=~first.inliers)
    assert torch.equal(out.planes[:, 0], first.planes) and torch.equal(out.planes[:, 1], second.planes)
    # a min_inliers nobody meets: nothing counts, and later planes do not count either
    none = f.segment_planes(X, 2, min_inliers=2000, distance_threshold=thr, num_hypotheses=512, seed=40)
    assert (_np(none.labels) == -1).all() and not _np(none.planes).any() and not _np(none.num_inliers).any()


def test_floor_removal_lets_dbscan_see_the_objects(dev):
    """A floor and three blobs resting on it: cluster_dbscan on all points finds one cluster (everything is
    density-connected through the floor), on ~inliers three."""
    f = _api()
    Xn, floor, eps, min_points, thr = ref.floor_and_blobs_scene()  # (reachable: test_plane_cpu.py)
    X = _t(Xn, dev)
    whole = f.cluster_dbscan(X, eps, min_points)
    assert int(whole.num_clusters[0]) == 1
    seg = f.segment_plane(X, distance_threshold=thr, num_hypotheses=256, seed=3, axis=(0, 0, 1), max_angle_deg=15.0)
    assert np.array_equal(_np(seg.inliers), floor) and float(seg.planes[0, 2]) > 0.999
    rest = ~seg.inliers
    objects = f.cluster_dbscan(X[rest][None], eps, min_points)
    assert int(objects.num_clusters[0]) == 3 and int((objects.labels >= 0).sum()) == 480


def test_zz_report_rmse(dev):
    """Not a check of its own: prints the largest rmse error the tests above saw against its bound."""
    print(f"largest |rmse - float64 rmse| on the device: {_RMSE_WORST[0]:.3e} (bound {_RMSE_WORST[1]:.3e})")
    assert _RMSE_WORST[0] <= _RMSE_WORST[1] or _RMSE_WORST[1] == 0.0
