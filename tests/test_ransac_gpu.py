"""GPU suite of ransac_alignment against the numpy checker tests/ransac_ref.py, in stages, so that no threshold decision
is compared across precisions:

  1  drawn samples                bit-equal to the checker's integers
  2  hypothesis transforms        float64 solve of the DEVICE's samples; validity flags bit-equal to the float32 checker
  3  counts                       bit-equal to the float32 checker on the DEVICE's transforms
  4  best                         exact from the DEVICE's counts
  5  final mask, num_inliers      bit-equal to the float32 evaluation of the DEVICE's final transform; rmse against
                                  float64 within ransac_ref.rmse_bound; on scenes with margins also the refinement chain
  6  planted sets                 the mask is the planted set, the motion is the planted motion to within the noise

What stage 6 asserts is established on the CPU by test_ransac_cpu.py::test_gpu_scene_is_reachable."""
import numpy as np
import pytest
import torch

import buffers
import ransac_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
_RUNS = {}
_RMSE_WORST = [0.0, 0.0]  # (largest |rmse - rmse64|, its bound)


def _api():
    from pytorch3d_pointops_amd import functions

    return functions


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _call(dev, X, Y, corr=None, len1=None, len2=None, *, thr=ref.THR, H=256, estimate_scale=False, ratio=0.9,
          refine_steps=2, seed=0, samples=None, hypotheses=True):
    """ransac_alignment on numpy inputs (lengths through Pointclouds-free padded tensors: the boundary takes them)."""
    from pytorch3d_pointops_amd import _C_ransac

    out = _C_ransac.ransac_alignment(_t(X, dev), _t(Y, dev), _t(corr, dev), _t(len1, dev), _t(len2, dev),
                                     _t(samples, dev), H if samples is None else samples.shape[1], seed, thr, ratio,
                                     estimate_scale, refine_steps, want_hypotheses=hypotheses)
    names = "R T s mask num_inliers rmse best counts hyp_R hyp_T hyp_s samples".split()
    return {k: _np(v) for k, v in zip(names, out)}


def _bars(Y):
    return 1e-5, 1e-5 * (1.0 + (np.abs(Y).max() if Y.size else 0.0))


def check_stages(got, X, Y, corr, len1, len2, kw, given_samples=None, first_cloud=0, chain=False):
    """Stages 1-5 of the module docstring on one result."""
    N, P1, P2 = X.shape[0], X.shape[1], Y.shape[1]
    H = got["counts"].shape[1]
    thr, es = kw["thr"], kw["estimate_scale"]
    tgt = ref.targets(corr, ref.lengths_of(len1, N, P1), ref.lengths_of(len2, N, P2), N, P1)
    # 1
    want_samples = given_samples if given_samples is not None else ref.draw_samples(tgt, H, kw["seed"], first_cloud)
    assert np.array_equal(got["samples"], want_samples)
    # 2
    x, y, ok = ref.gather_triples(X, Y, tgt, got["samples"])
    valid = ref.hypothesis_valid(x, y, ok, kw["ratio"], es, np.float32)
    assert np.array_equal(got["counts"] >= 0, valid)
    hR, hT, hs, S = ref.alignment(x, y, None, es)
    inv = ~valid
    assert np.array_equal(got["hyp_R"][inv], np.broadcast_to(np.eye(3, dtype=np.float32), (inv.sum(), 3, 3)))
    assert not got["hyp_T"][inv].any() and (got["hyp_s"][inv] == 1).all()
    well = valid & ref.well_determined(S)
    assert (valid & ~well).sum() <= 0.01 * max(valid.sum(), 1) or H < 100
    bar_R, bar_T = _bars(Y)
    if well.any():
        assert np.abs(got["hyp_R"][well] - hR[well]).max() <= bar_R
        assert np.abs(got["hyp_T"][well] - hT[well]).max() <= bar_T
        assert (np.abs(got["hyp_s"][well] - hs[well]) <= 1e-5 * hs[well]).all()
    for a in ("hyp_R", "hyp_T", "hyp_s"):
        assert np.isfinite(got[a]).all()
    # 3
    want_counts = ref.counts(got["hyp_R"], got["hyp_T"], got["hyp_s"], valid, X, Y, tgt, thr, np.float32)
    assert np.array_equal(got["counts"], want_counts)
    # 4
    best = ref.select(got["counts"])
    assert np.array_equal(got["best"], best)
    # 5
    mask, num, _ = ref.evaluate(got["R"], got["T"], got["s"], X, Y, tgt, thr, np.float32)
    none = best < 0
    mask[none], num[none] = False, 0
    assert np.array_equal(got["mask"], mask) and np.array_equal(got["num_inliers"], num)
    assert np.array_equal(got["R"][none], np.broadcast_to(np.eye(3, dtype=np.float32), (none.sum(), 3, 3)))
    assert not got["T"][none].any() and (got["s"][none] == 1).all() and not got["rmse"][none].any()
    err = np.abs(got["rmse"] - ref.rmse64(got["R"], got["T"], got["s"], X, Y, tgt, got["mask"]))
    bound = ref.rmse_bound(got["s"], got["T"], X, Y)
    k = int(np.argmax(err / bound))
    if err[k] > _RMSE_WORST[0]:
        _RMSE_WORST[:] = [float(err[k]), float(bound[k])]
    print(f"rmse: largest |device - float64| = {err.max():.3e} (bound {bound[k]:.3e})")
    assert (err <= bound).all()
    if chain:  # the refinement from the device's winner: fits in float64, decisions in float32
        n, b = np.arange(N), np.maximum(best, 0)
        R, T, s, cmask, cnum, _, accepted = ref.refine(got["hyp_R"][n, b], got["hyp_T"][n, b], got["hyp_s"][n, b], best,
                                                       X, Y, tgt, thr, kw["refine_steps"], es, np.float32)
        assert np.array_equal(got["mask"], cmask) and np.array_equal(got["num_inliers"], cnum)
        assert np.abs(got["R"] - R).max() <= bar_R and np.abs(got["T"] - T).max() <= bar_T
        assert (np.abs(got["s"] - s) <= 1e-5 * s).all()
        return accepted
    return None


def _scene_run(dev, name):
    if name not in _RUNS:
        sc, kw = ref.make_scene(name)
        _RUNS[name] = (sc, kw, _call(dev, sc["X"], sc["Y"], sc["corr"], sc["len1"], sc["len2"], **kw))
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("name", list(ref.SCENES))
def test_scene_in_stages(dev, name):
    sc, kw, got = _scene_run(dev, name)
    planted = ref.SCENES[name].get("planted", True)
    check_stages(got, sc["X"], sc["Y"], sc["corr"], sc["len1"], sc["len2"], kw, chain=planted)
    if not planted:
        return
    # 6
    assert np.array_equal(got["mask"], sc["planted"])
    assert np.array_equal(got["num_inliers"], sc["planted"].sum(1))
    if kw["refine_steps"] > 0:  # the final transform is the float64 weighted alignment of the device's (final) mask
        tgt = ref.targets(sc["corr"], ref.lengths_of(sc["len1"], *sc["X"].shape[:2]),
                          ref.lengths_of(sc["len2"], sc["X"].shape[0], sc["Y"].shape[1]), *sc["X"].shape[:2])
        R, T, s, _ = ref.fit_mask(sc["X"], sc["Y"], tgt, got["mask"], kw["estimate_scale"])
        bar_R, bar_T = _bars(sc["Y"])
        assert np.abs(got["R"] - R).max() <= bar_R and np.abs(got["T"] - T).max() <= bar_T
        assert (np.abs(got["s"] - s) <= 1e-5 * s).all()
    # the motion: a least-squares fit is no further from the noisy targets than the planted motion is, so its rms
    # distance from the planted motion over the planted rows is at most twice the noise (0.2 thr); the unrefined winner
    # holds every planted row within thr of its noisy target
    for n in range(len(sc["X"])):
        x = sc["X"][n, sc["planted"][n]].astype(np.float64)
        fit = got["s"][n].astype(np.float64) * (x @ got["R"][n].astype(np.float64)) + got["T"][n]
        truth = sc["scale"] * (x @ sc["R0"][n]) + sc["T0"][n]
        d = np.linalg.norm(fit - truth, axis=1)
        if kw["refine_steps"] > 0:
            assert np.sqrt((d * d).mean()) <= 0.4 * kw["thr"] + 1e-5
        else:
            assert d.max() <= 1.2 * kw["thr"] + 1e-5


def test_small_clouds_beside_a_normal_one(dev):
    """M = 0, 1, 2, 3, 5 valid pairs, a zero-length cloud and a normal cloud in one batch; two rows share a target."""
    sc = ref.scene(21, 64, 0.6, N=7)
    X, Y, corr = sc["X"], sc["Y"], sc["corr"].copy()
    len1 = np.full(7, 64, np.int64)
    for n, M in enumerate((0, 1, 2, 3, 5)):
        keep = np.nonzero(sc["planted"][n])[0][:M]
        row = np.full(64, -1, np.int64)
        row[keep] = corr[n, keep]
        corr[n] = row
    len1[5] = 0
    corr[6, 1] = corr[6, 0]  # a shared target
    kw = dict(thr=ref.THR, H=64, estimate_scale=False, ratio=0.9, refine_steps=2, seed=5)
    got = _call(dev, X, Y, corr, len1, None, **kw)
    check_stages(got, X, Y, corr, len1, None, kw, chain=True)
    assert got["best"][[0, 1, 2, 5]].tolist() == [-1] * 4 and (got["samples"][[0, 1, 2, 5]] == -1).all()
    assert got["best"][3] >= 0 and got["num_inliers"][3] == 3 and got["num_inliers"][4] == 5
    assert got["best"][6] >= 0 and got["num_inliers"][6] >= 20


@pytest.mark.parametrize("es", [False, True], ids=["rigid", "scale"])
def test_given_samples(dev, es):
    """The caller's triples: an invalid row, a duplicated row and an all-invalid cloud give counts of -1 and the
    identity; nothing is drawn."""
    sc = ref.scene(22, 100, 0.5, N=2, scale=1.3 if es else 1.0)
    X, Y, corr = sc["X"], sc["Y"], sc["corr"]
    p = np.nonzero(sc["planted"][0])[0]
    bad = int(np.nonzero(corr[0] < 0)[0][0])
    samples = np.array([[[p[0], p[1], p[2]], [p[3], bad, p[4]], [p[5], p[5], p[6]], [p[7], p[8], 100], [p[2], p[1], p[0]]],
                        [[bad, bad, bad]] * 5], np.int64)
    samples[1, :, :] = np.nonzero(corr[1] < 0)[0][0]
    kw = dict(thr=ref.THR, estimate_scale=es, ratio=0.9, refine_steps=1, seed=0)
    got = _call(dev, X, Y, corr, samples=samples, **kw)
    check_stages(got, X, Y, corr, None, None, kw, given_samples=samples)
    assert (got["counts"][0] >= 0).tolist() == [True, False, False, False, True]
    assert (got["counts"][1] == -1).all() and got["best"].tolist() == [0, -1]
    assert not got["mask"][1].any() and got["num_inliers"][1] == 0 and got["num_inliers"][0] >= 3


def test_hand_case_is_exact(dev):
    """tests/test_ransac_cpu.py::test_hand_case_translation on the device: exact T, counts by hand on both sides of
    the threshold."""
    T = np.array([0.5, -0.25, 2.0], np.float32)
    X = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0]]] * 3, np.float32)
    Y = X + T
    for n, offset in enumerate((0.25, 0.25 - 2.0 ** -20, 0.25 + 2.0 ** -20)):
        Y[n, 3, 0] = np.float32(0.5 + offset)
    Y[:, 4] = 5.0
    samples = np.array([[[0, 1, 2], [2, 2, 1], [0, 1, 7], [0, 1, 4]]] * 3, np.int64)
    got = _call(dev, X, Y, thr=0.25, samples=samples, ratio=0.0, refine_steps=0)
    assert np.array_equal(got["hyp_T"][:, 0], np.stack([T] * 3)) and (got["hyp_s"][:, 0] == 1).all()
    assert np.abs(got["hyp_R"][:, 0] - np.eye(3)).max() < 1e-7
    assert got["counts"][:, 0].tolist() == [4, 4, 3] and (got["counts"][:, 1:3] == -1).all()
    assert got["best"].tolist() == [0, 0, 0] and got["num_inliers"].tolist() == [4, 4, 3]
    assert got["mask"].tolist() == [[True, True, True, True, False]] * 2 + [[True, True, True, False, False]]
    edge = _call(dev, X, Y, thr=0.25, samples=samples, ratio=0.9, refine_steps=0)
    assert (edge["counts"][:, 3] == -1).all() and edge["best"].tolist() == [0, 0, 0]


def test_rejected_refinement_keeps_the_winner(dev):
    X, Y, samples, thr = ref.rejected_refit_scene()
    kw = dict(thr=thr, estimate_scale=False, ratio=0.0, refine_steps=3, seed=0)
    got = _call(dev, X, Y, samples=samples, **kw)
    accepted = check_stages(got, X, Y, None, None, None, kw, given_samples=samples, chain=True)
    assert accepted.tolist() == [0] and got["num_inliers"].tolist() == [9]
    assert np.array_equal(got["R"], got["hyp_R"][:, 0]) and np.array_equal(got["T"], got["hyp_T"][:, 0])
    free = _call(dev, X, Y, samples=samples, **dict(kw, refine_steps=0))
    for k in ("R", "T", "s", "mask", "num_inliers", "rmse"):
        assert np.array_equal(got[k], free[k]), k


def test_empty_batch_and_empty_clouds(dev):
    """N == 0 launches nothing; P1 == 0 (or no target rows) is the identity result, fully written."""
    for N, P1, P2 in ((0, 5, 5), (2, 0, 0), (2, 0, 7), (2, 6, 0)):
        X, Y = np.ones((N, P1, 3), np.float32), np.ones((N, P2, 3), np.float32)
        corr = np.zeros((N, P1), np.int64)
        got = _call(dev, X, Y, corr, H=5, refine_steps=1)
        assert got["mask"].shape == (N, P1) and got["counts"].shape == (N, 5) and got["samples"].shape == (N, 5, 3)
        assert not got["mask"].any() and (got["best"] == -1).all() and (got["counts"] == -1).all()
        assert (got["samples"] == -1).all() and not got["num_inliers"].any() and not got["rmse"].any()
        assert np.array_equal(got["R"], np.broadcast_to(np.eye(3, dtype=np.float32), (N, 3, 3)))
        assert not got["T"].any() and (got["s"] == 1).all() and (got["hyp_s"] == 1).all() and not got["hyp_T"].any()


def test_corr_none_is_the_identity_table(dev):
    sc = ref.scene(23, 300, 0.5, P2=300)
    X = sc["X"]
    Y = np.zeros_like(sc["Y"])  # row i of Y: the target of row i of X (a far point for the rows without a match)
    ok = (sc["corr"][0] >= 0) & (sc["corr"][0] < 300)
    Y[0, ok] = sc["Y"][0, sc["corr"][0, ok]]
    Y[0, ~ok] = 9.0
    table = np.arange(300, dtype=np.int64)[None]
    kw = dict(thr=ref.THR, H=256, seed=3)
    a, b = _call(dev, X, Y, None, **kw), _call(dev, X, Y, table, **kw)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["num_inliers"][0] == sc["planted"].sum()


def test_public_function_and_pointclouds(dev):
    """The public wrapper: a namedtuple of tensors that never require grad, None without return_hypotheses, lengths
    from Pointclouds equal to the padded call through the boundary."""
    from pytorch3d_pointops_amd.structures import Pointclouds

    f = _api()
    sc, kw, got = _scene_run(dev, "p1000")
    X, Y, corr = _t(sc["X"], dev).requires_grad_(True), _t(sc["Y"], dev), _t(sc["corr"], dev)
    pcx = Pointclouds([X[n, :int(sc["len1"][n])].detach() for n in range(3)])
    pcy = Pointclouds([Y[n, :int(sc["len2"][n])] for n in range(3)])
    P1 = int(sc["len1"].max())
    sol = f.ransac_alignment(pcx, pcy, corr[:, :P1], inlier_threshold=kw["thr"], num_hypotheses=kw["H"],
                             seed=kw["seed"], return_hypotheses=True)
    assert isinstance(sol, f.RansacSolution) and isinstance(sol.RTs, f.SimilarityTransform)
    assert sol.inliers.dtype == torch.bool and sol.num_inliers.dtype == torch.int64 and sol.best.dtype == torch.int64
    assert sol.counts.dtype == torch.int32 and sol.samples.dtype == torch.int64
    assert np.array_equal(_np(sol.inliers), got["mask"][:, :P1]) and np.array_equal(_np(sol.RTs.R), got["R"])
    assert np.array_equal(_np(sol.best), got["best"]) and np.array_equal(_np(sol.samples), got["samples"])
    plain = f.ransac_alignment(X[:1], Y[:1], corr[:1], inlier_threshold=kw["thr"], num_hypotheses=64)
    assert plain.counts is None and plain.hypotheses is None and plain.samples is None
    assert not any(t.requires_grad for t in (*plain.RTs, plain.inliers, plain.num_inliers, plain.rmse, plain.best))


# ------------------------------------------------------------------------------------------------ determinism, streams
def _tensors(dev, sc):
    return _t(sc["X"], dev), _t(sc["Y"], dev), _t(sc["corr"], dev)


def _solve(f, X, Y, corr, kw):
    r = f.ransac_alignment(X, Y, corr, inlier_threshold=kw["thr"], num_hypotheses=kw["H"], seed=kw["seed"],
                           estimate_scale=kw["estimate_scale"], edge_length_ratio=kw["ratio"],
                           refine_steps=kw["refine_steps"], return_hypotheses=True)
    return (*r.RTs, r.inliers, r.num_inliers, r.rmse, r.best, r.counts, *r.hypotheses, r.samples)


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def test_two_runs_are_bit_equal_and_a_side_stream_too(dev):
    sc, kw = ref.make_scene("2chunk+1")
    X, Y, corr = _tensors(dev, sc)
    first = _solve(_api(), X, Y, corr, kw)
    assert _same(first, _solve(_api(), X, Y, corr, kw))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = _solve(_api(), X, Y, corr, kw)
    side.synchronize()
    assert _same(first, other)


@pytest.mark.parametrize("name", ["chunk-1", "2chunk+1", "h65"])
def test_lds_tile_scoring_changes_nothing(dev, monkeypatch, name):
    """POINTOPS_DEBUG=ransac_lds=1 sends the records through an LDS tile instead of the scalar path: every output is
    bit-equal."""
    sc, kw, want = _scene_run(dev, name)
    monkeypatch.setenv("POINTOPS_DEBUG", "ransac_lds=1")
    got = _call(dev, sc["X"], sc["Y"], sc["corr"], sc["len1"], sc["len2"], **kw)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_graph_capture_replays_the_eager_result(dev):
    from pytorch3d_pointops_amd import graphs

    sc, kw = ref.make_scene("chunk+1")
    X, Y, corr = _tensors(dev, sc)
    want = _solve(_api(), X, Y, corr, kw)
    x, y = X.clone(), Y.clone()
    step = graphs.capture(lambda a, b: _solve(_api(), a, b, corr, kw), (x, y))
    assert _same(step(), want)
    sc2 = ref.scene(31, sc["X"].shape[1], 0.5)  # other points through the static inputs, the same table
    X2, Y2 = _t(sc2["X"], dev), _t(sc2["Y"], dev)
    assert _same(step(X2, Y2), _solve(_api(), X2, Y2, corr, kw))


# ------------------------------------------------------------------------------------------------ buffer contract
_BASELINE = {}


def _under_contract(monkeypatch, dev, fill):
    sc, kw = ref.make_scene("p257")
    sib = ref.scene(32, 257, 0.5)
    args = _tensors(dev, sc)
    sargs = _tensors(dev, sib)
    short = "short" if fill == "ones" else False
    with buffers.contract(monkeypatch, fill, short_workspace=short, prototypes=PROTOS) as c:
        c.sibling(lambda: _solve(_api(), *sargs, kw))
        c.watch(X=args[0], Y=args[1], corr=args[2])
        out = _solve(_api(), *args, kw)
    c.assert_all_clear()
    assert [b.kind for b in c.buffers] == ["out"] * 12 + ["workspace"] and c.inputs_checked >= 3
    if short:
        assert {(n, how) for n, _, how in c.rejections} == {("pointops_ransac_alignment", "short"),
                                                            ("pointops_ransac_alignment", "null")}
    _, _, got = _scene_run(dev, "p257")
    assert np.array_equal(_np(out[3]), got["mask"]) and np.array_equal(_np(out[7]), got["counts"])
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
    from pytorch3d_pointops_amd import _C, _C_ransac

    X = torch.rand(1, 8, 3, device=dev)
    with pytest.raises(RuntimeError, match="ransac_alignment"):
        _C_ransac.ransac_alignment(X, X[:, :7], None, None, None, None, 4, 0, 0.1, 0.9, False, 1)
    outs = [torch.full((64,), 7, dtype=torch.uint8, device=dev) for _ in range(7)]
    ws = torch.zeros(_C._lib.pointops_ransac_workspace_bytes(1, 8, 4), dtype=torch.uint8, device=dev)
    for bad in (dict(H=0), dict(thr=-1.0), dict(ratio=2.0), dict(refine=-1), dict(P2=7)):
        a = dict(H=4, thr=0.1, ratio=0.9, refine=1, P2=8)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.ransac_alignment("ransac_alignment", dev, X, X, None, None, None, None, 1, 8, a["P2"], a["H"], 0, 0,
                                      a["thr"], a["ratio"], 0, a["refine"], *outs, None, None, None, None, None, ws,
                                      ws.numel())
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ big batch
def test_batch_of_65537_clouds_draws_by_the_global_index(dev):
    """One batch over the entry's limit goes in slices; clouds 0, 65 534, 65 535 and 65 536 equal the checker run on
    each alone with its index in the batch as first_cloud."""
    N, P1, H = 65537, 4, 64
    rng = np.random.default_rng(9400)
    X = rng.uniform(0, 1, (N, P1, 3)).astype(np.float32)
    Y = (X + np.float32(0.25)).astype(np.float32)
    Y[:, 3] += np.float32(5.0)  # one wrong match per cloud, too far for any triangle through it to pass the edge test
    kw = dict(thr=ref.THR, H=H, estimate_scale=False, ratio=0.9, refine_steps=1, seed=77)
    got = _call(dev, X, Y, **kw)
    for n in (0, 65534, 65535, 65536):
        one = {k: v[n:n + 1] for k, v in got.items()}
        check_stages(one, X[n:n + 1], Y[n:n + 1], None, None, None, kw, first_cloud=n)
        assert one["num_inliers"][0] == 3 and one["mask"][0].tolist() == [True, True, True, False]
    assert (got["num_inliers"] == 3).all() and (got["best"] >= 0).all()
    assert not np.array_equal(got["samples"][0], got["samples"][65535])  # (a restart at 0 would repeat cloud 0's draws)


# ------------------------------------------------------------------------------------------------ end to end
def test_registration_from_fpfh_matches_with_outliers(dev):
    """fpfh_ref.cloud("heightfield") moved and permuted, 70 % of the mutual matches overwritten by random rows:
    ransac_alignment then iterative_closest_point recovers the motion to ICP's bars on a moved copy (converged, 1e-5
    on R, 1e-5 (1 + max|Y|) on T: tests/test_points_alignment_gpu.py); corresponding_points_alignment on all the matches
    is printed for comparison."""
    import fpfh_ref

    f = _api()
    rng = np.random.default_rng(9500)
    pts, nrm = fpfh_ref.cloud("heightfield", 1, 700)
    mp, mn = fpfh_ref.moved(pts, nrm)
    perm = rng.permutation(700)
    X, Xn, Y, Yn = _t(pts, dev), _t(nrm, dev), _t(mp[:, perm], dev), _t(mn[:, perm], dev)
    match = f.mutual_nearest_neighbors(f.fpfh_features(X, Xn, K=16), f.fpfh_features(Y, Yn, K=16)).cpu().numpy()
    found = np.nonzero(match[0] >= 0)[0]
    spoiled = found[rng.permutation(len(found))[:int(0.7 * len(found))]]
    match[0, spoiled] = rng.integers(0, 700, len(spoiled))
    corr = _t(match, dev)
    R0, t0 = fpfh_ref.rigid_motion()  # y = R0 x + t0: row vectors x R0^T + t0
    sol = f.ransac_alignment(X, Y, corr, inlier_threshold=0.02, num_hypotheses=4096, seed=1)
    icp = f.iterative_closest_point(X, Y, init_transform=sol.RTs, max_iterations=50)
    R, T = icp.RTs.R[0].cpu().numpy().astype(np.float64), icp.RTs.T[0].cpu().numpy().astype(np.float64)
    Yg = torch.gather(Y, 1, corr.clamp(min=0)[..., None].expand(-1, -1, 3))
    w = (corr >= 0).float()
    ls = f.corresponding_points_alignment(X, Yg, weights=w)
    print("inliers kept by RANSAC:", int(sol.num_inliers[0]), "of", len(found), "matches;",
          "least squares on all matches lands |dR| =", float(np.abs(ls.R[0].cpu().numpy() - R0.T).max()),
          "RANSAC", float(np.abs(sol.RTs.R[0].cpu().numpy() - R0.T).max()), "RANSAC + ICP", float(np.abs(R - R0.T).max()))
    assert icp.converged is True
    assert np.abs(R - R0.T).max() <= 1e-5 and np.abs(T - t0).max() <= 1e-5 * (1.0 + float(np.abs(mp).max()))


def test_zz_report_rmse(dev):
    """Not a check of its own: prints the largest rmse error the tests above saw against its bound."""
    print(f"largest |rmse - float64 rmse| on the device: {_RMSE_WORST[0]:.3e} (bound {_RMSE_WORST[1]:.3e})")
    assert _RMSE_WORST[0] <= _RMSE_WORST[1] or _RMSE_WORST[1] == 0.0
