"""Every C ABI entry held to the buffer contract of include/pointops_amd.h under poisoned memory (tests/buffers.py).

One pass per operator path, untransformed, under each fill -- zero (the lucky state the rest of the suite mostly sees),
ones (0xFF: NaN / -1) and stale (what a sibling call of the same shapes, other points and full lengths left behind) --
with every output and workspace between two 64 KiB guards.  Per path and fill:
  * the results equal the reference the path's own test uses, through that test's comparison (bit-equal idx / dists and
    deterministic gradients against the oracle, 1e-5 for atomically accumulated ones, the float64 checkers of
    chamfer_ref.py, points_alignment_ref.py and test_points_normals_gpu.py) -- over EVERY element, padding included;
  * without atomics, the bytes of every output under ones and stale equal those under zero;
  * the path is asserted from the grid statistics where test_coordinate_frames_gpu.py asserts it;
  * all guards are intact, all tensors behind `const` parameters are bit-unchanged (idx, lengths and the self-query's
    shared tensor included);
  * under ones, every entry with a workspace is first called with `workspace_bytes - 1` and with a null workspace:
    POINTOPS_EWORKSPACE and untouched outputs -- ball_query instead falls back to the scan, as its header says, and
    must still match the oracle.
The knobs, versions and bases are those of test_coordinate_frames_gpu.py (the first base of each path, every base of
the long-list, wide and FPS paths).  Every search base gets three more clouds whose lengths are the edges (no queries; no
targets; fewer than K targets behind a ragged number of queries), every FPS base an empty cloud and one shorter than
its K, so that each kernel family meets rows and slots that are padding only -- the sibling's full lengths put live
data there.  The opt-in grid cache stays off; HIP-graph capture is out of scope."""
import types

import numpy as np
import pytest
import torch

import buffers
import cases
import test_chamfer_float64_gpu as chamfer
import test_coordinate_frames_gpu as fr
import test_gpu_parity as parity
import test_points_alignment_gpu as align
import test_points_normals_gpu as normals
from conftest import bits, load_golden
from test_boundary_cpu import declared_prototypes
from test_gpu_parity import G, close

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
_WANT = {}      # references, computed once per path
_BASELINE = {}  # output bytes under the zero fill, per path


def _contract(monkeypatch, fill, short=None):
    from pytorch3d_pointops_amd import _C

    assert not _C.grid_cache_enabled()
    if short is None:
        short = "short" if fill == "ones" else False
    return buffers.contract(monkeypatch, fill, short_workspace=short, prototypes=PROTOS)


def _held(monkeypatch, fill, key, real, sibling, atomic=False, entries=(), short=None):
    """Run `real()` (which asserts its own results) under the contract, after `sibling()` under the stale fill; then the
    guards, the inputs, the buffer sequence, the short-workspace rejections of `entries` and the bytes across fills."""
    with _contract(monkeypatch, fill, short) as c:
        c.sibling(sibling)
        real()
    c.assert_all_clear()
    if fill == "ones" or short:
        rejected = {name for name, _, _ in c.rejections}
        assert set(entries) <= rejected, (key, sorted(set(entries) - rejected))
    got = c.output_bytes()
    if fill == "zero" and not short:
        _BASELINE[key] = got
    elif not atomic:
        if key not in _BASELINE:
            _held(monkeypatch, "zero", key, real, sibling, atomic, entries)
        want = _BASELINE[key]
        assert [n for n, _ in got] == [n for n, _ in want], key
        for (name, a), (_, b) in zip(got, want):
            assert np.array_equal(a, b), (key, fill, name, "differs from the zero fill at byte",
                                          int(np.flatnonzero(a != b)[0]))
    return c


def _want(key, fn):
    if key not in _WANT:
        _WANT[key] = fn()
    return _WANT[key]


def _other(shape, seed):
    return cases.cloud(91000 + seed, shape)


FILLS = pytest.mark.parametrize("fill", buffers.FILLS)


# ------------------------------------------------------------------------------------------------ knn_points_idx
_UNTRANSFORMED = types.SimpleNamespace(name="untransformed")  # (the frame argument of the imported path assertions)
_STAT_CHECKS = {"box_search": fr._boxed, "refined_cells": fr._refined, "wave_sort": fr._wave_sorted}  # others: _grid_used


def _with_edge_clouds(b):
    """The base plus three clouds (copies of cloud 0's points, so shapes per cloud, knobs and the statistics of the
    base's own clouds stay as they are) whose lengths are the edges the header speaks of: a cloud without queries
    (every row padding), a cloud without targets (every slot padding) and one with fewer than K targets behind a ragged
    number of queries.  A self-query with one lengths vector gets lengths 0, K - 1 and P / 2 + 1."""
    P1, P2, K = b["p1"].shape[1], b["p2"].shape[1], b["K"]
    same = b["p2"] is b["p1"]
    p1 = np.concatenate([b["p1"]] + [b["p1"][:1]] * 3)
    p2 = p1 if same else np.concatenate([b["p2"]] + [b["p2"][:1]] * 3)
    few = max(K - 1, 0)
    if same and b["l2"] is b["l1"]:
        l1 = l2 = np.concatenate([b["l1"], [0, few, P1 // 2 + 1]]).astype(np.int64)
    else:
        l1 = np.concatenate([b["l1"], [0, min(P1, 7), P1 // 2 + 1]]).astype(np.int64)
        l2 = np.concatenate([b["l2"], [P2, 0, min(few, P2)]]).astype(np.int64)
    assert (l1 == 0).any() and (l2 == 0).any() and (l2 < K).any() and ((l1 > 0) & (l1 < P1)).any()
    return dict(b, p1=p1, p2=p2, l1=l1, l2=l2)


_KNN = {  # path: (table, knob, version, statistics)
    "brute_v0": (fr._BRUTE, "knn_small=0", 0, False), "scan_v2": (fr._BRUTE, "knn_small=0", 2, False),
    "grid_quad": (fr._GRID, "grid_quad=1", 3, True), "grid_lane": (fr._GRID, "grid_quad=0", 3, True),
    "grid_self": (fr._GRID, "", 3, True),
    "box_search": (fr._LONG, "grid_long_box=1", 3, True), "refined_cells": (fr._LONG, "", 3, True),
    "wave_sort": (fr._LONG, "", 3, True),
    "knn_small_q1": (fr._SMALLP, "knn_small=1,knn_small_q=1", 2, False),
    "knn_small_q2": (fr._SMALLP, "knn_small=1,knn_small_q=2", 2, False),
    "knn_wide": (fr._WIDEP, "", -1, False),
}
_EVERY_BASE = ("box_search", "refined_cells", "wave_sort", "knn_wide")
_KNN_PARAMS = [(path, name) for path, (table, _, _, _) in _KNN.items()
               for name in (table[path][1] if path in _EVERY_BASE else table[path][1][:1])]


def _knn_sibling_base(b, seed):
    """The same shapes, K and norm; other points; full lengths; a self-query stays one (the same objects twice)."""
    p1 = _other(b["p1"].shape, seed)
    same = b["p2"] is b["p1"]
    l1 = np.full(b["l1"].shape, p1.shape[1], np.int64)
    p2 = p1 if same else _other(b["p2"].shape, seed + 1)
    l2 = l1 if (same and b["l2"] is b["l1"]) else np.full(b["l2"].shape, p2.shape[1], np.int64)
    return dict(b, p1=p1, p2=p2, l1=l1, l2=l2)


@FILLS
@pytest.mark.parametrize("path,name", _KNN_PARAMS, ids=[f"{p}-{n}" for p, n in _KNN_PARAMS])
def test_knn_points_idx(dev, oracle, monkeypatch, path, name, fill):
    from pytorch3d_pointops_amd import _C

    table, knob, version, stats = _KNN[path]
    b = _want(("knn base", path, name), lambda: _with_edge_clouds(table[path][0](name)))
    what = (path, name, fill)
    wi, wd = _want(("knn", path, name), lambda: fr._knn_want(dev, oracle, b, b["p1"], b["p2"], fr._ORACLE_BASE_PAIRS))
    sb = _knn_sibling_base(b, len(name))

    def run(base, check):
        fr._env(monkeypatch, knob)
        i, d, st = fr._knn_gpu(dev, base, base["p1"], base["p2"], version, "stats" if stats else None)
        fr._env(monkeypatch, "")
        if check:
            if stats:  # (the path, from the statistics of the base's own, non-empty clouds)
                _STAT_CHECKS.get(path, fr._grid_used)(st, what, _UNTRANSFORMED, base)
            assert np.array_equal(i, wi), what  # (every element: padded rows and slots are the oracle's 0 / 0.0)
            assert np.array_equal(bits(d), bits(wd)), what

    ws = _C._lib.pointops_knn_workspace_bytes(*b["p1"].shape[:2], b["p2"].shape[1], b["p1"].shape[2], b["K"], version)
    entry = "pointops_knn_points_idx" if stats else "pointops_knn_points_idx_reuse"
    _held(monkeypatch, fill, ("knn", path, name), lambda: run(b, True), lambda: run(sb, False),
          entries=[entry] if ws else [])


# ------------------------------------------------------------------------------------------------ ball_query
_BALL_PARAMS = [(path, names[0]) for path, (_, names) in fr._BALL.items()]


def _ball(dev, oracle, monkeypatch, path, name, fill, short=None):
    from pytorch3d_pointops_amd import _C

    b = _want(("ball base", name), lambda: _with_edge_clouds(fr._ball_base(name)))
    what = (path, name, fill, short)
    wi, wd = _want(("ball", name), lambda: oracle.ball_query(b["p1"], b["p2"], b["l1"], b["l2"], b["K"], b["radius"]))
    sb = _knn_sibling_base(b, 50 + len(name))

    def run(base, check):
        fr._env(monkeypatch, fr._BALL_KNOBS[path])
        i, d = _C.ball_query(G(base["p1"], dev), G(base["p2"], dev), G(base["l1"], dev), G(base["l2"], dev), b["K"],
                             b["radius"])
        fr._env(monkeypatch, "")
        if check:
            i, d = i.cpu().numpy(), d.cpu().numpy()
            assert np.array_equal(i, wi), what  # (padding: -1 and 0.0, the oracle's)
            assert np.array_equal(bits(d), bits(wd)), what

    _held(monkeypatch, fill, ("ball", path, name), lambda: run(b, True), lambda: run(sb, False),
          entries=["pointops_ball_query"] if short else [], short=short or False)


@FILLS
@pytest.mark.parametrize("path,name", _BALL_PARAMS, ids=[f"{p}-{n}" for p, n in _BALL_PARAMS])
def test_ball_query(dev, oracle, monkeypatch, path, name, fill):
    _ball(dev, oracle, monkeypatch, path, name, fill)


@pytest.mark.parametrize("short", ["short", "null"])
@pytest.mark.parametrize("path,name", [p for p in _BALL_PARAMS if p[0].startswith("ball_grid")][:2])
def test_ball_query_without_its_workspace_scans(dev, oracle, monkeypatch, path, name, short):
    """A short or null workspace is no error for ball_query ("Without workspace every cloud is scanned"): the call
    itself is made that way, matches the oracle and the zero-fill bytes, and leaves the guards intact."""
    _ball(dev, oracle, monkeypatch, path, name, "ones", short)


# ------------------------------------------------------------------------------------------------ FPS
_FPS_PARAMS = [(path, name) for path, (_, names) in fr._FPS.items() for name in names]


@FILLS
@pytest.mark.parametrize("path,name", _FPS_PARAMS, ids=[f"{p}-{n}" for p, n in _FPS_PARAMS])
def test_sample_farthest_points(dev, oracle, monkeypatch, path, name, fill):
    from pytorch3d_pointops_amd import _C

    b = fr._fps_base(name)  # ... plus an empty cloud (lengths 0: a row of -1) and one shorter than its K
    b = dict(p1=np.concatenate([b["p1"]] + [b["p1"][:1]] * 2), lengths=np.concatenate([b["lengths"], [0, 3]]),
             K=np.concatenate([b["K"], [int(b["K"].max()), 9]]), start=np.concatenate([b["start"], [0, 2]]))
    N, P, _ = b["p1"].shape
    assert (P <= 4096) == (path != "fps_multi_workgroup")
    want = _want(("fps", name), lambda: oracle.sample_farthest_points(b["p1"], b["lengths"], b["K"], b["start"]))
    sib = dict(p1=_other(b["p1"].shape, 70 + len(name)), lengths=np.full((N,), P, np.int64), K=b["K"], start=b["start"])

    def run(base, check):
        fr._env(monkeypatch, "fps_small=0" if path == "fps_clusters" else "")
        # (max_K is passed: the sibling's full lengths must not change the output's shape)
        r = _C.sample_farthest_points(G(base["p1"], dev), G(base["lengths"], dev), G(base["K"], dev),
                                      G(base["start"], dev), max_K=int(b["K"].max()))
        fr._env(monkeypatch, "")
        if check:
            assert np.array_equal(r.cpu().numpy(), want), (path, name, fill)  # (-1 beyond min(lengths, K): the oracle's)

    _held(monkeypatch, fill, ("fps", path, name), lambda: run(b, True), lambda: run(sib, False),
          entries=["pointops_sample_farthest_points"])


# ------------------------------------------------------------------------------------------------ knn backward
_BWD_PARAMS = [(path, names[0]) for path, (_, names) in fr._BWD.items()]
_BWD_KNOBS = {"bwd_deterministic": "", "bwd_tiled": "knn_bwd_mode=tiled", "bwd_tiled_split3": "knn_bwd_mode=tiled,knn_bwd_split=3",
              "bwd_atomic": "knn_bwd_mode=atomic"}


@FILLS
@pytest.mark.parametrize("path,name", _BWD_PARAMS, ids=[f"{p}-{n}" for p, n in _BWD_PARAMS])
def test_knn_points_backward(dev, oracle, monkeypatch, path, name, fill):
    from pytorch3d_pointops_amd import _C

    b = fr._bwd_base(name)
    det = path == "bwd_deterministic"
    grad = cases.grad_for(name, (b["p1"].shape[0], b["p1"].shape[1], b["K"]))
    what = (path, name, fill)
    sb = _knn_sibling_base(b, 30 + len(name))

    def run(base, check):
        args = (G(base["p1"], dev), G(base["p2"], dev), G(base["l1"], dev), G(base["l2"], dev))
        idx, _ = _C.knn_points_idx(*args, b["norm"], b["K"], -1)
        fr._env(monkeypatch, _BWD_KNOBS[path])
        g1, g2 = _C.knn_points_backward(*args, idx, b["norm"], G(grad, dev), deterministic=det)
        fr._env(monkeypatch, "")
        if check:
            idx = idx.cpu().numpy()
            o1, o2 = _want(("bwd", path, name), lambda: oracle.knn_points_backward(
                base["p1"], base["p2"], base["l1"], base["l2"], idx, b["norm"], grad))
            g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
            assert np.array_equal(bits(g1), bits(o1)), what
            assert np.array_equal(bits(g2), bits(o2)) if det else fr._close_rel(g2, o2), what

    _held(monkeypatch, fill, ("bwd", path, name), lambda: run(b, True), lambda: run(sb, False), atomic=not det,
          entries=["pointops_knn_points_backward_det"] if det else [])


# ------------------------------------------------------------------------------------------------ gather
@FILLS
@pytest.mark.parametrize("U", [1, 3, 4])
def test_gather_neighbors(dev, monkeypatch, U, fill):
    """The shapes, generators and references of test_knn_gather_widths (K = 6): with lengths [K, 2, 0] and with -1 rows."""
    from oracle import oracle as O
    from pytorch3d_pointops_amd import _C, synth

    N, M, L, K = 3, 500, 333, 6
    x = cases.cloud(1900 + U, (N, M, U))
    idx = synth.randint(1901, 0, M - 1, (N, L, K))
    lengths = np.array([K, 2, 0])
    idx2 = idx.copy()
    idx2[:, ::5, 2] = -1

    def run(x, idx, idx2, lengths, check):
        out = _C.gather_neighbors(G(x, dev), G(idx, dev), G(lengths, dev))
        out2 = _C.gather_neighbors(G(x, dev), G(idx2, dev), None)
        if check:
            assert np.array_equal(bits(out.cpu().numpy()), bits(O.knn_gather(x, idx, lengths))), (U, fill)
            assert np.array_equal(bits(out2.cpu().numpy()), bits(O.masked_gather(x, idx2))), (U, fill)

    _held(monkeypatch, fill, ("gather", U), lambda: run(x, idx, idx2, lengths, True),
          lambda: run(_other(x.shape, U), synth.randint(1951, 0, M - 1, (N, L, K)),
                      synth.randint(1952, 0, M - 1, (N, L, K)), np.full((N,), K), False))


@FILLS
@pytest.mark.parametrize("mode", ["tiled", "tiled_split2", "atomic", "deterministic"])
@pytest.mark.parametrize("U", [1, 3, 4])
def test_gather_neighbors_backward(dev, monkeypatch, mode, U, fill):
    """The shapes, generators and float64 np.add.at reference of test_gather_backward_modes, at its 1e-5 (`close`);
    the deterministic form (table order: the same sum) within the same bar and bit-equal across fills."""
    from pytorch3d_pointops_amd import _C, synth

    knob = {"tiled": "gather_bwd_mode=tiled", "tiled_split2": "gather_bwd_mode=tiled,gather_bwd_split=2",
            "atomic": "gather_bwd_mode=atomic", "deterministic": ""}[mode]
    det = mode == "deterministic"
    N, L, K, M = 2, 3000, 8, 20000
    idx = synth.randint(1601, -1, M - 1, (N, L, K))
    idx[0, ::7, :] = 3
    go = cases.grad_for("gbm%d" % U, (N, L, K, U))
    go[1, 5::11] = 0.0
    lengths = np.array([8, 5])

    def want():
        ref = np.zeros((N, M, U), np.float64)
        for n in range(N):
            kk = int(lengths[n])
            ii = idx[n, :, :kk].reshape(-1)
            vv = go[n, :, :kk].reshape(-1, U).astype(np.float64)
            np.add.at(ref[n], ii[ii >= 0], vv[ii >= 0])
        return ref

    def run(go, idx, lengths, check):
        fr._env(monkeypatch, knob)
        gx = _C.gather_neighbors_backward(G(go, dev), G(idx, dev), G(lengths, dev), M, deterministic=det)
        fr._env(monkeypatch, "")
        if check:
            assert close(gx.cpu().numpy(), _want(("gbwd", U), want)), (mode, U, fill)

    _held(monkeypatch, fill, ("gather_bwd", mode, U), lambda: run(go, idx, lengths, True),
          lambda: run(cases.grad_for("sib%d" % U, go.shape), synth.randint(1661, 0, M - 1, (N, L, K)), np.array([8, 8]),
                      False), atomic=not det, entries=["pointops_gather_neighbors_backward_det"] if det else [])


# ------------------------------------------------------------------------------------------------ packed <-> padded
def _packed_case(name):
    if name != "unowned_rows":
        c = cases.packed_cases()[name]
        x, first, F = cases.packed_inputs(c)
        return x, first, F, int(c["max_size"])
    # rows 0 and 1 precede the first cloud: packed rows owned by no cloud, which must come back zero (and an empty cloud)
    return cases.cloud(405, (20, 3)) + np.float32(1.0), np.array([2, 7, 14, 14], np.int64), 20, 7


@FILLS
@pytest.mark.parametrize("name", sorted(cases.packed_cases()) + ["unowned_rows"])
def test_packed_padded(dev, oracle, monkeypatch, name, fill):
    from pytorch3d_pointops_amd import _C

    x, first, F, max_size = _packed_case(name)
    padded = _want(("p2p", name), lambda: oracle.packed_to_padded(x, first, max_size))
    back = _want(("pad2p", name), lambda: oracle.padded_to_packed(padded, first, F))
    if name == "unowned_rows":
        assert (back[:2] == 0).all() and (back[2:] != 0).all()
    else:
        g = load_golden("packed_padded")
        assert np.array_equal(padded, g[name + "/padded"].reshape(padded.shape))

    def run(x, check):
        p = _C.packed_to_padded(G(x, dev), G(first, dev), max_size)
        q = _C.padded_to_packed(p, G(first, dev), F)
        if check:
            assert np.array_equal(bits(p.cpu().numpy()), bits(padded)), (name, fill)
            assert np.array_equal(bits(q.cpu().numpy()), bits(back)), (name, fill)

    # (the sibling: other points; "full lengths" has no meaning for offsets -- the padding it leaves behind is the
    # sibling's own zeros, and the ones fill is what shows an unwritten padding row here)
    _held(monkeypatch, fill, ("packed", name), lambda: run(x, True), lambda: run(_other(x.shape, 5) + 1.0, False))


# ------------------------------------------------------------------------------------------------ sample_pdf
@FILLS
@pytest.mark.parametrize("name", sorted(cases.sample_pdf_cases()))
def test_sample_pdf(dev, oracle, monkeypatch, name, fill):
    """In place on `outputs`, the entry's one non-const buffer: it is taken from the seam so that it lies between
    guards (its content on entry is the quantiles, so the fills do not apply to it)."""
    from pytorch3d_pointops_amd import _C

    c = cases.sample_pdf_cases()[name]
    want = _want(("pdf", name), lambda: oracle.sample_pdf(c["bins"], c["weights"], c["u"], c["eps"]))
    assert np.array_equal(bits(want), bits(load_golden("sample_pdf")[name + "/samples"]))

    def run(check):
        out = _C._out(c["u"].shape, dtype=torch.float32, device=dev)
        out.copy_(G(c["u"], dev))
        _C.sample_pdf(G(c["bins"], dev), G(c["weights"], dev), out, c["eps"])
        if check:
            assert np.array_equal(bits(out.cpu().numpy()), bits(want)), (name, fill)

    _held(monkeypatch, fill, ("pdf", name), lambda: run(True), lambda: run(False))


# ------------------------------------------------------------------------------------------------ covariances
@FILLS
@pytest.mark.parametrize("D,K", [(1, 3), (3, 8), (5, 7), (8, 12)])
def test_point_covariances(dev, monkeypatch, D, K, fill):
    """The generator, the composed torch reference and `close` of test_point_covariances_wide_and_wmean."""
    from pytorch3d_pointops_amd import _C

    knn = cases.cloud(2100 + D, (2, 300, K, D))
    gcov = cases.grad_for("covw%d" % D, (2, 300, D, D))

    def want():
        t = torch.from_numpy(knn).double().requires_grad_(True)
        cd = t - t.mean(2, keepdim=True)
        ref = (cd.unsqueeze(4) * cd.unsqueeze(3)).mean(2)
        (ref * torch.from_numpy(gcov).double()).sum().backward()
        return ref.detach().numpy(), t.grad.numpy()

    def run(knn, check):
        cov = _C.point_covariances(G(knn, dev))
        gk = _C.point_covariances_backward(G(knn, dev), G(gcov, dev))
        if check:
            ref, gref = _want(("cov", D), want)
            assert close(cov.cpu().numpy(), ref) and close(gk.cpu().numpy(), gref), (D, K, fill)

    _held(monkeypatch, fill, ("cov", D), lambda: run(knn, True), lambda: run(_other(knn.shape, D), False))


# ------------------------------------------------------------------------------------------------ local frames
@FILLS
def test_local_frames(dev, monkeypatch, fill):
    """test_against_float64_eigh of test_points_normals_gpu.py (its eigh comparison and bars; lengths P, P - 137,
    K + 1; padded rows exactly zero) and its gradient test, run as they are under the contract.  The sibling makes the
    same calls on full clouds of another seed."""
    import pytorch3d_pointops_amd.functions.points_normals as pn
    from pytorch3d_pointops_amd.structures import Pointclouds

    N, P, K = 3, 700, 16

    def sibling():
        pts = G(normals._clouds("uniform", N, P, 4900), dev)
        pc = Pointclouds([pts[n] for n in range(N)])
        pn.estimate_pointcloud_local_coord_frames(pc, K)
        pn.estimate_pointcloud_local_coord_frames(pc, K, False)
        normals._reference(pc.points_padded(), pc.num_points_per_cloud(), K)

    _held(monkeypatch, fill, ("local_frames",), lambda: normals.test_against_float64_eigh(dev, "uniform", K), sibling)


@FILLS
def test_local_frames_backward(dev, monkeypatch, fill):
    """test_gradients_against_float64 (disambiguated) under the contract; its scatter of the point gradients uses
    atomics.  The sibling is the same run on a cloud of another seed."""
    cloud = cases.cloud

    def sibling():
        with monkeypatch.context() as m:
            m.setattr(cases, "cloud", lambda seed, shape, *a: cloud(seed + 977, shape, *a))
            normals.test_gradients_against_float64(dev, True)

    _held(monkeypatch, fill, ("local_frames_bwd",), lambda: normals.test_gradients_against_float64(dev, True), sibling,
          atomic=True)


# ------------------------------------------------------------------------------------------------ registration
def _reseeded(monkeypatch, fn, *args):
    cloud = align._cloud

    def sibling():
        with monkeypatch.context() as m:
            m.setattr(align, "_cloud", lambda name, N, P, seed: cloud(name, N, P, seed + 977))
            fn(*args)

    return sibling


@FILLS
def test_points_alignment(dev, monkeypatch, fill):
    """test_alignment_ragged_and_degenerate (lengths 0, 1, 2, 3 next to ordinary ones, collinear and coincident clouds)
    against the float64 checker of points_alignment_ref.py, under the contract."""
    _held(monkeypatch, fill, ("alignment",), lambda: align.test_alignment_ragged_and_degenerate(dev),
          _reseeded(monkeypatch, align.test_alignment_ragged_and_degenerate, dev), entries=["pointops_points_alignment"])


@FILLS
def test_points_alignment_backward(dev, monkeypatch, fill):
    """test_alignment_gradients_against_float64 (with scale; lengths 400, 333, 57 through the containers)."""
    _held(monkeypatch, fill, ("alignment_bwd",), lambda: align.test_alignment_gradients_against_float64(dev, True),
          _reseeded(monkeypatch, align.test_alignment_gradients_against_float64, dev, True),
          entries=["pointops_points_alignment"])


@FILLS
def test_icp(dev, monkeypatch, fill):
    """test_icp_one_iteration_is_exact_composition (the float64 checker on the package's own neighbour table) and one
    run of three iterations, whose every result equals the run on ordinary buffers bit for bit (no floating-point
    atomics).  The state's buffers are filled once, at construction: it keeps the grid, rmse and Xt between steps."""
    icp = align._api().iterative_closest_point
    X, Y, lx, ly, _ = align._subset_setup(7000, align.SUBSET_SIZES)
    sX, sY, slx, sly, _ = align._subset_setup(7977, [(2000, 3000)] * 3)

    def three(X, Y, lx, ly):
        pcx, pcy = align._pcs(X, Y, lx, ly, dev)
        sol = icp(pcx, pcy, max_iterations=3, relative_rmse_thr=-1.0, estimate_scale=True)
        assert len(sol.t_history) == 3
        return [sol.rmse, sol.Xt.points_padded()] + [t for h in sol.t_history for t in h]

    plain = _want(("icp",), lambda: [t.cpu() for t in three(X, Y, lx, ly)])

    def real():
        align.test_icp_one_iteration_is_exact_composition(dev)
        for a, b in zip(three(X, Y, lx, ly), plain):
            assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)), fill

    def sibling():  # the calls of test_icp_one_iteration_is_exact_composition, then the three iterations
        from pytorch3d_pointops_amd.functions import knn_points

        pcx, pcy = align._pcs(sX, sY, slx, sly, dev)
        for estimate_scale in (False, True):
            icp(pcx, pcy, max_iterations=1, estimate_scale=estimate_scale)
            knn_points(pcx.points_padded(), pcy.points_padded(), slx.to(dev), sly.to(dev), K=1)
        three(sX, sY, slx, sly)

    _held(monkeypatch, fill, ("icp",), real, sibling, entries=["pointops_icp_iteration"])


# ------------------------------------------------------------------------------------------------ chamfer
_CHAMFER_CASES = ["d1", "d3", "c4", "c3_c5", "c1"]  # without / with features (both backward kernels), batch_reduction
# "mean" (d1, c3_c5, c1) and None (d3, c4), weights (c1); lengths: full / partial, x empty, y empty, length 1
_CHAMFER_ROUTES = {"pair": ("pointops_chamfer_pair_forward", "pointops_chamfer_pair_backward"),
                   "direction": ("pointops_chamfer_forward",), "composed_forced": ()}


@FILLS
@pytest.mark.parametrize("route", sorted(_CHAMFER_ROUTES))
@pytest.mark.parametrize("name", _CHAMFER_CASES)
def test_chamfer(dev, oracle, monkeypatch, name, route, fill):
    """The smallest cases of test_chamfer_routes_vs_float64 on the one-call pair (chamfer_pair_forward / _backward), the
    per-direction node (chamfer_forward / _backward / _backward_accumulate) and the composed path (chamfer_reduce),
    against chamfer_ref.py through that test's `_compare`; the route is asserted from its call counts."""
    c = next(k for k in chamfer.CASES if k["name"] == name)
    kw, mode = next((kw, mode) for r, kw, mode in chamfer._routes(c) if r == route)
    want = _want(("chamfer", name, route), lambda: chamfer._run_ref(chamfer.CachedKnn(oracle), c, kw))
    N, P1, D = c["x"].shape
    P2 = c["y"].shape[1]
    s = chamfer._case("sibling", 977, D, tuple(v.shape[2] for _, v in sorted(c["fx"].items())), N=N, P1=P1, P2=P2,
                      norm=c["norm"], abs_cosine=c["abs_cosine"], weights=c["w"], pr=c["pr"], br=c["br"], lengths="full")
    calls = chamfer._counting(monkeypatch)

    def run(case, check):
        for k in calls:
            calls[k] = 0
        with chamfer._mode(monkeypatch, mode):
            got = chamfer._run_gpu(dev, case, kw)
        if check:
            assert (calls["pair"], calls["forward"], calls["composed"]) == chamfer._expected_calls(c, route, kw), calls
            chamfer._compare(got, want, (name, route, fill))

    _held(monkeypatch, fill, ("chamfer", name, route), lambda: run(c, True), lambda: run(s, False), atomic=True,
          entries=_CHAMFER_ROUTES[route])


@FILLS
def test_chamfer_of_an_empty_batch(dev, monkeypatch, fill):
    """N == 0: test_chamfer_of_an_empty_batch_is_zero, with the fill in place of its hand-freed NaN block."""
    run = lambda: parity.test_chamfer_of_an_empty_batch_is_zero(dev)  # noqa: E731
    _held(monkeypatch, fill, ("chamfer_empty",), run, run, atomic=True)


# ------------------------------------------------------------------------------------------------ the tables
def test_every_path_of_the_frames_tables_is_here(dev):
    """No path is left out: every path of the tables of test_coordinate_frames_gpu.py has its entry here (a path added
    there without one fails this test), with every base of the long-list, wide and FPS paths."""
    assert set(_KNN) == set(fr._BRUTE) | set(fr._GRID) | set(fr._LONG) | set(fr._SMALLP) | set(fr._WIDEP)
    assert all(path in table for path, (table, _, _, _) in _KNN.items())
    assert {p for p, _ in _KNN_PARAMS} == set(_KNN) and len(_KNN_PARAMS) == 15
    for table in (fr._LONG, fr._WIDEP):
        assert all((path, name) in _KNN_PARAMS for path, (_, names) in table.items() for name in names)
    assert [p for p, _ in _BALL_PARAMS] == list(fr._BALL) and set(fr._BALL) == set(fr._BALL_KNOBS)
    assert _FPS_PARAMS == [(path, name) for path, (_, names) in fr._FPS.items() for name in names] and len(_FPS_PARAMS) == 7
    assert [p for p, _ in _BWD_PARAMS] == list(fr._BWD) and set(fr._BWD) == set(_BWD_KNOBS)
    assert set(_CHAMFER_CASES) <= {c["name"] for c in chamfer.CASES}
    assert set(_CHAMFER_ROUTES) <= {r for r, _, _ in chamfer._routes(chamfer.CASES[0])}
