"""knn_in_radius on the GPU against tests/knn_in_radius_ref.py, byte for byte:
    cases        every case of tests/knn_in_radius_cases.py on three paths -- the library's choice (under guarded,
                 poisoned buffers with a short and a null workspace tried first), POINTOPS_DEBUG=knn_in_radius_grid=0 (the
                 raw cloud) and =1 (a grid whatever the size), the forced ones each in ONE fresh child process that runs
                 the whole case file -- and, on finite cases, against functions.knn_points masked on the device
    rule         counts = the non-negative slots; a row's dists ascend, equal dists in ascending idx
    bytes        two calls, a cloud alone and in its batch, reuse = 1 with new queries against a fresh call
    gradients    of (w * dists).sum() against a float64 torch evaluation over the same idx
    contract     the other fills, bad native arguments, empty shapes, 65 540 clouds, a side stream, a captured graph
                 replayed with new coordinates, the Pointclouds method, the composed routes (D = 4, K = 65)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import buffers
import knn_in_radius_cases as cases
import knn_in_radius_ref as ref
from conftest import ROOT
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
ENTRY = "pointops_knn_in_radius"
CASES = cases.build_cases()
_WANT = {}


def _want(name):
    if name not in _WANT:
        c = CASES[name]
        _WANT[name] = ref.knn_in_radius(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)
    return _WANT[name]


def _assert_equal(got, want, what, keys=cases.KEYS):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} is {a.dtype}{a.shape}, want {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))
            at = tuple(bad[0][:-1])
            raise AssertionError(f"{what}: {k} differs at {len(bad)} bytes, first at {at}: got {a[at]!r}, want {b[at]!r}")


def _assert_rule(got, what):
    idx, d = got["idx"], got["dists"]
    assert np.array_equal(got["counts"], (idx >= 0).sum(2)), f"{what}: counts"
    assert np.all((idx[..., 1:] < 0) | (idx[..., :-1] >= 0)), f"{what}: a hole in a row"
    valid = idx[..., 1:] >= 0
    assert np.all(~valid | (d[..., :-1] < d[..., 1:]) | ((d[..., :-1] == d[..., 1:]) & (idx[..., :-1] < idx[..., 1:]))), what
    assert np.all((idx >= 0) | (d == 0)), f"{what}: a padded distance"


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _npy(out):
    return {k: t.detach().cpu().numpy() for k, t in zip(cases.KEYS, out)}


@pytest.fixture(scope="module")
def forced_paths(tmp_path_factory):
    """{knob value: the npz a fresh child process saved of every case under POINTOPS_DEBUG=knn_in_radius_grid=value}"""
    out = {}
    for value in (0, 1):
        path = str(tmp_path_factory.mktemp("knn_in_radius") / f"grid{value}.npz")
        env = dict(os.environ, POINTOPS_DEBUG=f"knn_in_radius_grid={value}",
                   PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "knn_in_radius_cases.py"), path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out[value] = np.load(path)
    return out


# ------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("name", [n for n in CASES if n != cases.AUTO])
def test_case_equals_the_checker_on_every_path(dev, monkeypatch, forced_paths, name):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    c, want = CASES[name], _want(name)
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=PROTOS) as k:
        got = cases.run_case(dev, c)
    k.assert_all_clear()
    assert {(n, how) for n, _, how in k.rejections} == {(ENTRY, "short"), (ENTRY, "null")}
    assert [b.kind for b in k.buffers] == ["out"] * 3 + ["workspace"] and k.inputs_checked >= 2
    _assert_equal(got, want, f"{name} [default]")
    _assert_rule(got, name)
    for value, saved in forced_paths.items():
        _assert_equal({key: saved[f"{name}/{key}"] for key in cases.KEYS}, want, f"{name} [knn_in_radius_grid={value}]")
    if c.finite:
        p1, p2, l1, l2 = _dev(dev, c.p1, c.p2, c.lengths1, c.lengths2)
        nn = f.knn_points(p1, p2, l1, l2, K=c.K)
        r2 = float(ref.r2_of(c.radius))
        keep = (nn.dists < r2) & (torch.arange(c.K, device=dev)[None, None] < l2[:, None, None]) & \
            (torch.arange(p1.shape[1], device=dev)[None, :, None] < l1[:, None, None])
        masked = dict(idx=torch.where(keep, nn.idx, -1), dists=torch.where(keep, nn.dists, 0.0),
                      counts=keep.sum(2).to(torch.int32))
        _assert_equal({key: v.cpu().numpy() for key, v in masked.items()}, want, f"{name} [knn_points masked]")


def test_self_query_as_the_same_tensor_and_as_a_clone_agree(dev, monkeypatch):
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    a, b = cases.run_case(dev, CASES["self-same-tensor"]), cases.run_case(dev, CASES["self-clone"])
    _assert_equal(a, b, "same tensor against clone")
    assert (a["idx"][0, :, 0] == np.arange(700)).all() and not a["dists"][0, :, 0].any()  # (itself first, at d2 = 0)


def test_the_library_chooses_its_path_on_a_large_cloud(dev, monkeypatch):
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    from pytorch3d_pointops_amd import _C

    c = CASES[cases.AUTO]
    small = _C._lib.pointops_knn_in_radius_workspace_bytes(1, 100, 100, 3, 8)
    assert _C._lib.pointops_knn_in_radius_workspace_bytes(1, 20000, 20000, 3, 8) > 100 * small  # (a grid's worth)
    got = cases.run_case(dev, c)
    _assert_equal(got, _want(cases.AUTO), cases.AUTO)
    _assert_rule(got, cases.AUTO)
    assert (got["counts"] < 8).any() and (got["counts"] == 8).any()


# ------------------------------------------------------------------------------------------------ bytes
def test_two_calls_and_a_cloud_alone_give_the_same_bytes(dev, monkeypatch):
    from pytorch3d_pointops_amd import _C_knn_in_radius as op

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    for name in ("uniform-D3-K9", "surface-and-clutter-K4", "nan-and-inf-rows"):
        c = CASES[name]
        first = cases.run_case(dev, c)
        _assert_equal(cases.run_case(dev, c), first, f"{name}: second call")
        for n in range(c.p1.shape[0]):
            t = _dev(dev, c.p1[n:n + 1], c.p2[n:n + 1], c.lengths1[n:n + 1], c.lengths2[n:n + 1])
            alone = _npy(op.knn_in_radius(*t, c.K, c.radius))
            _assert_equal(alone, {k: v[n:n + 1] for k, v in first.items()}, f"{name}: cloud {n} alone")


@pytest.mark.parametrize("name", ["uniform-D3-K5", "surface-and-clutter-K1", "self-clone", "one-row-K1"])
def test_reuse_with_new_queries_equals_a_fresh_call(dev, monkeypatch, name):
    from pytorch3d_pointops_amd import _C_knn_in_radius as op

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    c = CASES[name]
    p1, p2, l1, l2 = _dev(dev, c.p1, c.p2, c.lengths1, c.lengths2)
    *first, ws = op.knn_in_radius(p1, p2, l1, l2, c.K, c.radius)
    _assert_equal(_npy(first), _want(name), f"{name}: the call that builds")
    q = np.ascontiguousarray(c.p1[:, ::-1] * np.float32(0.97) + np.float32(0.01))  # other queries, same shape
    lq = np.maximum(c.lengths1 - 1, 0)
    q1, lq1 = _dev(dev, q, lq)
    *again, ws2 = op.knn_in_radius(q1, p2, lq1, l2, c.K, c.radius, workspace=ws, reuse=True)
    assert ws2 is ws
    want = ref.knn_in_radius(q, c.p2, lq, c.lengths2, c.K, c.radius)
    _assert_equal(_npy(again), want, f"{name}: reuse = 1")
    _assert_equal(_npy(op.knn_in_radius(q1, p2, lq1, l2, c.K, c.radius)[:3]), want, f"{name}: fresh")
    with pytest.raises(RuntimeError, match="reuse needs the workspace"):
        op.knn_in_radius(q1, p2, lq1, l2, c.K, c.radius, reuse=True)


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name", ["uniform-D3-K8", "uniform-D2-K4", "duplicates-K5", "self-same-tensor"])
def test_gradients_against_float64_over_the_same_idx(dev, monkeypatch, name):
    """The backward is knn_points': fp32 atomics on p2's side.  The project's bound for atomically accumulated
    gradients is 1e-5 of the largest gradient entry."""
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    c = CASES[name]
    p2, l2 = _dev(dev, c.p2, c.lengths2)
    p2.requires_grad_(True)
    if c.same:
        p1, l1 = p2, l2
    else:
        p1, l1 = _dev(dev, c.p1, c.lengths1)
        p1.requires_grad_(True)
    r = f.knn_in_radius(p1, p2, l1, l2, K=c.K, radius=c.radius)
    assert r.dists.requires_grad and not r.idx.requires_grad and not r.counts.requires_grad
    _assert_equal({k: getattr(r, k).detach().cpu().numpy() for k in cases.KEYS}, _want(name), name)
    w = torch.from_numpy(np.random.default_rng(5).uniform(0.5, 1.5, r.dists.shape).astype(np.float32)).to(dev)
    (w * r.dists).sum().backward()
    a = p1.detach().double().requires_grad_(True)
    b = a if c.same else p2.detach().double().requires_grad_(True)
    hit = r.idx >= 0
    nb = torch.gather(b[:, None].expand(-1, a.shape[1], -1, -1), 2,
                      r.idx.clamp(min=0)[..., None].expand(-1, -1, -1, a.shape[2]))
    d64 = ((a[:, :, None, :] - nb) ** 2).sum(-1)
    (w.double() * torch.where(hit, d64, torch.zeros_like(d64))).sum().backward()  # (padded slots contribute nothing)
    for got, want, what in ((p1.grad, a.grad, "p1"),) + (() if c.same else ((p2.grad, b.grad, "p2"),)):
        scale = float(want.abs().max())
        assert scale > 0 and float((got.double() - want).abs().max()) <= 1e-5 * scale, f"{name}: grad {what}"
    with torch.no_grad():
        assert not f.knn_in_radius(p1, p2, l1, l2, K=c.K, radius=c.radius).dists.requires_grad
    plain = f.knn_in_radius(p1.detach(), p2.detach(), l1, l2, K=c.K, radius=c.radius, return_nn=True)
    assert plain.dists.grad_fn is None and plain.knn.shape == r.idx.shape + (c.p2.shape[2],)
    assert torch.equal(plain.knn, f.masked_gather(p2.detach(), r.idx))


# ------------------------------------------------------------------------------------------------ contract
@pytest.mark.parametrize("fill", ["zero", "stale"])
def test_entry_under_the_other_fills(dev, monkeypatch, fill):
    from pytorch3d_pointops_amd import _C_knn_in_radius as op

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    name = "uniform-D3-K9"
    c = CASES[name]
    p1, p2, l1, l2 = _dev(dev, c.p1, c.p2, c.lengths1, c.lengths2)
    s1, s2 = _dev(dev, c.p1[::-1], c.p2[::-1])
    with buffers.contract(monkeypatch, fill, prototypes=PROTOS) as k:
        k.sibling(lambda: op.knn_in_radius(s1, s2, None, None, c.K, c.radius))
        k.watch(p1=p1, p2=p2, lengths1=l1, lengths2=l2)
        out = op.knn_in_radius(p1, p2, l1, l2, c.K, c.radius)
    k.assert_all_clear()
    assert [b.kind for b in k.buffers] == ["out"] * 3 + ["workspace"] and k.inputs_checked >= 4
    _assert_equal(_npy(out), _want(name), f"[{fill}]")


def test_bad_native_arguments_are_rejected_with_nothing_written(dev):
    from pytorch3d_pointops_amd import _C

    X = torch.rand(1, 8, 3, device=dev)
    outs = [torch.full((4096,), 7, dtype=torch.uint8, device=dev) for _ in range(3)]
    sizer = _C._lib.pointops_knn_in_radius_workspace_bytes
    ws = torch.zeros(sizer(1, 8, 8, 3, 4), dtype=torch.uint8, device=dev)
    for args in ((65536, 8, 8, 3, 4), (-1, 8, 8, 3, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 4), (1, 8, 8, 3, 0), (1, 8, 8, 3, 65),
                 (1, 2 ** 30, 8, 3, 4), (1, 8, -1, 3, 4), (0, 8, 8, 3, 4)):
        assert sizer(*args) == 0
    for bad in (dict(r=0.0), dict(r=-1.0), dict(r=float("inf")), dict(r=float("nan")), dict(D=0), dict(D=4), dict(K=0),
                dict(K=65), dict(N=65536), dict(N=-1), dict(P1=2 ** 30), dict(P2=-1), dict(reuse=2), dict(reuse=-1)):
        a = dict(r=0.1, N=1, P1=8, P2=8, D=3, K=4, reuse=0)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            _C._call.knn_in_radius("knn_in_radius", dev, X, X, None, None, a["N"], a["P1"], a["P2"], a["D"], a["K"],
                                   a["r"], *outs, ws, ws.numel(), a["reuse"])
    for short in ((ws, ws.numel() - 1), (None, ws.numel())):
        with pytest.raises(RuntimeError, match=r"failed \(-3\)"):
            _C._call.knn_in_radius("knn_in_radius", dev, X, X, None, None, 1, 8, 8, 3, 4, 0.1, *outs, *short, 0)
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    # counts is optional, and null lengths mean P
    _C._call.knn_in_radius("knn_in_radius", dev, X, X, None, None, 1, 8, 8, 3, 4, 0.6, outs[0], outs[1], None, ws,
                           ws.numel(), 0)
    want = ref.knn_in_radius(X.cpu().numpy(), X.cpu().numpy(), None, None, 4, 0.6)
    assert outs[0][:256].view(torch.int64).cpu().numpy().reshape(1, 8, 4).tobytes() == want["idx"].tobytes()
    assert outs[1][:128].view(torch.float32).cpu().numpy().reshape(1, 8, 4).tobytes() == want["dists"].tobytes()
    assert bool((outs[2] == 7).all())


def test_empty_batches_and_empty_clouds(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    for N, P1, P2 in ((0, 5, 5), (0, 0, 0), (3, 0, 6), (3, 6, 0)):
        r = f.knn_in_radius(torch.zeros((N, P1, 3), device=dev), torch.zeros((N, P2, 3), device=dev), K=3, radius=0.5)
        assert r.idx.shape == (N, P1, 3) and r.dists.shape == (N, P1, 3) and r.counts.shape == (N, P1)
        assert bool((r.idx == -1).all()) and not bool(r.dists.any()) and not bool(r.counts.any())


def test_many_clouds_cross_the_slice_boundary(dev, monkeypatch):
    """65 540 clouds of 3 points go to the entry in two slices through one workspace."""
    from pytorch3d_pointops_amd import _C_knn_in_radius as op

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    N, P, K, radius = 65540, 3, 2, 0.5
    rng = np.random.default_rng(77)
    p1, p2 = (rng.uniform(0, 1, (N, P, 3)).astype(np.float32) for _ in range(2))
    l1, l2 = (rng.integers(0, P + 1, N).astype(np.int64) for _ in range(2))
    l1[[0, 65534, 65535, 65536, N - 1]] = P
    l2[[0, 65534, 65535, 65536, N - 1]] = P
    t = _dev(dev, p1, p2, l1, l2)
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=PROTOS) as k:
        k.watch(p1=t[0], p2=t[1])
        got = _npy(op.knn_in_radius(*t, K, radius))
    k.assert_all_clear()
    assert len(k.rejections) == 4  # two native calls
    _assert_equal(got, ref.knn_in_radius(p1, p2, l1, l2, K, radius), "65 540 clouds")
    assert 1000 < (got["counts"] == 1).sum() and 1000 < (got["counts"] == 2).sum()


def test_a_side_stream_gives_the_same_bytes(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    name = "surface-and-clutter-K4"
    c = CASES[name]
    t = _dev(dev, c.p1, c.p2, c.lengths1, c.lengths2)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        r = f.knn_in_radius(*t, K=c.K, radius=c.radius)
    side.synchronize()
    _assert_equal({k: getattr(r, k).cpu().numpy() for k in cases.KEYS}, _want(name), "side stream")


def test_graph_capture_replays_with_new_coordinates(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd import graphs

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    c = CASES["surface-and-clutter-K4"]
    l1, l2 = _dev(dev, c.lengths1, c.lengths2)

    def call(a, b):
        r = f.knn_in_radius(a, b, l1, l2, K=c.K, radius=c.radius)
        return r.idx, r.dists, r.counts

    p1, p2 = _dev(dev, c.p1, c.p2)
    step = graphs.capture(call, (p1.clone(), p2.clone()))
    _assert_equal(_npy(step()), _want("surface-and-clutter-K4"), "first scene, replayed")
    q1, q2 = np.ascontiguousarray(c.p1[::-1]), np.ascontiguousarray(c.p2[::-1] * np.float32(1.01))
    want2 = ref.knn_in_radius(q1, q2, c.lengths1, c.lengths2, c.K, c.radius)
    for replay in range(2):
        _assert_equal(_npy(step(*_dev(dev, q1, q2))), want2, f"second scene, replay {replay}")
    assert want2["idx"].tobytes() != _want("surface-and-clutter-K4")["idx"].tobytes()


def test_the_pointclouds_method(dev, monkeypatch):
    from pytorch3d_pointops_amd.structures import Pointclouds

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    c = CASES["uniform-D3-K5"]
    a = Pointclouds([torch.from_numpy(c.p1[n, :c.lengths1[n]]).to(dev) for n in range(4)])
    b = Pointclouds([torch.from_numpy(c.p2[n, :c.lengths2[n]]).to(dev) for n in range(4)])
    r = a.knn_in_radius(b, K=c.K, radius=c.radius)
    _assert_equal({k: getattr(r, k).cpu().numpy() for k in cases.KEYS}, _want("uniform-D3-K5"), "other")
    s = b.knn_in_radius(K=3, radius=0.1, return_nn=True)
    want = ref.knn_in_radius(c.p2, c.p2, c.lengths2, c.lengths2, 3, 0.1)
    _assert_equal({k: getattr(s, k).cpu().numpy() for k in cases.KEYS}, want, "itself")
    assert s.knn.shape == (4, 700, 3, 3)


@pytest.mark.parametrize("D,K", [(4, 3), (3, 65), (5, 70)])
def test_the_composed_routes_equal_the_checker(dev, monkeypatch, D, K):
    from pytorch3d_pointops_amd import functions as f

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    rng = np.random.default_rng(D * 100 + K)
    p1, p2 = rng.uniform(0, 1, (2, 150, D)).astype(np.float32), rng.uniform(0, 1, (2, 200, D)).astype(np.float32)
    l1, l2 = np.array([150, 40]), np.array([200, 30])
    radius = {4: 0.3, 3: 0.45, 5: 0.8}[D]
    t = _dev(dev, p1, p2, l1, l2)
    t[0].requires_grad_(True)
    r = f.knn_in_radius(*t, K=K, radius=radius)
    got = {k: getattr(r, k).detach().cpu().numpy() for k in cases.KEYS}
    _assert_equal(got, ref.knn_in_radius(p1, p2, l1, l2, K, radius), f"D = {D}, K = {K}")
    assert (got["counts"] > 0).any() and (got["counts"][:, :40] < K).any() and r.dists.requires_grad
