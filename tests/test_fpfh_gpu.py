"""GPU suite of the FPFH feature (functions/fpfh.py, csrc/fpfh.hip), staged so that no discontinuity is compared across
precisions:
  1. the pair features against the float64 checker (tests/fpfh_ref.py) on the same fp32 inputs and the same table,
     each error over its conditioning term;
  2. the bins and the SPFH bit for bit, recomputed in numpy float32 from the device's OWN pair features;
  3. the FPFH against float64 from the device's OWN SPFH;
then the edges, the buffer contract, determinism and graph capture, a rigid motion, the correspondence search and the
routes of the public function.  Per case the device runs once and the float64 reference is computed once."""
import numpy as np
import pytest
import torch

import buffers
import fpfh_ref as ref
from conftest import bits
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
CASES = [(name, K) for name in ref.CLOUDS for K in ref.KS]
_RUNS = {}


def _api():
    from pytorch3d_pointops_amd import functions

    return functions


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Run:
    """One device evaluation of a cloud over a table, and the float64 pair features of the same inputs."""

    def __init__(self, dev, pts, nrm, lengths, idx):
        f = _api()
        self.pts, self.nrm, self.lengths = pts, nrm, None if lengths is None else np.asarray(lengths, np.int64)
        self.t = (_t(pts, dev), _t(nrm, dev), None if lengths is None else _t(self.lengths, dev))
        self.tidx = idx
        self.idx = idx.cpu().numpy()
        self.pair = f.point_pair_features(self.t[0], self.t[1], idx, self.t[2])
        self.fpfh, self.spfh = f.fpfh_features(self.t[0], self.t[1], self.t[2], idx=idx, return_spfh=True)
        assert not (self.pair.requires_grad or self.fpfh.requires_grad or self.spfh.requires_grad)
        self.f64 = ref.pair_features(pts, nrm, self.idx, self.lengths, np.float64)
        N, P = pts.shape[:2]
        self.valid = np.arange(P)[None, :] < (np.full(N, P) if lengths is None else self.lengths)[:, None]


def _knn_run(dev, pts, nrm, lengths, K):
    tp, tl = _t(pts, dev), _t(np.asarray(lengths, np.int64), dev)
    return _Run(dev, pts, nrm, lengths, _api().knn_points(tp, tp, tl, tl, K=K).idx)


def _run(dev, name, K):
    if (name, K) not in _RUNS:
        N, P = ref.shape_for(K)
        pts, nrm = ref.cloud(name, N, P)
        _RUNS[name, K] = _knn_run(dev, pts, nrm, ref.lengths_for(P, K), K)
    return _RUNS[name, K]


def _check_pair_features(r, what):
    got = r.pair.cpu().numpy()
    rep = ref.pair_feature_report(got, r.f64)
    print(what, "device error over bound (f1, f2, f3, d):", rep["ratio"], "excluded:", rep["excluded"])
    assert rep["excluded"] <= 0.01, what
    assert np.array_equal(got[..., 3][rep["kept"]] > 0, r.f64["counted"][rep["kept"]]), what
    assert not got[~r.f64["live"]].any(), what  # dead slots and padding rows: exact zeros
    assert max(rep["ratio"]) <= 1.0, (what, rep["ratio"])


def _check_spfh_bits(r, what):
    got = r.pair.cpu().numpy()
    want = ref.spfh_from_bins(ref.bins(got), got[..., 3] > 0)
    have = r.spfh.cpu().numpy()
    assert np.array_equal(bits(have), bits(want)), (what, int((bits(have) != bits(want)).sum()))
    return have


def _check_fpfh(r, what):
    have = r.fpfh.cpu().numpy()
    want = ref.fpfh_from_spfh(r.spfh.cpu().numpy(), r.idx, r.f64["live"], r.f64["d2"], np.float64)
    err = float(np.abs(have - want).max()) if have.size else 0.0
    print(what, "device fpfh error over 200 * 2^-24:", err / (200 * ref.EPS))
    assert not have[~r.valid].any() and not r.spfh.cpu().numpy()[~r.valid].any(), what
    assert err <= ref.T_FPFH, (what, err)
    return have


def _staged(r, what):
    _check_pair_features(r, what)
    _check_spfh_bits(r, what)
    return _check_fpfh(r, what)


def _group_sums(h):
    return h.astype(np.float64).reshape(*h.shape[:2], 3, 11).sum(-1)


# ------------------------------------------------------------------------------------------------ 1-3: the stages
@pytest.mark.parametrize("name,K", CASES)
def test_pair_features_against_float64(dev, name, K):
    _check_pair_features(_run(dev, name, K), f"{name} K={K}")


@pytest.mark.parametrize("name,K", CASES)
def test_bins_and_spfh_bit_exact(dev, name, K):
    r = _run(dev, name, K)
    sp = _check_spfh_bits(r, f"{name} K={K}")
    sums = _group_sums(sp)
    m = (r.pair.cpu().numpy()[..., 3] > 0).sum(2)
    assert np.abs(sums[m > 0] - 100.0).max(initial=0.0) <= 1e-4 and not sums[m == 0].any()


@pytest.mark.parametrize("name,K", CASES)
def test_fpfh_against_float64(dev, name, K):
    _check_fpfh(_run(dev, name, K), f"{name} K={K}")


# ------------------------------------------------------------------------------------------------ 4: edges
def test_self_table_gives_zeros(dev):
    r = _run(dev, "uniform", 1)
    assert (r.idx[r.valid][:, 0] == np.nonzero(r.valid)[1]).all()  # K = 1: every row holds itself
    assert not r.pair.any() and not r.spfh.any() and not r.fpfh.any()


def test_ball_query_table_with_empty_rows(dev):
    N, P, K = 3, 700, 4
    pts, nrm = ref.cloud("uniform", N, P)
    lengths = ref.lengths_for(P, K)  # (about 1.5 points within the radius of a point: P(none) = 0.22, P(>= 3) = 0.19)
    tp, tl = _t(pts, dev), _t(lengths, dev)
    idx = _api().ball_query(tp, tp, tl, tl, K=K, radius=0.08, return_nn=False).idx
    r = _Run(dev, pts, nrm, lengths, idx)
    _staged(r, "ball_query")
    assert (r.idx == -1).any()
    alone = r.valid & ((r.idx >= 0).sum(2) == 1)  # only itself within the radius
    crowded = (r.idx >= 0).all(2)
    assert alone.any() and crowded.any()
    assert not r.spfh.cpu().numpy()[alone].any() and not r.fpfh.cpu().numpy()[alone].any()


@pytest.mark.parametrize("kind", ["duplicates", "zero_normals"])
def test_degenerate_clouds_stay_finite(dev, kind):
    N, P, K = 2, 300, 8
    pts, nrm = ref.cloud("sphere", N, P)
    if kind == "duplicates":
        pts[:, 1::2] = pts[:, ::2]  # every point twice, with different normals
    else:
        nrm[:] = 0.0
    r = _knn_run(dev, pts, nrm, [P, P - 37], K)
    if kind == "duplicates":
        _check_pair_features(r, kind)  # (with zero normals every slot has s = 0: nothing to compare)
    _check_spfh_bits(r, kind)
    fp = _check_fpfh(r, kind)
    sp = r.spfh.cpu().numpy()
    assert np.isfinite(fp).all() and np.isfinite(sp).all() and np.isfinite(r.pair.cpu().numpy()).all()
    sums = _group_sums(sp)
    assert (np.minimum(np.abs(sums - 100.0), np.abs(sums)) <= 1e-4).all()
    if kind == "zero_normals":
        assert not fp.any() and not r.pair.any()  # dp x 0 = 0: no slot is counted
    else:
        assert (sums[r.valid] > 0).all()
        twin = r.idx[0, 0] == 1  # point 0's table holds its duplicate, a dead slot
        assert twin.any() and not r.pair.cpu().numpy()[0, 0][twin].any()


def test_smallest_and_empty_shapes(dev):
    f = _api()
    one = torch.zeros(1, 1, 1, dtype=torch.int64, device=dev)
    p = torch.ones(1, 1, 3, device=dev)
    fp, sp = f.fpfh_features(p, p, idx=one, return_spfh=True)
    assert fp.shape == (1, 1, 33) and not fp.any() and not sp.any()
    assert not f.point_pair_features(p, p, one).any()
    for N, P in ((0, 5), (2, 0)):
        p = torch.ones(N, P, 3, device=dev)
        idx = torch.zeros(N, P, 4, dtype=torch.int64, device=dev)
        fp, sp = f.fpfh_features(p, p, idx=idx, return_spfh=True)
        assert fp.shape == (N, P, 33) and sp.shape == (N, P, 33) and fp.dtype == torch.float32
        assert f.point_pair_features(p, p, idx).shape == (N, P, 4, 4)


def test_lengths_shorter_than_K(dev):
    """knn_points pads the table of a cloud with fewer than K points with index 0: in a row i != 0 that slot points at
    the live point 0 and is counted (again); in row 0 it is the self match."""
    N, P, K = 2, 50, 8
    pts, nrm = ref.cloud("heightfield", N, P)
    r = _knn_run(dev, pts, nrm, [P, 5], K)
    _staged(r, "short cloud")
    assert (r.idx[1, :5, 5:] == 0).all()
    d = r.pair.cpu().numpy()[1, :5, :, 3]
    assert (d[1:, 5:] > 0).all() and not d[0, 5:].any()
    assert (d[1:, 5:] == d[1:, 5:6]).all()


# ------------------------------------------------------------------------------------------------ 5: memory contract
_BASELINE = {}


def _both_entries(p, n, idx, lengths):
    f = _api()
    pair = f.point_pair_features(p, n, idx, lengths)
    fp, sp = f.fpfh_features(p, n, lengths, idx=idx, return_spfh=True)
    return pair, sp, fp


def _under_contract(monkeypatch, dev, fill):
    r = _run(dev, "heightfield", 16)
    N, P = ref.shape_for(16)
    spts, snrm = ref.cloud("sphere", N, P, seed=1)  # the sibling: other points, full lengths, its own table
    sp, sn, sl = _t(spts, dev), _t(snrm, dev), _t(np.full(N, P, np.int64), dev)
    sidx = _api().knn_points(sp, sp, sl, sl, K=16).idx
    with buffers.contract(monkeypatch, fill, prototypes=PROTOS) as c:
        c.sibling(lambda: _both_entries(sp, sn, sidx, sl))
        c.watch(points=r.t[0], normals=r.t[1], lengths=r.t[2], idx=r.tidx)
        out = _both_entries(r.t[0], r.t[1], r.tidx, r.t[2])
    c.assert_all_clear()
    assert [b.kind for b in c.buffers] == ["out"] * 4 and c.inputs_checked >= 8
    for got, want in zip(out, (r.pair, r.spfh, r.fpfh)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
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


# ------------------------------------------------------------------------------------------------ 6: determinism
def test_two_runs_are_bit_equal(dev):
    r = _run(dev, "sphere", 50)
    pair, sp, fp = _both_entries(r.t[0], r.t[1], r.tidx, r.t[2])
    for got, want in ((pair, r.pair), (sp, r.spfh), (fp, r.fpfh)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_graph_capture_replays_the_eager_result(dev):
    from pytorch3d_pointops_amd import graphs

    r = _run(dev, "heightfield", 16)
    p, n = r.t[0].clone(), r.t[1].clone()
    step = graphs.capture(lambda a, b: _api().fpfh_features(a, b, r.t[2], idx=r.tidx, return_spfh=True), (p, n))
    fp, sp = step()
    assert torch.equal(fp.view(torch.int32), r.fpfh.view(torch.int32))
    assert torch.equal(sp.view(torch.int32), r.spfh.view(torch.int32))
    q = _run(dev, "sphere", 16)  # other points through the static inputs, the same table
    want = _api().fpfh_features(q.t[0], q.t[1], r.t[2], idx=r.tidx)
    assert torch.equal(step(q.t[0], q.t[1])[0].view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 7: rigid motion
def _moved_run(dev):
    if "moved" not in _RUNS:
        r = _run(dev, "heightfield", 16)
        mp, mn = ref.moved(r.pts, r.nrm)
        _RUNS["moved"] = _Run(dev, mp, mn, r.lengths, r.tidx)
    return _RUNS["moved"]


def test_rigid_motion(dev):
    r, m = _run(dev, "heightfield", 16), _moved_run(dev)
    diff = (r.fpfh - m.fpfh).abs().amax(-1).cpu().numpy()[r.valid]
    print("rigid motion: rows above 1e-3:", int((diff > 1e-3).sum()), "of", diff.size, "median", float(np.median(diff)))
    assert (diff > 1e-3).mean() <= 0.01


# ------------------------------------------------------------------------------------------------ 8: correspondences
def test_mutual_nearest_neighbors_against_brute_force(dev):
    rng = np.random.default_rng(11)
    N, P1, P2, D = 3, 300, 257, 33
    a, b = rng.random((N, P1, D), np.float32), rng.random((N, P2, D), np.float32)
    l1, l2 = np.array([300, 163, 40]), np.array([257, 100, 0])
    got = _api().mutual_nearest_neighbors(_t(a, dev), _t(b, dev), _t(l1, dev), _t(l2, dev)).cpu().numpy()
    assert got.shape == (N, P1) and got.dtype == np.int64
    want = np.full((N, P1), -1, np.int64)
    for n in range(N):
        if l1[n] and l2[n]:
            d = ((a[n, :l1[n], None].astype(np.float64) - b[n, None, :l2[n]].astype(np.float64)) ** 2).sum(-1)
            fwd, bwd = d.argmin(1), d.argmin(0)
            rows = np.arange(l1[n])
            want[n, :l1[n]] = np.where(bwd[fwd] == rows, fwd, -1)
    assert np.array_equal(got, want)
    assert (want[0] >= 0).any() and (want[0] == -1).any() and (want[2] == -1).all()
    full = _api().mutual_nearest_neighbors(_t(a[:1], dev), _t(b[:1], dev)).cpu().numpy()
    assert np.array_equal(full, want[:1])
    assert _api().mutual_nearest_neighbors(_t(a[:, :0], dev), _t(b, dev)).shape == (N, 0)
    assert (_api().mutual_nearest_neighbors(_t(a, dev), _t(b[:, :0], dev)) == -1).all()


def test_descriptors_match_a_moved_and_permuted_cloud(dev):
    r, m = _run(dev, "heightfield", 16), _moved_run(dev)
    P = r.pts.shape[1]
    perm = np.random.default_rng(12).permutation(P)
    f1, f2 = r.fpfh[:1], m.fpfh[:1][:, _t(perm, dev)]  # row j of f2 describes point perm[j]
    match = _api().mutual_nearest_neighbors(f1, f2).cpu().numpy()[0]
    found = match >= 0
    print("mutual matches:", int(found.sum()), "of", P)
    assert found.mean() >= 0.99
    assert (perm[match[found]] == np.nonzero(found)[0]).all()


# ------------------------------------------------------------------------------------------------ 9: routes
def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_routes_equal_their_explicit_composition(dev):
    from pytorch3d_pointops_amd.structures import Pointclouds

    f = _api()
    r = _run(dev, "sphere", 16)
    p, n, lengths = r.t
    assert _same(f.fpfh_features(p, n, lengths, K=16), r.fpfh)  # (the case's table is knn_points')
    ball = f.ball_query(p, p, lengths, lengths, K=12, radius=0.3, return_nn=False).idx
    assert _same(f.fpfh_features(p, n, lengths, K=12, radius=0.3), f.fpfh_features(p, n, lengths, idx=ball))
    assert (ball == -1).any()
    pc = Pointclouds([p[i, :int(r.lengths[i])] for i in range(p.shape[0])])
    assert _same(f.fpfh_features(pc, n, K=16), r.fpfh)
    est = f.estimate_pointcloud_normals(pc, neighborhood_size=16)
    got, sp = f.fpfh_features(pc, K=16, return_spfh=True)
    want, wsp = f.fpfh_features(p, est, lengths, idx=r.tidx, return_spfh=True)
    assert _same(got, want) and _same(sp, wsp) and not _same(got, r.fpfh)
    full = f.estimate_pointcloud_normals(p, neighborhood_size=16)
    idx = f.knn_points(p, p, K=16).idx
    assert _same(f.fpfh_features(p, K=16), f.fpfh_features(p, full, idx=idx))


def test_compiled_call_returns_the_eager_result(dev):
    f = _api()
    r = _run(dev, "sphere", 16)
    p, n, lengths = r.t

    def fn(a, b):
        return f.fpfh_features(a * 1.0, b, lengths, K=16) + 0.0

    assert _same(torch.compile(fn, backend="aot_eager")(p, n), r.fpfh)
