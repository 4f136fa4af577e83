"""registration_icp(search="bounded") -- every step's search is the K = 1 knn_in_radius with the run's radius -- against
search="exact", byte for byte, on the scenes and helpers of tests/test_registration_gpu.py:
    public       every field of the result, both estimations, with and without clutter, check_every 0 and 1, a planar
                 (degenerate) cloud and empty clouds beside a healthy one, evaluate_registration, a captured graph
    steps        through RegistrationState, at each of four steps: idx / dists equal the exact run's wherever d2 < r2 and
                 are (-1, 0) elsewhere; everything the step derives from them is byte-equal
    contract     the step in the new mode under poisoned buffers, with its own search workspace short and null"""
import numpy as np
import pytest
import torch

import buffers
import registration_ref as ref
import test_registration_gpu as base
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("check_every", [1, 0])
@pytest.mark.parametrize("clutter", [False, True], ids=["clean", "clutter"])
@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
def test_every_public_output_equals_the_exact_search(dev, monkeypatch, estimation, clutter, check_every):
    from pytorch3d_pointops_amd.functions import registration_icp

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    src, tgt = base._clouds(dev, clutter)
    kw = dict(estimation=estimation, max_iterations=12, check_every=check_every)
    exact = base._fields(registration_icp(src, tgt, ref.R_MAX, **kw))
    bounded = base._fields(registration_icp(src, tgt, ref.R_MAX, search="bounded", **kw))
    base._assert_bytes_equal(bounded, exact, "bounded against exact")
    assert exact["num_correspondences"].min() > 100
    base._assert_bytes_equal(base._fields(registration_icp(src, tgt, ref.R_MAX, search="exact", **kw)), exact, "the keyword")


@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
def test_degenerate_and_empty_clouds_beside_a_healthy_one(dev, monkeypatch, estimation):
    from pytorch3d_pointops_amd.functions import registration_icp
    from pytorch3d_pointops_amd.structures import Pointclouds

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    X, Y, Nr, lx, ly, _ = base._degenerate_batch()
    Xd, Yd, Nd = base._G(dev, X, Y, Nr)
    src = Pointclouds([Xd[n, :lx[n]] for n in range(6)])
    tgt = Pointclouds([Yd[n, :ly[n]] for n in range(6)], features={"normals": [Nd[n, :ly[n]] for n in range(6)]})
    for r_max in (ref.R_MAX, 1e-7):  # (the second: nothing matches anywhere)
        exact = base._fields(registration_icp(src, tgt, r_max, estimation=estimation, max_iterations=20))
        bounded = base._fields(registration_icp(src, tgt, r_max, estimation=estimation, max_iterations=20,
                                                search="bounded"))
        base._assert_bytes_equal(bounded, exact, f"r_max = {r_max}")
    assert set(exact["status"].tolist()) == {ref.DEGENERATE}


def test_evaluate_registration_equals_the_exact_search(dev, monkeypatch):
    from pytorch3d_pointops_amd.functions import evaluate_registration

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    for clutter in (False, True):
        src, tgt = base._clouds(dev, clutter)
        exact = base._fields(evaluate_registration(src, tgt, ref.R_MAX))
        base._assert_bytes_equal(base._fields(evaluate_registration(src, tgt, ref.R_MAX, search="bounded")), exact,
                                 "evaluate_registration")
        base._assert_bytes_equal(base._fields(src.evaluate_registration(tgt, ref.R_MAX, search="bounded")), exact,
                                 "the Pointclouds method")
        assert 0 < exact["num_correspondences"].min()


@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
def test_each_of_four_steps_against_the_exact_run(dev, monkeypatch, estimation):
    from pytorch3d_pointops_amd import _C_registration

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    steps = 4
    exact, _ = base._state(dev, True, estimation, steps, want_moments=True)
    bounded, _ = base._state(dev, True, estimation, steps, want_moments=True, search="bounded")
    assert bounded.search_version == _C_registration.SEARCH_BOUNDED == -2 and bounded.reuse_grid
    _, _, _, lx, ly, _ = base._batch(True)
    r2 = np.float32(ref.R_MAX) * np.float32(ref.R_MAX)
    rows = np.arange(base.P1)[None, :] < lx[:, None]
    names = ("Xt", "state", "status", "iterations", "correspondences", "num_correspondences", "all_frozen", "moments")
    for i in range(steps):
        exact.step(update=True)
        bounded.step(update=True)
        torch.cuda.synchronize()
        ei, ed, bi, bd = (base._npy(t) for t in (exact.idx, exact.dists, bounded.idx, bounded.dists))
        inside = rows & (ed < r2)
        assert inside.any() and (rows & ~inside).any(), f"step {i}"  # (the clutter rows have nothing inside)
        assert np.array_equal(bi[inside], ei[inside]) and bd[inside].tobytes() == ed[inside].tobytes(), f"step {i}"
        assert (bi[~inside] == -1).all() and not bd[~inside].any(), f"step {i}: rows with nothing inside the radius"
        for k in names:
            assert base._npy(getattr(bounded, k)).tobytes() == base._npy(getattr(exact, k)).tobytes(), f"step {i}: {k}"
        for k in ("R", "T", "fitness", "inlier_rmse"):
            assert base._npy(getattr(bounded, k)[i]).tobytes() == base._npy(getattr(exact, k)[i]).tobytes(), f"step {i}: {k}"
    fresh, _ = base._state(dev, True, estimation, steps, reuse_grid=False, search="bounded")  # every step builds
    for i in range(steps):
        fresh.step(update=True)
    for k in ("idx", "dists", "Xt", "state"):
        assert base._npy(getattr(fresh, k)).tobytes() == base._npy(getattr(bounded, k)).tobytes(), f"reuse_grid=False: {k}"


def test_the_whole_bounded_run_replays_from_a_graph(dev, monkeypatch):
    from pytorch3d_pointops_amd import graphs
    from pytorch3d_pointops_amd.functions import registration_icp

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    sc = base._batch(True)[5][1]  # (700, 1100), full lengths: padded tensors in; the target gets a grid
    X, Y, Nr = base._G(dev, sc.X[None], sc.Y[None], sc.normals[None])
    names = ("R", "T", "fitness", "inlier_rmse", "num_correspondences", "correspondences", "iterations", "status", "Xt")

    def fn(x, y, nr, search="bounded"):
        r = registration_icp(x, y, ref.R_MAX, target_normals=nr, max_iterations=8, check_every=0, search=search)
        return tuple(getattr(r, k) for k in names) + tuple(r.history)

    eager = [base._npy(t).copy() for t in fn(X, Y, Nr, search="exact")]
    assert max(ref.pose_error(eager[0][0], eager[1][0], sc)) <= 1e-5
    g = graphs.capture(fn, (X, Y, Nr))
    for replay in range(2):
        out = g()
        torch.cuda.synchronize()
        for name, a, b in zip(names + ("hR", "hT", "hf", "hr"), out, eager):
            assert base._npy(a).tobytes() == b.tobytes(), f"replay {replay}: {name} differs from the exact eager run"


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_buffer_contract_of_the_bounded_step(dev, monkeypatch, fill):
    from pytorch3d_pointops_amd.functions import registration_icp

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)

    def runner(clutter):
        src, tgt = base._clouds(dev, clutter)
        src.points_padded(), tgt.points_padded(), tgt.get_features_padded("normals")  # (padded outside the contract)
        return (lambda: registration_icp(src, tgt, ref.R_MAX, max_iterations=5, check_every=0, search="bounded")), src, tgt

    run, src, tgt = runner(True)
    sibling, _, _ = runner(False)
    plain = base._once("bounded contract plain", lambda: base._fields(run()))
    with buffers.contract(monkeypatch, fill, short_workspace="short" if fill == "ones" else False,
                          prototypes=declared_prototypes()) as c:
        c.sibling(sibling)
        c.watch(source=src.points_padded(), target=tgt.points_padded(), normals=tgt.get_features_padded("normals"),
                len_x=src.num_points_per_cloud(), len_y=tgt.num_points_per_cloud())
        got = base._fields(run())
    c.assert_all_clear()
    assert c.inputs_checked > 0
    base._assert_bytes_equal(got, plain, f"under the {fill} fill")
    if fill == "ones":  # both workspaces -- the search's own among them -- one byte short and null
        rejected = {(name, label) for name, _, label in c.rejections}
        assert {("pointops_registration_step", "short"), ("pointops_registration_step", "null")} <= rejected
        assert len({at for name, at, _ in c.rejections if name == "pointops_registration_step"}) == 2


def test_an_unknown_search_raises(dev):
    from pytorch3d_pointops_amd import _C_registration
    from pytorch3d_pointops_amd.functions import evaluate_registration, registration_icp

    src, tgt = base._clouds(dev, False)
    for call in (lambda: registration_icp(src, tgt, ref.R_MAX, search="nonsense"),
                 lambda: evaluate_registration(src, tgt, ref.R_MAX, search=None),
                 lambda: base._state(dev, False, "point_to_plane", 2, search="nonsense")):
        with pytest.raises(ValueError, match="search"):
            call()
    assert _C_registration.SEARCHES == ("exact", "bounded")
