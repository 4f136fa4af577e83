"""registration_icp / evaluate_registration on the GPU against tests/registration_ref.py, the numpy checker of the
REGISTRATION block of include/pointops_amd.h.  tests/test_registration_cpu.py certifies the inputs: on these scenes the
checker itself converges to the true pose, and the untrimmed run does not.

Every test builds on the surface of the experiment (registration_ref.scene).  The base batch is N = 3, ragged
(P1, P2) = (2500, 3000), (700, 1100), (300, 400): cloud 0 spans two blocks of partials (more than 2048 rows) and both
search families run across the tests (the batch on the scan it takes by itself and, forced by POINTOPS_DEBUG
registration_grid=1, on the grid, whose reuse across steps the stage test and the contract test then exercise).
Bounds: bit equality where the definition is exact (search, mask, count, correspondences, fitness); the derived
n * 2^-52 * majorant of registration_ref's docstring on the fp64 sums; 8 cond(A) 2^-52 |x| on the solve, whose x the step
writes behind the sums of its optional `moments` output; 1e-6 on R, T and 1e-5 (1 + max |Y|) on Xt, the bounds of the
existing ICP tests; 1e-5 on the recovered pose."""
import numpy as np
import pytest
import torch

import buffers
import registration_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

SHAPES = ((2500, 3000), (700, 1100), (300, 400))
P1, P2 = SHAPES[0]
SEED = 7
PAD = 9.0  # what padding rows hold in the raw batches: nothing may read it
POINT_ITERATIONS = 60
_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _batch(clutter):
    """(X (3,P1,3), Y (3,P2,3), normals, len_x, len_y, scenes): the base batch as numpy, padding rows = PAD"""
    def make():
        scenes = [ref.scene(SEED, a, b, clutter) for a, b in SHAPES]
        X, Y, Nr = (np.full((3, P, 3), PAD, np.float32) for P in (P1, P2, P2))
        for n, sc in enumerate(scenes):
            X[n, :len(sc.X)], Y[n, :len(sc.Y)], Nr[n, :len(sc.Y)] = sc.X, sc.Y, sc.normals
        return X, Y, Nr, np.array([a for a, _ in SHAPES]), np.array([b for _, b in SHAPES]), scenes
    return _once(("batch", clutter), make)


def _clouds(dev, clutter):
    from pytorch3d_pointops_amd.structures import Pointclouds

    *_, scenes = _batch(clutter)
    G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return (Pointclouds([G(sc.X) for sc in scenes]),
            Pointclouds([G(sc.Y) for sc in scenes], features={"normals": [G(sc.normals) for sc in scenes]}))


def _loop(clutter, estimation, n):
    """the checker's whole loop on cloud n of the base batch, once"""
    def make():
        sc = _batch(clutter)[5][n]
        return ref.icp(sc.X, sc.Y, len(sc.X), len(sc.Y), ref.R_MAX, estimation, sc.normals,
                       max_iterations=POINT_ITERATIONS if estimation == "point_to_point" else 30)
    return _once(("loop", clutter, estimation, n), make)


def _G(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _npy(t):
    return t.detach().cpu().numpy()


def _fields(r):
    """every tensor of a RegistrationResult, by name"""
    out = {k: getattr(r, k) for k in r._fields if k not in ("Xt", "history")}
    out["Xt"] = r.Xt if torch.is_tensor(r.Xt) else r.Xt.points_padded()
    out.update({"history." + k: getattr(r.history, k) for k in r.history._fields})
    return {k: _npy(v) for k, v in out.items()}


def _assert_bytes_equal(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def _state(dev, clutter, estimation, steps, **kw):
    from pytorch3d_pointops_amd import _C_registration

    X, Y, Nr, lx, ly, _ = _batch(clutter)
    t = _G(dev, X, Y, Nr, lx, ly)
    return _C_registration.RegistrationState(t[0], t[1], t[2], t[3], t[4], None, None, ref.R_MAX, estimation, steps,
                                             1e-6, 1e-6, **kw), t


def _search_family(monkeypatch, grid):
    """The base batch is below the size at which the K=1 search takes the grid by itself; POINTOPS_DEBUG
    registration_grid=1 (read by the library at call time) sends the step's search through it at any size."""
    if grid:
        monkeypatch.setenv("POINTOPS_DEBUG", "registration_grid=1")
    else:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)


# ------------------------------------------------------------------------------------------------ 1. stage by stage
@pytest.mark.parametrize("grid", [False, True], ids=["search-by-shape", "grid"])
@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
def test_every_stage_of_a_step_against_the_checker(dev, monkeypatch, estimation, grid):
    from pytorch3d_pointops_amd.functions import knn_points

    steps = 4
    _search_family(monkeypatch, grid)
    state, (Xd, Yd, Nd, lxd, lyd) = _state(dev, True, estimation, steps, want_moments=True)
    assert state.uses_grid == grid and state.reuse_grid == grid  # (the grid is built by step 0 and reused after it)
    # (the run asked for its search family once: the steps below and knn_points run without the knob)
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    X, Y, Nr, lx, ly, _ = _batch(True)
    ymax = float(np.abs(Y[Y != PAD]).max())
    Xt_before = X.copy()
    for n in range(3):
        Xt_before[n, lx[n]:] = 0
    R_acc, T_acc = [np.eye(3) for _ in range(3)], [np.zeros(3) for _ in range(3)]
    for i in range(steps):
        state.step(update=True)
        torch.cuda.synchronize()
        knn = knn_points(torch.from_numpy(Xt_before).to(dev), Yd, lxd, lyd, K=1)
        idx, d2 = _npy(state.idx), _npy(state.dists)
        assert np.array_equal(idx, _npy(knn.idx)[..., 0]), f"step {i}: idx differs from knn_points"
        assert d2.tobytes() == _npy(knn.dists)[..., 0].tobytes(), f"step {i}: d2 differs from knn_points"
        mom, st = _npy(state.moments), _npy(state.state)
        Rh, Th, fit, rmse = (_npy(t[i]) for t in (state.R, state.T, state.fitness, state.inlier_rmse))
        corr, num, status, its = (_npy(t) for t in (state.correspondences, state.num_correspondences, state.status,
                                                    state.iterations))
        Xt_after = _npy(state.Xt)
        for n in range(3):
            tag = f"step {i}, cloud {n}"
            mask, c, f, r, s = ref.evaluate(d2[n], lx[n], ly[n], ref.R_MAX)
            assert c >= 7, tag  # (the derived bound holds from 7 terms on)
            assert np.array_equal(corr[n], np.where(mask, idx[n], -1)) and num[n] == c and mom[n, 27] == c, tag
            assert np.float32(fit[n]).tobytes() == np.float32(f).tobytes(), tag
            assert abs(mom[n, 28] - s) <= c * ref.U52 * s, tag
            assert abs(float(rmse[n]) - float(r)) <= 2.0 ** -23 * float(r), tag
            assert status[n] == ref.RUNNING and its[n] == i + 1, tag  # (four steps cannot settle: see the certificate)
            if estimation == "point_to_plane":
                m = ref.plane_moments(Xt_before[n], Y[n], Nr[n], idx[n], mask)
                errA = np.abs(mom[n, :21] - ref.upper(m.A)) / (c * ref.U52 * ref.upper(m.abs_A))
                errb = np.abs(mom[n, 21:27] - m.b) / (c * ref.U52 * m.abs_b)
                print(f"{tag}: c = {c}, worst A error / bound = {errA.max():.3f}, b: {errb.max():.3f}")
                assert errA.max() <= 1 and errb.max() <= 1, tag
                A = np.zeros((6, 6))
                A[np.triu_indices(6)] = mom[n, :21]
                A = A + np.triu(A, 1).T
                x = np.linalg.solve(A, mom[n, 21:27])
                R_dev, T_dev = st[n, :9].reshape(3, 3), st[n, 9:12]
                x_dev = mom[n, 29:35]  # the device's own x
                bound = 8 * np.linalg.cond(A) * ref.U52 * np.linalg.norm(x)
                print(f"{tag}: cond(A) = {np.linalg.cond(A):.3g}, |x_dev - x| = {np.linalg.norm(x_dev - x):.3g}, "
                      f"bound = {bound:.3g}")
                assert np.linalg.norm(x_dev - x) <= bound, tag
                # and the state is that x composed onto the state before (the checker's compose, to fp64 rounding)
                R_own, T_own = ref.compose(R_acc[n], T_acc[n], ref.rotation_delta(*x_dev[:3]), m.c0, x_dev[3:])
                assert np.abs(R_dev - R_own).max() <= 4 * ref.U52 and \
                    np.abs(T_dev - T_own).max() <= 4 * ref.U52 * (1 + np.abs(T_acc[n]).max() + np.abs(m.c0).max()), tag
                R_want, T_want = ref.compose(R_acc[n], T_acc[n], ref.rotation_delta(*x[:3]), m.c0, x[3:])
            else:
                want, mag = ref.alignment_moments(X[n], Y[n], idx[n], mask)
                err = np.abs(mom[n, :24] - want) / np.maximum(c * ref.U52 * mag, 1e-300)
                print(f"{tag}: c = {c}, worst moment error / bound = {err.max():.3f}")
                assert err.max() <= 1 and not mom[n, 24:27].any() and not mom[n, 29:].any(), tag
                R_want, T_want = ref.kabsch(*ref.point_moments(X[n], Y[n], idx[n], mask))
                R_dev, T_dev = st[n, :9].reshape(3, 3), st[n, 9:12]
            assert np.abs(R_dev - R_want).max() <= 1e-6 and np.abs(T_dev - T_want).max() <= 1e-6, tag
            assert np.array_equal(Rh[n], R_dev.astype(np.float32)) and np.array_equal(Th[n], T_dev.astype(np.float32)), tag
            assert np.abs(Xt_after[n] - ref.apply(X[n], R_want, T_want, lx[n])).max() <= 1e-5 * (1 + ymax), tag
            assert Xt_after[n].tobytes() == ref.apply(X[n], R_dev, T_dev, lx[n]).tobytes(), tag  # (the fp32 arithmetic)
            R_acc[n], T_acc[n] = R_dev.copy(), T_dev.copy()
        Xt_before = Xt_after.copy()
    assert int(state.all_frozen.item()) == 0


# ------------------------------------------------------------------------------------------------ 2. the fixed point
@pytest.mark.parametrize("clutter", [False, True], ids=["clean", "clutter"])
@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
def test_the_true_pose_is_recovered(dev, estimation, clutter):
    from pytorch3d_pointops_amd.functions import registration_icp

    src, tgt = _clouds(dev, clutter)
    max_iterations = POINT_ITERATIONS if estimation == "point_to_point" else 30
    r = registration_icp(src, tgt, ref.R_MAX, estimation=estimation, max_iterations=max_iterations)
    got = _fields(r)
    scenes = _batch(clutter)[5]
    for n, sc in enumerate(scenes):
        want = _loop(clutter, estimation, n)
        eR, eT = ref.pose_error(got["R"][n], got["T"][n], sc)
        print(f"{estimation} clutter={clutter} cloud {n}: {got['iterations'][n]} updates on the GPU, "
              f"{want.iterations} in the checker; |R-R*| = {eR:.2e}, |T-T*| = {eT:.2e}")
        assert eR <= 1e-5 and eT <= 1e-5
        assert np.linalg.norm(got["R"][n] - want.R) <= 1e-5 and np.linalg.norm(got["T"][n] - want.T) <= 1e-5
        assert got["status"][n] == ref.CONVERGED and got["converged"][n] and got["iterations"][n] <= max_iterations
        assert float(got["fitness"][n]) == sc.overlap / len(sc.X) and got["num_correspondences"][n] == sc.overlap
        assert float(got["inlier_rmse"][n]) < 1e-6
    assert got["history.R"].shape == (max_iterations + 1, 3, 3, 3)
    assert np.array_equal(got["history.R"][-1], got["R"]) and np.array_equal(got["history.fitness"][-1], got["fitness"])


# ------------------------------------------------------------------------------------------------ 3. the gap
def test_the_untrimmed_icp_is_dragged_off_where_this_one_is_not(dev):
    from pytorch3d_pointops_amd.functions import iterative_closest_point, registration_icp

    src, tgt = _clouds(dev, True)
    old = iterative_closest_point(src, tgt, max_iterations=40)
    new = registration_icp(src, tgt, ref.R_MAX)
    for n, sc in enumerate(_batch(True)[5]):
        e_old = ref.pose_error(_npy(old.RTs.R)[n], _npy(old.RTs.T)[n], sc)[0]
        e_new = max(ref.pose_error(_npy(new.R)[n], _npy(new.T)[n], sc))
        print(f"cloud {n}: |R-R*| = {e_old:.2f} untrimmed, {e_new:.2e} trimmed point-to-plane")
        assert e_old > 0.1 and e_new <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. evaluation
@pytest.mark.parametrize("pose", ["identity", "true", "registered"])
def test_evaluate_registration_equals_the_checker(dev, pose):
    from pytorch3d_pointops_amd.functions import evaluate_registration, registration_icp

    src, tgt = _clouds(dev, True)
    scenes = _batch(True)[5]
    if pose == "identity":
        transform, R, T = None, [np.eye(3)] * 3, [np.zeros(3)] * 3
    elif pose == "true":
        R, T = [sc.R_true.astype(np.float32) for sc in scenes], [sc.T_true.astype(np.float32) for sc in scenes]
        transform = tuple(_G(dev, np.stack(R), np.stack(T)))
    else:
        reg = registration_icp(src, tgt, ref.R_MAX)
        transform, R, T = (reg.R, reg.T), _npy(reg.R), _npy(reg.T)
    got = _fields(evaluate_registration(src, tgt, ref.R_MAX, transform))
    for n, sc in enumerate(scenes):
        a, b = len(sc.X), len(sc.Y)
        Xt = ref.apply(sc.X, R[n], T[n], a)
        idx, d2 = ref.nearest(Xt, sc.Y, a, b)
        mask, c, f, r, _ = ref.evaluate(d2, a, b, ref.R_MAX)
        assert got["Xt"][n, :a].tobytes() == Xt.tobytes() and not got["Xt"][n, a:].any()
        assert np.array_equal(got["correspondences"][n, :a], np.where(mask, idx, -1))
        assert (got["correspondences"][n, a:] == -1).all() and got["num_correspondences"][n] == c
        assert np.float32(got["fitness"][n]).tobytes() == np.float32(f).tobytes()
        assert abs(float(got["inlier_rmse"][n]) - float(r)) <= 2.0 ** -23 * float(r)
        if pose != "identity":
            assert float(f) == sc.overlap / a  # the overlap share, exactly
        assert got["status"][n] == ref.RUNNING and got["iterations"][n] == 0 and not got["converged"][n]
        assert np.array_equal(got["R"][n], np.asarray(R[n], np.float32))
        assert np.array_equal(got["T"][n], np.asarray(T[n], np.float32))
    assert got["history.R"].shape[0] == 1


# ------------------------------------------------------------------------------------------------ 5. degenerate inputs
def _degenerate_batch():
    """(X (6,300,3), Y (6,400,3), normals, len_x, len_y, scene 0): cloud 0 the experiment, cloud 1 a planar target,
    clouds 2-4 with 0, 1 and 5 source rows, cloud 5 without target rows"""
    a, b = SHAPES[2]
    sc, pl = ref.scene(SEED, a, b, True), ref.planar_scene(SEED, a, b)
    X = np.stack([sc.X, pl.X] + [sc.X] * 4)
    Y = np.stack([sc.Y, pl.Y] + [sc.Y] * 4)
    Nr = np.stack([sc.normals, pl.normals] + [sc.normals] * 4)
    return X, Y, Nr, np.array([a, a, 0, 1, 5, a]), np.array([b, b, b, b, b, 0]), sc


@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
def test_degenerate_clouds_freeze_and_block_nobody(dev, estimation):
    from pytorch3d_pointops_amd.functions import registration_icp
    from pytorch3d_pointops_amd.structures import Pointclouds

    X, Y, Nr, lx, ly, sc = _degenerate_batch()
    (Xd, Yd, Nd) = _G(dev, X, Y, Nr)
    src = Pointclouds([Xd[n, :lx[n]] for n in range(6)])
    tgt = Pointclouds([Yd[n, :ly[n]] for n in range(6)], features={"normals": [Nd[n, :ly[n]] for n in range(6)]})
    R0 = np.stack([ref.rotation([0, 0, 1], 0.01).astype(np.float32)] * 6)
    T0 = np.stack([np.array([0.002, -0.001, 0.003], np.float32)] * 6)
    r = registration_icp(src, tgt, ref.R_MAX, tuple(_G(dev, R0, T0)), estimation=estimation,
                         max_iterations=POINT_ITERATIONS)
    got = _fields(r)
    for v in got.values():
        assert np.isfinite(v.astype(np.float64)).all()
    frozen = [2, 3, 5] + ([1, 4] if estimation == "point_to_plane" else [])  # (5 rows are enough for point to point)
    for n in frozen:
        assert got["status"][n] == ref.DEGENERATE and got["iterations"][n] == 0 and not got["converged"][n], n
        assert got["R"][n].tobytes() == R0[n].tobytes() and got["T"][n].tobytes() == T0[n].tobytes(), n
        assert (got["history.R"][:, n] == R0[n]).all() and (got["history.T"][:, n] == T0[n]).all(), n
    assert got["num_correspondences"][2] == 0 and got["num_correspondences"][5] == 0
    assert (got["correspondences"][2] == -1).all() and (got["correspondences"][5] == -1).all()
    assert got["fitness"][2] == 0 and got["fitness"][5] == 0 and got["inlier_rmse"][5] == 0
    if estimation == "point_to_plane":
        assert got["num_correspondences"][1] >= 6  # refused by the pivot rule, not by the count
    # the experiment beside them converges as it does alone
    assert got["status"][0] == ref.CONVERGED and max(ref.pose_error(got["R"][0], got["T"][0], sc)) <= 1e-5
    # a threshold so small that nothing matches
    tiny = _fields(registration_icp(src, tgt, 1e-7, tuple(_G(dev, R0, T0)), estimation=estimation))
    assert (tiny["status"] == ref.DEGENERATE).all() and not tiny["num_correspondences"].any()
    assert tiny["R"].tobytes() == R0.tobytes() and tiny["T"].tobytes() == T0.tobytes()
    assert (tiny["correspondences"] == -1).all() and not tiny["fitness"].any() and not tiny["inlier_rmse"].any()
    for v in tiny.values():
        assert np.isfinite(v.astype(np.float64)).all()


# ------------------------------------------------------------------------------------------------ 6. reproducibility
@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
def test_bytes_are_reproducible_and_independent_of_the_batch(dev, estimation):
    from pytorch3d_pointops_amd import _C_registration
    from pytorch3d_pointops_amd.functions import registration_icp

    src, tgt = _clouds(dev, True)
    kw = dict(estimation=estimation, max_iterations=12)
    first = _fields(registration_icp(src, tgt, ref.R_MAX, **kw))
    _assert_bytes_equal(_fields(registration_icp(src, tgt, ref.R_MAX, **kw)), first, "second call")
    _assert_bytes_equal(_fields(registration_icp(src, tgt, ref.R_MAX, check_every=0, **kw)), first, "check_every=0")
    _assert_bytes_equal(_fields(registration_icp(src, tgt, ref.R_MAX, check_every=5, **kw)), first, "check_every=5")
    # Each cloud ALONE, N = 1, at the batch's padded widths: the launch is (nb, 1) and the search chooses its family
    # for one cloud.  Through the state class, which takes the padded rows and explicit lengths as they are.
    X, Y, Nr, lx, ly, _ = _batch(True)

    def run(sl):
        t = _G(dev, X[sl], Y[sl], Nr[sl], lx[sl], ly[sl])
        st = _C_registration.RegistrationState(*t, None, None, ref.R_MAX, estimation, 13, 1e-6, 1e-6)
        for i in range(13):
            st.step(update=i < 12)
        names = ("Xt", "state", "status", "iterations", "idx", "dists", "correspondences", "num_correspondences", "R",
                 "T", "fitness", "inlier_rmse")
        return {k: _npy(getattr(st, k)) for k in names}

    batch = run(slice(0, 3))
    for k in ("R", "T", "fitness", "inlier_rmse"):  # (the same run as the public call's)
        assert batch[k].tobytes() == first["history." + k].tobytes(), k
    assert batch["status"].tobytes() == first["status"].tobytes()
    history = ("R", "T", "fitness", "inlier_rmse")
    for n in range(3):
        alone = run(slice(n, n + 1))
        _assert_bytes_equal(alone, {k: np.take(v, [n], axis=1 if k in history else 0) for k, v in batch.items()},
                            f"cloud {n} alone")


# ------------------------------------------------------------------------------------------------ 7. the buffer contract
def _contract_run(dev, clutter):
    from pytorch3d_pointops_amd.functions import registration_icp

    src, tgt = _clouds(dev, clutter)
    src.points_padded(), tgt.points_padded(), tgt.get_features_padded("normals")  # (padded once, outside the contract)
    return lambda: registration_icp(src, tgt, ref.R_MAX, max_iterations=5, check_every=0), (src, tgt)


@pytest.mark.parametrize("fill", buffers.FILLS)
def test_buffer_contract(dev, monkeypatch, fill):
    _search_family(monkeypatch, True)  # (the grid: the search has a workspace to be short of)
    run, (src, tgt) = _contract_run(dev, True)
    sibling, _ = _contract_run(dev, False)
    plain = _once("contract plain", lambda: _fields(run()))
    with buffers.contract(monkeypatch, fill, short_workspace="short" if fill == "ones" else False,
                          prototypes=declared_prototypes()) as c:
        c.sibling(sibling)
        c.watch(source=src.points_padded(), target=tgt.points_padded(), normals=tgt.get_features_padded("normals"),
                len_x=src.num_points_per_cloud(), len_y=tgt.num_points_per_cloud())
        got = _fields(run())
    c.assert_all_clear()
    assert c.inputs_checked > 0
    _assert_bytes_equal(got, plain, f"under the {fill} fill")  # (an unwritten element would show)
    if fill == "ones":  # both workspaces, one byte short and null: POINTOPS_EWORKSPACE, nothing written
        rejected = {(name, label) for name, _, label in c.rejections}
        assert {("pointops_registration_step", "short"), ("pointops_registration_step", "null")} <= rejected
        assert len({at for name, at, _ in c.rejections if name == "pointops_registration_step"}) == 2
    key = "contract bytes"
    bytes_ = c.output_bytes()
    if key in _CACHE:  # every output buffer, padding included, holds the same bytes under every fill
        assert [n for n, _ in bytes_] == [n for n, _ in _CACHE[key]]
        for (name, a), (_, b) in zip(bytes_, _CACHE[key]):
            assert np.array_equal(a, b), (fill, name)
    else:
        _CACHE[key] = bytes_


# ------------------------------------------------------------------------------------------------ 8. streams and graphs
def test_side_stream(dev):
    from pytorch3d_pointops_amd.functions import registration_icp

    src, tgt = _clouds(dev, True)
    want = _fields(registration_icp(src, tgt, ref.R_MAX, max_iterations=8))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = registration_icp(src, tgt, ref.R_MAX, max_iterations=8)
    side.synchronize()
    _assert_bytes_equal(_fields(got), want, "side stream")


def test_the_whole_run_replays_from_a_graph(dev):
    from pytorch3d_pointops_amd import graphs
    from pytorch3d_pointops_amd.functions import registration_icp

    sc = _batch(True)[5][2]  # (300, 400), full lengths: padded tensors in
    X, Y, Nr = _G(dev, sc.X[None], sc.Y[None], sc.normals[None])
    names = ("R", "T", "fitness", "inlier_rmse", "num_correspondences", "correspondences", "iterations", "status", "Xt")

    def fn(x, y, nr):
        r = registration_icp(x, y, ref.R_MAX, target_normals=nr, max_iterations=8, check_every=0)
        return tuple(getattr(r, k) for k in names) + tuple(r.history)

    eager = [_npy(t).copy() for t in fn(X, Y, Nr)]
    assert max(ref.pose_error(eager[0][0], eager[1][0], sc)) <= 1e-5
    g = graphs.capture(fn, (X, Y, Nr))
    for replay in range(2):
        out = g()
        torch.cuda.synchronize()
        for name, a, b in zip(names + ("hR", "hT", "hf", "hr"), out, eager):
            assert _npy(a).tobytes() == b.tobytes(), f"replay {replay}: {name} differs from eager"


# ------------------------------------------------------------------------------------------------ 9. containers
def test_pointclouds_in_and_out(dev):
    from pytorch3d_pointops_amd.functions import SimilarityTransform, registration_icp
    from pytorch3d_pointops_amd.structures import Pointclouds

    src, tgt = _clouds(dev, True)
    scenes = _batch(True)[5]
    R0 = np.stack([ref.rotation([1, 1, 0], 0.03).astype(np.float32)] * 3)
    T0 = np.stack([np.array([0.01, 0.0, -0.01], np.float32)] * 3)
    R0d, T0d = _G(dev, R0, T0)
    init = SimilarityTransform(R0d, T0d, torch.ones(3, device=dev))
    r = src.registration_icp(tgt, ref.R_MAX, init_transform=init)
    assert isinstance(r.Xt, Pointclouds) and r.Xt.num_points_per_cloud().tolist() == [a for a, _ in SHAPES]
    same = registration_icp(src, tgt, ref.R_MAX, init, target_normals=tgt.get_features_padded("normals"))
    _assert_bytes_equal(_fields(r), _fields(same), "method against function")
    got = _fields(r)
    # honoured: the evaluation of the initial transform is what the run's first step saw
    first = _fields(src.evaluate_registration(tgt, ref.R_MAX, init))
    assert first["R"].tobytes() == R0.tobytes() and first["T"].tobytes() == T0.tobytes()
    one = _fields(registration_icp(src, tgt, ref.R_MAX, init, max_iterations=1))
    assert one["history.fitness"][0].tobytes() == first["fitness"].tobytes()
    assert one["history.inlier_rmse"][0].tobytes() == first["inlier_rmse"].tobytes()
    for n, sc in enumerate(scenes):
        assert max(ref.pose_error(got["R"][n], got["T"][n], sc)) <= 1e-5
        a = len(sc.X)
        assert np.abs(got["Xt"][n, :a] - ref.apply(sc.X, got["R"][n], got["T"][n], a)).max() == 0
    ev = src.evaluate_registration(tgt, ref.R_MAX, (r.R, r.T))
    assert torch.equal(ev.fitness, r.fitness) and torch.equal(ev.correspondences, r.correspondences)
    with pytest.raises(ValueError, match="estimate_pointcloud_normals"):
        src.registration_icp(Pointclouds(tgt.points_list()), ref.R_MAX)
    with pytest.raises(RuntimeError, match="65536"):
        big = torch.zeros((65536, 1, 3), device=dev)
        registration_icp(big, big, 0.1, estimation="point_to_point")
