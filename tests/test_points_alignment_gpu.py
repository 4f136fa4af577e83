"""GPU suite of the registration feature (functions/points_alignment.py, csrc/points_alignment.hip) against the
float64 checker (tests/points_alignment_ref.py) fed the same fp32 inputs.

Alignment bars (where the checker's singular values satisfy sigma_{d-1} + sigma_d >= 1e-3 sigma_1):
max|R - R64| <= 1e-5, |T - T64| <= 1e-5 (1 + max|Y|), |s - s64| <= 1e-5 s64.  Everywhere: finite, R^T R = I to 1e-5,
det R = +1 unless reflections are allowed.  Gradients: <= 1e-3 of the largest reference gradient entry.
ICP trajectories are not compared step by step (a float32 and a float64 run may pick different neighbours on
near-ties): one iteration is checked as an exact composition, the fixed point against the truth and the checker,
and the history against the checker's alignment on the package's own neighbour tables."""
import numpy as np
import pytest
import torch

import points_alignment_ref as ref
from pytorch3d_pointops_amd import synth

pytestmark = pytest.mark.gpu


def _api():
    from pytorch3d_pointops_amd.functions import points_alignment

    return points_alignment


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cloud(name, N, P, seed):
    return torch.from_numpy(np.stack([synth.distribution(name, seed + n, P) for n in range(N)]))


def _moved(X, seed, noise=0.01, mirror=False):
    """Y = s X R + T + noise for random per-cloud similarity transforms (fp32 result)."""
    N = X.shape[0]
    g = _gen(seed)
    axes = torch.randn((N, 3), generator=g, dtype=torch.float64)
    angles = (torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * 3.0
    R = torch.stack([ref.rotation(axes[n], angles[n]) for n in range(N)])
    if mirror:
        R = R * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)
    T = torch.rand((N, 3), generator=g, dtype=torch.float64) - 0.5
    s = 0.7 + 0.6 * torch.rand((N,), generator=g, dtype=torch.float64)
    Y = ref.apply(X, R, T, s) + noise * torch.randn(X.shape, generator=g, dtype=torch.float64)
    return Y.float()


def _check_alignment(got, want, ymax, allow_reflection, what=""):
    """got = (R, T, s) fp32 tensors, want = the checker's (R, T, s, S)."""
    R, T, s = (t.detach().double().cpu() for t in got[:3])
    R64, T64, s64, S = (t.detach() for t in want)
    d = R.shape[-1]
    assert bool(torch.isfinite(R).all() and torch.isfinite(T).all() and torch.isfinite(s).all()), what
    orth = (R.transpose(1, 2) @ R - torch.eye(d, dtype=torch.float64)).abs().amax((1, 2))
    print(f"{what}: max |R^T R - I| = {float(orth.max()):.3e}")
    assert float(orth.max()) <= 1e-5, what
    if not allow_reflection:
        assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-5, what
    ok = ref.well_determined(S)
    if allow_reflection:
        # a rank-deficient C has two optimal R once reflections are allowed (mirror images across the data's plane)
        # and the checker's own pick follows LAPACK's sign of a null vector: such clouds keep the orthogonality check
        ok = ok & (S[:, -1] > 1e-9 * S[:, 0])
    if bool(ok.any()):
        eR = (R - R64).abs().amax((1, 2))[ok]
        eT = (T - T64).abs().amax(1)[ok]
        es = ((s - s64).abs() - 1e-5 * s64.abs())[ok]  # |s - s64| <= 1e-5 s64, also where both are 0
        print(f"{what}: well determined {int(ok.sum())}/{len(ok)}  max|dR| = {float(eR.max()):.3e}  "
              f"max|dT| = {float(eT.max()):.3e}  max(|ds| - 1e-5 s) = {float(es.max()):.3e}")
        assert float(eR.max()) <= 1e-5, what
        assert float(eT.max()) <= 1e-5 * (1 + ymax), what
        assert float(es.max()) <= 0.0, what
    return ok


FLAGS = [(False, False), (True, False), (False, True), (True, True)]
ALIGN_CASES = [("uniform", 1, 200000), ("sphere", 4, 5000), ("aniso_100", 3, 700), ("uniform", 64, 5),
               ("uniform", 7, 1000)]


@pytest.mark.parametrize("name,N,P", ALIGN_CASES)
def test_alignment_against_float64(dev, name, N, P):
    cpa = _api().corresponding_points_alignment
    X = _cloud(name, N, P, 5000 + P)
    g = _gen(P)
    weights = {"none": None, "random": torch.rand((N, P), generator=g),
               "binary": (torch.rand((N, P), generator=g) < 0.7).float()}
    for mirror in (False, True):
        Y = _moved(X, 77 + P, mirror=mirror)
        ymax = float(Y.abs().max())
        for estimate_scale, allow_reflection in FLAGS:
            for wname, w in weights.items():
                got = cpa(X.to(dev), Y.to(dev), None if w is None else w.to(dev), estimate_scale, allow_reflection)
                want = ref.alignment(X, Y, w, estimate_scale, allow_reflection)
                ok = _check_alignment(got, want, ymax, allow_reflection,
                                      f"{name} N={N} P={P} mirror={mirror} scale={estimate_scale} "
                                      f"refl={allow_reflection} w={wname}")
                if P >= 100:  # full-rank noisy clouds: every cloud is held to the accuracy bars
                    assert bool(ok.all())


def test_alignment_ragged_and_degenerate(dev):
    """Lengths 0, 1, 2, 3 next to ordinary ones, collinear and coincident clouds: finite proper rotations everywhere,
    the accuracy bars where the rotation is determined, and the identity for an all-zero cross-covariance."""
    from pytorch3d_pointops_amd.structures import Pointclouds

    cpa = _api().corresponding_points_alignment
    P = 300
    lens = [300, 0, 1, 2, 3, 50, 299, 4]
    N = len(lens)
    X = _cloud("uniform", N, P, 6100)
    Y = _moved(X, 6200)
    line = torch.linspace(0, 1, P)[:, None] * torch.tensor([0.3, -0.5, 0.8])
    Xd = torch.stack([line + 0.1, torch.full((P, 3), 0.25), X[0], torch.zeros(P, 3)])
    Yd = torch.stack([line @ ref.rotation([0.0, 0.0, 1.0], 0.4).float() - 0.2, torch.full((P, 3), -0.5), X[0] * 0 + 0.5,
                      torch.zeros(P, 3)])
    mask = ref.valid_mask(lens, P).float()
    for estimate_scale, allow_reflection in FLAGS:
        pcx = Pointclouds([X[n, :lens[n]].to(dev) for n in range(N)])
        pcy = Pointclouds([Y[n, :lens[n]].to(dev) for n in range(N)])
        with pytest.warns(UserWarning):
            got = cpa(pcx, pcy, None, estimate_scale, allow_reflection)
        want = ref.alignment(X, Y, mask, estimate_scale, allow_reflection)
        ok = _check_alignment(got, want, float(Y.abs().max()), allow_reflection, f"ragged {estimate_scale}")
        # length 2 leaves the rotation about the segment free; lengths 0 and 1 (C = 0) must give the identity
        assert bool(ok[0]) and bool(ok[5:].all()) and not bool(ok[3])
        assert torch.equal(got.R[2].cpu(), torch.eye(3))
        assert torch.equal(got.R[1].cpu(), torch.eye(3))  # the empty cloud
        w = torch.rand((N, P), generator=_gen(3)) * mask  # weights through the container, as a list
        got = cpa(pcx, pcy, [w[n, :lens[n]].to(dev) for n in range(N)], estimate_scale, allow_reflection)
        _check_alignment(got, ref.alignment(X, Y, w, estimate_scale, allow_reflection), float(Y.abs().max()),
                         allow_reflection, f"ragged weighted {estimate_scale}")
        with pytest.warns(UserWarning, match="low rank"):
            got = cpa(Xd.to(dev), Yd.to(dev), None, estimate_scale, allow_reflection)
        _check_alignment(got, ref.alignment(Xd, Yd, None, estimate_scale, allow_reflection), 1.0, allow_reflection,
                         f"degenerate {estimate_scale}")
        assert torch.equal(got.R[1:].cpu(), torch.eye(3).expand(3, 3, 3))  # coincident / constant target / zeros
    # a cloud far from the origin: the pivot keeps the fp64 sums free of cancellation
    far = X[:2] * 0.01 + 1000.0
    Yf = _moved(far, 6300, noise=1e-4)
    got = cpa(far.to(dev), Yf.to(dev))
    _check_alignment(got, ref.alignment(far, Yf), float(Yf.abs().max()), False, "far from the origin")


def test_alignment_cloud_with_all_zero_weights(dev):
    """A cloud whose rows hold points but whose weights are all zero (a mask that leaves nothing): by the definition
    W = eps, the means and C are 0, so R = I and T = 0 exactly (s = 1, or 0 / eps = 0 with estimate_scale) -- the pivots (row 0 of X and of Y) must not leak
    into T -- and the clouds next to it keep the bits they have without it."""
    cpa = _api().corresponding_points_alignment
    X = _cloud("uniform", 3, 50, 6400) + 0.5
    Y = _moved(X, 6401)
    w = torch.rand((3, 50), generator=_gen(6402)) + 0.1
    w[1] = 0.0
    for estimate_scale, allow_reflection in FLAGS:
        got = cpa(X.to(dev), Y.to(dev), w.to(dev), estimate_scale, allow_reflection)
        assert torch.equal(got.R[1].cpu(), torch.eye(3)) and torch.equal(got.T[1].cpu(), torch.zeros(3))
        assert float(got.s[1]) == (0.0 if estimate_scale else 1.0)  # tr(E S) / max(0, eps) = 0
        _check_alignment(got, ref.alignment(X, Y, w, estimate_scale, allow_reflection), float(Y.abs().max()),
                         allow_reflection, f"zero weights {estimate_scale} {allow_reflection}")
        alone = cpa(X[[0, 2]].to(dev), Y[[0, 2]].to(dev), w[[0, 2]].to(dev), estimate_scale, allow_reflection)
        for u, v in zip(got, alone):
            assert torch.equal(u[[0, 2]], v)


def test_alignment_d2(dev):
    cpa = _api().corresponding_points_alignment
    g = _gen(8)
    X = torch.rand((5, 400, 2), generator=g)
    c, s_ = np.cos(0.9), np.sin(0.9)
    Y = 1.2 * X @ torch.tensor([[c, s_], [-s_, c]], dtype=torch.float32) + 0.3 + 0.01 * torch.randn(X.shape, generator=g)
    for estimate_scale, allow_reflection in FLAGS:
        got = cpa(X.to(dev), Y.to(dev), None, estimate_scale, allow_reflection)
        ok = _check_alignment(got, ref.alignment(X, Y, None, estimate_scale, allow_reflection),
                              float(Y.abs().max()), allow_reflection, "d=2")
        assert bool(ok.all())


def test_alignment_reproducible(dev):
    cpa = _api().corresponding_points_alignment
    X = _cloud("uniform", 3, 70000, 6400).to(dev)
    Y = _moved(X.cpu(), 6401).to(dev)
    w = torch.rand((3, 70000), generator=_gen(6402)).to(dev)
    a, b = cpa(X, Y, w, True), cpa(X, Y, w, True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("estimate_scale", [False, True])
def test_alignment_gradients_against_float64(dev, estimate_scale):
    from pytorch3d_pointops_amd.structures import Pointclouds

    cpa = _api().corresponding_points_alignment
    N, P = 3, 400
    lens = [400, 333, 57]
    X = _cloud("uniform", N, P, 6500)
    Y = _moved(X, 6501, noise=0.05)
    mask = ref.valid_mask(lens, P)
    w = (0.2 + torch.rand((N, P), generator=_gen(6502))) * mask
    g = _gen(6503)
    gR, gT, gs = (torch.randn(sh, generator=g, dtype=torch.float64) for sh in ((N, 3, 3), (N, 3), (N,)))

    def loss(R, T, s):
        dev_ = R.device
        return (R * gR.to(dev_, R.dtype)).sum() + (T * gT.to(dev_, T.dtype)).sum() + (s * gs.to(dev_, s.dtype)).sum()

    leaves64 = [t.double().clone().requires_grad_(True) for t in (X, Y, w)]
    R64, T64, s64, S = ref.alignment(*leaves64, estimate_scale=estimate_scale)
    assert bool(ref.well_determined(S).all())
    want = torch.autograd.grad(loss(R64, T64, s64), leaves64)

    leaves = [t.to(dev).clone().requires_grad_(True) for t in (X, Y, w)]
    got = torch.autograd.grad(loss(*cpa(*leaves, estimate_scale=estimate_scale)), leaves)
    for name, u, v in zip("XYw", got, want):
        scale = float(v.abs().max())
        err = float((u.double().cpu() - v).abs().max())
        print(f"grad {name}: max err {err:.3e}, largest reference entry {scale:.3e}")
        assert bool(torch.isfinite(u).all()) and scale > 0 and err <= 1e-3 * scale
    # containers, default weights: only X and Y are differentiated; padded rows get zero
    lx = [X[n, :lens[n]].to(dev).clone().requires_grad_(True) for n in range(N)]
    ly = [Y[n, :lens[n]].to(dev).clone().requires_grad_(True) for n in range(N)]
    got = torch.autograd.grad(loss(*cpa(Pointclouds(lx), Pointclouds(ly), estimate_scale=estimate_scale)), lx + ly)
    l64 = [t.double().clone().requires_grad_(True) for t in (X, Y)]
    R64, T64, s64, _ = ref.alignment(*l64, mask.double(), estimate_scale=estimate_scale)
    want = torch.autograd.grad(loss(R64, T64, s64), l64)
    for k in range(2):
        scale = float(want[k].abs().max())
        for n in range(N):
            err = float((got[k * N + n].double().cpu() - want[k][n, :lens[n]]).abs().max())
            assert err <= 1e-3 * scale


def test_alignment_graph_capture(dev):
    from pytorch3d_pointops_amd import graphs

    cpa = _api().corresponding_points_alignment

    def fn(a, b):
        return tuple(cpa(a, b, estimate_scale=True))

    X = _cloud("uniform", 2, 3000, 6600)
    a, b = X.to(dev), _moved(X, 6601).to(dev)
    step = graphs.capture(fn, (a, b))
    assert all(torch.equal(u, v) for u, v in zip(step(), fn(a, b)))
    X2 = _cloud("sphere", 2, 3000, 6602)
    a2, b2 = X2.to(dev), _moved(X2, 6603).to(dev)
    want = fn(a2, b2)
    assert all(torch.equal(u, v) for u, v in zip(step(a2, b2), want))


# ------------------------------------------------------------------------------------------------------ ICP
def _subset_setup(seed, sizes, noise=0.0, similarity=False, motion=1.0):
    """Y uniform in the unit cube; X a random subset of Y (all of Y for `similarity`) moved so that s X R + T = Y rows.
    sizes: [(rows of X, rows of Y)] per cloud; `motion` scales the rotation angle and the translation.  Returns padded fp32 X, Y, lengths and the true fp64 (R, T, s)."""
    g = _gen(seed)
    N = len(sizes)
    P1, P2 = max(a for a, _ in sizes), max(b for _, b in sizes)
    X, Y = torch.zeros((N, P1, 3)), torch.zeros((N, P2, 3))
    Rs, Ts, ss = [], [], []
    for n, (a, b) in enumerate(sizes):
        y = torch.rand((b, 3), generator=g, dtype=torch.float64)
        axis = torch.randn(3, generator=g, dtype=torch.float64)
        if similarity:
            angle = 0.04 + 0.06 * float(torch.rand((), generator=g))
            s = 0.9 + 0.2 * float(torch.rand((), generator=g))
        else:
            angle = 0.10 + 0.08 * float(torch.rand((), generator=g))
            s = 1.0
        R = ref.rotation(axis, motion * angle)
        T = motion * 0.03 * (torch.randn(3, generator=g, dtype=torch.float64) / 3 ** 0.5)
        pick = torch.randperm(b, generator=g)[:a] if a < b else torch.arange(b)
        x = ((y[pick] - T) @ R.T) / s
        x = x + noise * torch.randn(x.shape, generator=g, dtype=torch.float64)
        X[n, :a], Y[n, :b] = x.float(), y.float()
        Rs.append(R), Ts.append(T), ss.append(s)
    lx = torch.tensor([a for a, _ in sizes])
    ly = torch.tensor([b for _, b in sizes])
    return X, Y, lx, ly, (torch.stack(Rs), torch.stack(Ts), torch.tensor(ss, dtype=torch.float64))


def _pcs(X, Y, lx, ly, dev):
    from pytorch3d_pointops_amd.structures import Pointclouds

    return (Pointclouds([X[n, :int(lx[n])].to(dev) for n in range(len(lx))]),
            Pointclouds([Y[n, :int(ly[n])].to(dev) for n in range(len(ly))]))


SUBSET_SIZES = [(2000, 3000), (1500, 2600), (1200, 3000)]


def test_icp_one_iteration_is_exact_composition(dev):
    from pytorch3d_pointops_amd.functions import knn_points

    icp = _api().iterative_closest_point
    X, Y, lx, ly, _ = _subset_setup(7000, SUBSET_SIZES)
    pcx, pcy = _pcs(X, Y, lx, ly, dev)
    for estimate_scale in (False, True):
        sol = icp(pcx, pcy, max_iterations=1, estimate_scale=estimate_scale)
        assert len(sol.t_history) == 1 and sol.converged is False
        idx = knn_points(pcx.points_padded(), pcy.points_padded(), lx.to(dev), ly.to(dev), K=1).idx[..., 0].cpu()
        mask = ref.valid_mask(lx, X.shape[1]).double()
        Ynn = ref.gather(Y.double(), idx)
        want = ref.alignment(X, Ynn, mask, estimate_scale)
        ymax = float(Y.abs().max())
        _check_alignment(sol.t_history[0], want, ymax, False, "one iteration")
        assert all(torch.equal(u, v) for u, v in zip(sol.RTs, sol.t_history[0]))
        Xt64 = ref.apply(X, *want[:3]) * mask[..., None]
        assert float((sol.Xt.points_padded().double().cpu() - Xt64).abs().max()) <= 1e-5 * (1 + ymax)
        rmse64 = ((((Xt64 - Ynn) ** 2).sum(2) * mask).sum(1) / lx.double()).sqrt()
        assert float((sol.rmse.double().cpu() - rmse64).abs().max()) <= 1e-5 * (1 + ymax)


@pytest.mark.parametrize("sizes,noise", [(SUBSET_SIZES, 0.0), (SUBSET_SIZES, 0.002)])
def test_icp_fixed_point(dev, sizes, noise):
    icp = _api().iterative_closest_point
    X, Y, lx, ly, (Rt, Tt, _) = _subset_setup(7100 + len(sizes), sizes, noise=noise)
    pcx, pcy = _pcs(X, Y, lx, ly, dev)
    sol = icp(pcx, pcy)
    want = ref.icp(X, Y, lx, ly)
    print(f"sizes {sizes} noise {noise}: {len(sol.t_history)} iterations fused, {want.iterations} float64 checker; "
          f"rmse {sol.rmse.tolist()}")
    assert sol.converged is True and want.converged
    assert len(sol.t_history) <= 100
    R, T = sol.RTs.R.double().cpu(), sol.RTs.T.double().cpu()
    print(f"  |R - checker| = {float((R - want.R).abs().max()):.3e}  |T - checker| = "
          f"{float((T - want.T).abs().max()):.3e}  |R - truth| = {float((R - Rt).abs().max()):.3e}")
    assert float((R - want.R).abs().max()) <= 1e-5 and float((T - want.T).abs().max()) <= 1e-5
    rmse = sol.rmse.double().cpu()
    if noise == 0.0:
        assert float((R - Rt).abs().max()) <= 1e-5 and float((T - Tt).abs().max()) <= 1e-5
        assert float(rmse.max()) <= 1e-5
    else:
        assert float(((rmse - want.rmse).abs() / want.rmse).max()) <= 1e-5
    assert torch.equal(sol.RTs.s.cpu(), torch.ones(len(sizes)))


def test_icp_estimate_scale_full_overlap(dev):
    """X = all of Y under a similarity (s in [0.9, 1.1], rotation <= 0.1 rad): the checker alone converges to the
    truth at this size (asserted first), and the fused path must land on the same transform."""
    icp = _api().iterative_closest_point
    sizes = [(1500, 1500), (1000, 1000), (1200, 1200)]
    X, Y, lx, ly, (Rt, Tt, st) = _subset_setup(7200, sizes, similarity=True)
    want = ref.icp(X, Y, lx, ly, estimate_scale=True)
    assert want.converged
    assert float((want.R - Rt).abs().max()) <= 1e-6 and float((want.s - st).abs().max()) <= 1e-6
    pcx, pcy = _pcs(X, Y, lx, ly, dev)
    sol = icp(pcx, pcy, estimate_scale=True)
    print(f"estimate_scale: {len(sol.t_history)} iterations fused, {want.iterations} checker")
    assert sol.converged is True
    R, T, s = (t.double().cpu() for t in sol.RTs)
    assert float((R - want.R).abs().max()) <= 1e-5 and float((T - want.T).abs().max()) <= 1e-5
    assert float(((s - want.s).abs() / want.s).max()) <= 1e-5
    assert float((R - Rt).abs().max()) <= 1e-5 and float((T - Tt).abs().max()) <= 1e-5


def test_icp_history_is_consistent(dev):
    from pytorch3d_pointops_amd.functions import knn_points

    icp = _api().iterative_closest_point
    X, Y, lx, ly, _ = _subset_setup(7300, SUBSET_SIZES)
    Xd, Yd, lxd, lyd = X.to(dev), Y.to(dev), lx.to(dev), ly.to(dev)
    pcx, pcy = _pcs(X, Y, lx, ly, dev)
    long = icp(pcx, pcy, max_iterations=7, relative_rmse_thr=-1)
    assert len(long.t_history) == 7 and long.converged is False
    mask = ref.valid_mask(lx, X.shape[1]).double()
    ymax = float(Y.abs().max())
    runs = {i: icp(pcx, pcy, max_iterations=i, relative_rmse_thr=-1) for i in (1, 2, 3, 5, 6)}
    for i, run in runs.items():
        assert len(run.t_history) == i and run.converged is False
        for a, b in zip(run.t_history, long.t_history[:i]):
            assert all(torch.equal(u, v) for u, v in zip(a, b))
    for i in (1, 2, 5):
        Xt_i = runs[i].Xt.points_padded()
        idx_i = knn_points(Xt_i, Yd, lxd, lyd, K=1).idx[..., 0].cpu()
        want = ref.alignment(X, ref.gather(Y.double(), idx_i), mask)
        _check_alignment(long.t_history[i], want, ymax, False, f"history entry {i}")
        Xt_next = runs[i + 1].Xt.points_padded().double().cpu()
        assert float((Xt_next - ref.apply(X, *want[:3]) * mask[..., None]).abs().max()) <= 1e-5 * (1 + ymax)
    assert Xd.shape == Xt_i.shape


def test_icp_reuse_is_real_and_safe(dev):
    import pytorch3d_pointops_amd as pkg
    from pytorch3d_pointops_amd import _C

    icp = _api().iterative_closest_point
    sizes = [(15000, 20000), (12000, 20000)]
    X, Y, lx, ly, (Rt, Tt, _) = _subset_setup(7400, sizes)
    assert _C._lib.pointops_knn_uses_grid(2, 15000, 20000, 3, 1, -1) == 1
    pcx, pcy = _pcs(X, Y, lx, ly, dev)
    sol = icp(pcx, pcy)  # the grid family's fixed point, against the truth
    print(f"grid shape: converged after {len(sol.t_history)} iterations, rmse {sol.rmse.tolist()}")
    assert sol.converged is True and float(sol.rmse.max()) <= 1e-5
    assert float((sol.RTs.R.double().cpu() - Rt).abs().max()) <= 1e-5
    assert float((sol.RTs.T.double().cpu() - Tt).abs().max()) <= 1e-5

    def run(**kw):
        sol = icp(pcx, pcy, max_iterations=6, relative_rmse_thr=-1, **kw)
        return [sol.rmse, sol.Xt.points_padded()] + [t for h in sol.t_history for t in h]

    was_on = _C.grid_cache_enabled()
    try:
        pkg.set_grid_cache(False)
        before = dict(_C.grid_cache_stats)
        off = run()
        assert _C.grid_cache_stats == before
        pkg.set_grid_cache(True)
        before = dict(_C.grid_cache_stats)
        on = run()
        assert _C.grid_cache_stats == before and len(_C._GRID_CACHE) == 0
    finally:
        pkg.set_grid_cache(was_on)
    rebuilt = run(_reuse_grid=False)
    assert all(torch.equal(u, v) for u, v in zip(off, on))
    assert all(torch.equal(u, v) for u, v in zip(off, rebuilt))


def test_icp_init_transform_containers_and_empty_cloud(dev):
    from pytorch3d_pointops_amd.structures import Pointclouds

    api = _api()
    X, Y, lx, ly, (Rt, Tt, st) = _subset_setup(7500, SUBSET_SIZES)
    pcx, pcy = _pcs(X, Y, lx, ly, dev)
    init = api.SimilarityTransform(Rt.float().to(dev), Tt.float().to(dev), st.float().to(dev))
    sol = api.iterative_closest_point(pcx, pcy, init_transform=init)
    assert sol.converged is True and len(sol.t_history) <= 2
    assert float((sol.RTs.R.double().cpu() - Rt).abs().max()) <= 1e-5
    assert isinstance(sol.Xt, Pointclouds)
    assert torch.equal(sol.Xt.num_points_per_cloud(), pcx.num_points_per_cloud())
    padded = sol.Xt.points_padded()
    assert bool((padded[1, int(lx[1]):] == 0).all()) and bool(torch.isfinite(padded).all())
    # tensors in, tensors out; an empty cloud neither blocks convergence nor produces NaN
    lens = [2000, 0, 1200]
    pcx = Pointclouds([X[n, :lens[n]].to(dev) for n in range(3)])
    sol = api.iterative_closest_point(pcx, pcy)
    assert sol.converged is True
    assert all(bool(torch.isfinite(t).all()) for t in (sol.rmse, *sol.RTs, sol.Xt.points_padded()))
    assert float(sol.rmse[1]) == 0.0 and torch.equal(sol.RTs.R[1].cpu(), torch.eye(3))
    assert float((sol.RTs.R[0].double().cpu() - Rt[0]).abs().max()) <= 1e-5
    sol = api.iterative_closest_point(X[:1, :2000].to(dev), Y[:1].to(dev))
    assert torch.is_tensor(sol.Xt) and sol.Xt.shape == (1, 2000, 3) and sol.converged is True
    assert not sol.Xt.requires_grad


@pytest.mark.parametrize("sizes", [[(1024, 1024), (1024, 1024)], [(300, 400), (250, 380)]])
def test_icp_other_search_families(dev, sizes):
    """B=2, P=1024 (the small-batch family) and a ragged shape below every grid threshold (sparser clouds: a smaller
    motion, so that the nearest neighbours start out mostly right)."""
    icp = _api().iterative_closest_point
    X, Y, lx, ly, _ = _subset_setup(7600, sizes, motion=0.25)
    sol = icp(X.to(dev), Y.to(dev)) if sizes[0][0] == sizes[1][0] else icp(*_pcs(X, Y, lx, ly, dev))
    want = ref.icp(X, Y, lx, ly)
    assert sol.converged is True and want.converged
    assert float((sol.RTs.R.double().cpu() - want.R).abs().max()) <= 1e-5
    assert float((sol.RTs.T.double().cpu() - want.T).abs().max()) <= 1e-5


def test_icp_runs_exactly_max_iterations(dev, capsys):
    icp = _api().iterative_closest_point
    X, Y, lx, ly, _ = _subset_setup(7700, SUBSET_SIZES)
    sol = icp(*_pcs(X, Y, lx, ly, dev), relative_rmse_thr=-1, max_iterations=7, verbose=True)
    assert len(sol.t_history) == 7 and sol.converged is False
    assert capsys.readouterr().out.count("ICP iteration") == 7


def test_icp_float64_takes_the_composition(dev):
    """float64 clouds go through the torch composition over the public knn_points: same fixed point."""
    icp = _api().iterative_closest_point
    X, Y, lx, ly, (Rt, Tt, _) = _subset_setup(7800, [(500, 800), (500, 800)], motion=0.25)
    sol = icp(X.double().to(dev), Y.double().to(dev))
    assert sol.RTs.R.dtype == torch.float64
    want = ref.icp(X, Y)
    assert sol.converged == want.converged
    assert float((sol.RTs.R.cpu() - want.R).abs().max()) <= 1e-5
