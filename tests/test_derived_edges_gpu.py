"""The operators built on the searches -- point covariances, local frames, alignment -- at the edges the other suites do
not reach: the switch between the staged and the direct kernels, row tiles, K = 1 and 2, degenerate neighbourhoods, launch
plan boundaries and rank-deficient clouds.  Every test calls the `_C` entries directly, so every input is chosen, and
compares with the plain restatements of tests/derived_ref.py (validated on the CPU by test_derived_ref_cpu.py).

u = 2^-24 throughout.  Each test prints its largest observed error as a multiple of its bound."""
import numpy as np
import pytest
import torch

import cases
import derived_ref as dr
import points_alignment_ref as ref
import registered_ops_cases as roc
from pytorch3d_pointops_amd import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -149  # spacing of fp32 subnormals (see tests/native/small_solvers_main.cpp)


def _C():
    from pytorch3d_pointops_amd import _C as c

    return c


def _signed(seed, shape):
    return (synth.uniform_f32(seed, shape) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _n(t):
    return t.detach().cpu().numpy()


def _rotations(seed, shape):
    """float64 rotation matrices (QR of random matrices, determinant fixed to +1)."""
    q = np.linalg.qr(_signed(seed, tuple(shape) + (3, 3)).astype(np.float64))[0]
    q[..., :, 0] *= np.sign(np.linalg.det(q))[..., None]
    return q


# ================================================================================================ 1. covariances
COV_PAIRS = [(3, 21), (3, 22), (2, 32), (2, 33), (1, 64), (1, 65), (4, 16), (4, 17), (3, 50), (3, 1), (8, 8), (8, 9)]
COV_ROWS = [(1, 1), (1, 127), (1, 128), (1, 129), (1, 255), (1, 256), (1, 257), (3, 171)]  # N * P = 1 .. 513


@pytest.mark.parametrize("D,K", COV_PAIRS)
def test_covariances_bit_equal_either_side_of_the_staged_switch(dev, D, K):
    """point_covariances and point_covariances_backward equal the fp32 restatement in every value: (D, K) either side of
    K * D = 64 (staged / direct form, compile-time D = 2, 3 and runtime D), row counts either side of the row tiles of
    128 (staged) and 256 (direct) and of more than one block."""
    C = _C()
    for N, P in COV_ROWS:
        knn = _signed(8100 + 7 * K + D + P, (N, P, K, D)) + np.float32(0.25)
        G = _signed(8200 + 7 * K + D + P, (N, P, D, D))
        got = _n(C.point_covariances(_t(knn, dev)))
        want = dr.cov_fp32(knn)
        assert got.shape == want.shape and np.array_equal(got, want), \
            (N, P, "forward", int((got != want).sum()), float(np.abs(got - want).max()))
        got = _n(C.point_covariances_backward(_t(knn, dev), _t(G, dev)))
        want = dr.cov_backward_fp32(knn, G)
        assert got.shape == want.shape and np.array_equal(got, want), \
            (N, P, "backward", int((got != want).sum()), float(np.abs(got - want).max()))


# ================================================================================================ 2. local frames
def _frames_forward_checks(dev, pts, idx, lengths, what, sign_check):
    """All the forward checks on one (points, idx, lengths); returns the share of rows left out of the sign check per
    column (None without sign check)."""
    C = _C()
    N, P, K = idx.shape
    p_d, i_d, l_d = _t(pts, dev), _t(idx, dev), _t(np.asarray(lengths, np.int64), dev)
    curv_t, raw_t = C.local_frames(p_d, l_d, i_d, False)
    curv2_t, frames_t = C.local_frames(p_d, l_d, i_d, True)
    assert torch.equal(curv_t, curv2_t), what
    curv, raw, frames = (_n(t).astype(np.float64) for t in (curv_t, raw_t, frames_t))
    valid = dr.valid_rows(lengths, P)
    assert bool((curv[~valid] == 0).all() and (raw[~valid] == 0).all() and (frames[~valid] == 0).all()), what
    if not valid.any():
        return None
    nb = dr.gather_neighbourhoods(pts, idx, lengths)
    c32 = dr.cov_fp32(nb)
    # the "same C" claim of the kernel's header: point_covariances(gather_neighbors(points, idx, lengths)) on the GPU
    cov_gpu = _n(C.point_covariances(C.gather_neighbors(p_d, i_d, l_d)))
    assert np.array_equal(cov_gpu[valid], c32[valid]), what
    c64 = c32.astype(np.float64)[valid]
    lam64 = np.linalg.eigvalsh(c64)
    lam_gpu = np.linalg.eigvalsh(cov_gpu.astype(np.float64)[valid])
    lmax = np.abs(lam64).max(-1, keepdims=True)
    cv, V = curv[valid], raw[valid]
    worst = {}
    for name, lam in (("restated C", lam64), ("GPU C", lam_gpu)):
        err = np.abs(cv - lam)
        assert bool((err <= 4 * U * lmax).all()), (what, name, float((err / np.maximum(4 * U * lmax, 1e-300)).max()))
        worst["curv"] = float((err / np.maximum(4 * U * lmax, 1e-300)).max())
    assert bool((cv[:, 0] <= cv[:, 1]).all() and (cv[:, 1] <= cv[:, 2]).all()), what
    orth = np.abs(np.einsum("raj,raq->rjq", V, V) - np.eye(3)).max((-1, -2))
    assert bool((orth <= 4 * U).all()), (what, "orthogonality", float(orth.max() / U))
    worst["orth"] = float(orth.max() / (4 * U))
    rec = np.abs(np.einsum("raj,rj,rbj->rab", V, cv, V) - c64).max((-1, -2))
    rec_bound = 8 * U * np.abs(c64).max((-1, -2)) + TINY
    assert bool((rec <= rec_bound).all()), (what, "reconstruction", float((rec / rec_bound).max()))
    worst["rec"] = float((rec / rec_bound).max())
    # disambiguated: columns 0 and 2 are the raw columns up to sign, column 1 = n x z
    F = frames[valid]
    sign = {}
    for j in (0, 2):
        same, neg = (F[:, :, j] == V[:, :, j]).all(-1), (F[:, :, j] == -V[:, :, j]).all(-1)
        assert bool((same | neg).all()), (what, "column", j)
        sign[j] = np.where(same, 1.0, -1.0)
    y = np.cross(F[:, :, 0], F[:, :, 2])
    yerr = np.abs(F[:, :, 1] - y).max()
    assert yerr <= 4 * U, (what, "y = n x z", yerr / U)
    worst["y"] = float(yerr / (4 * U))
    left_out = None
    if sign_check:
        # the majority rule in float64 on the kernel's own raw vectors: flip when fewer than K / 2 projections are > 0
        xi = pts.astype(np.float64)[valid]
        dx = nb.astype(np.float64)[valid] - xi[:, None, :]
        norm = np.sqrt((dx * dx).sum(-1))
        left_out = {}
        for j in (0, 2):
            p = np.einsum("rkd,rd->rk", dx, V[:, :, j])
            want = np.where(2 * (p > 0).sum(1) < K, -1.0, 1.0)
            unclear = ((np.abs(p) > 0) & (np.abs(p) <= 1e-5 * norm)).any(1)
            if K == 3 and j == 0:
                continue  # three points are coplanar: every projection on their normal is rounding noise
            assert bool((sign[j] == want)[~unclear].all()), (what, "sign of column", j,
                                                             int(((sign[j] != want) & ~unclear).sum()))
            left_out[j] = float(unclear.mean())
    print(f"{what}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + ("" if left_out is None else f"  left out of the sign check {left_out}"))
    return left_out


def _mid(P):
    return 40 if P > 64 else (P + 1) // 2  # P > 64: every tile after the first lies wholly past this length


@pytest.mark.parametrize("K", [1, 2, 3, 4, 63, 64, 65, 80])
def test_local_frames_every_valid_row_uniform(dev, K):
    """Uniform clouds, knn tables: K either side of the staged switch (kLfStageMaxK = 64) and K = 1, 2 (rank 0 and 1),
    P below, at and past a tile of 64, lengths {P, a mid-tile value, 0} -- at P = 65 and 130 the middle cloud ends in
    the first tile, so whole tiles lie past its length.  No eigenvalue-separation mask: every valid row is checked."""
    for P in (1, 63, 64, 65, 130):
        pts = _signed(8300 + K + P, (3, P, 3))
        lengths = np.array([P, _mid(P), 0])
        idx = roc.knn_table(pts, pts, lengths, lengths, K)
        left = _frames_forward_checks(dev, pts, idx, lengths, f"uniform K={K} P={P}", sign_check=True)
        if K >= 4 and P >= 63:  # (P = 1 is a single point: every projection is zero or rounding noise)
            assert all(v <= 0.02 for v in left.values()), left


@pytest.mark.parametrize("scale", [2.0 ** -30, 2.0 ** 30])
def test_local_frames_rescaled(dev, scale):
    P, K = 130, 8
    pts = (_signed(8400, (3, P, 3)) * np.float32(scale)).astype(np.float32)
    lengths = np.array([P, 97, 0])
    idx = roc.knn_table(pts, pts, lengths, lengths, K)
    left = _frames_forward_checks(dev, pts, idx, lengths, f"uniform x {scale:g}", sign_check=True)
    assert all(v <= 0.02 for v in left.values()), left


def test_local_frames_ball_table_and_out_of_range_entries(dev):
    """A ball_query-style table: -1 padding, and entries >= P (documented as zero rows, like gather_neighbors)."""
    P, K = 130, 8
    pts = _signed(8500, (3, P, 3))
    lengths = np.array([P, 97, 0])
    idx = roc.ball_table(pts, pts, lengths, lengths, K, 0.45)
    assert bool((idx == -1).any()) and bool((idx[0] >= 0).sum(1).min() >= 1)
    pick = synth.randint(8501, 0, 9, idx.shape)
    idx = np.where(pick == 0, P, np.where(pick == 1, 10 * P + 3, np.where(pick == 2, -7, idx))).astype(np.int64)
    _frames_forward_checks(dev, pts, idx, lengths, "ball table", sign_check=True)
    idx[:] = -1  # every neighbour a zero row: C = 0, identity frame before disambiguation
    _frames_forward_checks(dev, pts, idx, lengths, "all padding", sign_check=False)
    curv, raw = _C().local_frames(_t(pts, dev), _t(lengths, dev), _t(idx, dev), False)
    assert bool((curv == 0).all())
    assert torch.equal(raw[0], torch.eye(3, device=dev).expand(P, 3, 3))


def _crafted_shapes():
    """name -> (count, 3) float64 points; every shape has 4 or 6 points, so a table of K = 12 weighs them equally."""
    s = {"coincident": np.tile([[0.5, 0.25, -1.0]], (4, 1)),
         "collinear": np.outer(np.arange(6) - 2.5, [0.25, -0.5, 1.0]),
         "coplanar": np.array([[x, y, 0.0] for x in (-1.0, 0.0, 1.0) for y in (-0.5, 0.5)]),
         "octahedron": np.concatenate([np.eye(3), -np.eye(3)]),  # triple eigenvalue
         "square_and_axis": np.array([[1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0], [0, 0, 0.5], [0, 0, -0.5]], float)}
    return s


@pytest.mark.parametrize("moved", [False, True], ids=["exact", "rotated_and_shifted"])
def test_local_frames_degenerate_neighbourhoods(dev, moved):
    """Coincident, collinear and coplanar points, a triple and a double eigenvalue: exactly (centred, axis-aligned: the
    fp32 covariance is exactly degenerate) and after a rotation and a shift (degenerate up to rounding).  Every row of a
    cloud lists all of its points as neighbours.  No sign check on these."""
    shapes = _crafted_shapes()
    K, P = 12, 6
    rot = _rotations(8600, (len(shapes),))
    pts = np.zeros((len(shapes), P, 3), np.float32)
    lengths = np.zeros(len(shapes), np.int64)
    idx = np.zeros((len(shapes), P, K), np.int64)
    for n, (name, s) in enumerate(shapes.items()):
        if moved:
            s = s @ rot[n] + np.array([0.5, 0.25, -1.0])
        pts[n, :len(s)] = s.astype(np.float32)
        lengths[n] = len(s)
        idx[n] = np.arange(K) % len(s)
    # lengths[n] < K would zero the slots k >= lengths[n]: the clouds get the rows, the table stays complete
    big = np.concatenate([pts, np.zeros((len(shapes), K - P, 3), np.float32)], axis=1)
    big_idx = np.concatenate([idx, np.zeros((len(shapes), K - P, K), np.int64)], axis=1)
    _frames_forward_checks(dev, big, big_idx, np.full(len(shapes), K), f"crafted moved={moved}", sign_check=False)
    if not moved:
        curv, raw = _C().local_frames(_t(big, dev), _t(np.full(len(shapes), K), dev), _t(big_idx, dev), False)
        names = list(shapes)
        c = _n(curv)
        assert bool((c[names.index("coincident"), :4] == 0).all())
        assert bool((c[names.index("collinear"), :6, 2] > 0).all())  # (rank 1 exactly; the null pair is rounding of Jacobi)
        assert bool((c[names.index("coplanar"), :6, 0] == 0).all()) and bool((c[names.index("coplanar"), :6, 1] > 0).all())
        o = c[names.index("octahedron"), :6]
        assert bool((o[:, 0] == o[:, 2]).all()) and bool((o[:, 0] > 0).all())
        q = c[names.index("square_and_axis"), :6]
        assert bool((q[:, 1] == q[:, 2]).all()) and bool((q[:, 0] < q[:, 1]).all())


# ================================================================================================ 3. local_frames_backward
@pytest.mark.parametrize("disambiguate", [False, True])
@pytest.mark.parametrize("N,P,lengths", [(1, 1, [1]), (1, 255, [255]), (1, 256, [256]), (1, 257, [200]),
                                          (3, 171, [171, 100, 0])])
def test_local_frames_backward_per_entry(dev, N, P, lengths, disambiguate):
    """Constructed saved outputs: frames are fp32 roundings of random rotations (column 1 rebuilt as n x z in fp32 with
    `disambiguate`), curvatures ascending in three groups of rows -- gaps >= 0.1 lambda_max, gaps of 1e-4 lambda_max,
    and rows i % 7 == 3 with two equal eigenvalues.  Per entry |got - ref64| <= 32 u sum_{j,q} |w64[j][q]|: a term
    w v_a v_b carries about 14 roundings (the fold's cross product and sum 4, the dot product 5, the difference and the
    quotient 2, the two products and the sum 3), each at most u / 2 of a term bounded by |w|, with a factor of 2 -- a bar
    per ROW, so that a wrong row cannot hide behind a large one.  Rows with equal eigenvalues may be non-finite."""
    lengths = np.array(lengths, np.int64)
    q = _rotations(8700 + P, (N, P)).astype(np.float32)
    if disambiguate:
        n_, z_ = q[..., :, 0], q[..., :, 2]
        q[..., 0, 1] = n_[..., 1] * z_[..., 2] - n_[..., 2] * z_[..., 1]
        q[..., 1, 1] = n_[..., 2] * z_[..., 0] - n_[..., 0] * z_[..., 2]
        q[..., 2, 1] = n_[..., 0] * z_[..., 1] - n_[..., 1] * z_[..., 0]
    u3 = synth.uniform_f32(8710 + P, (N, P, 3)).astype(np.float64)
    row = np.arange(P)[None, :] + np.zeros((N, 1), np.int64)
    wide = np.stack([u3[..., 0], u3[..., 0] + 0.3 + u3[..., 1], u3[..., 0] + 1.5 + u3[..., 2]], -1)  # gaps >= 0.3, max < 3.5
    top = 0.5 + u3[..., 0]
    close = np.stack([top * (1 - 2e-4), top * (1 - 1e-4), top], -1)
    curv = np.where((row % 2 == 0)[..., None], wide, close)
    equal = row % 7 == 3
    curv[equal, 1] = curv[equal, 0]
    curv = curv.astype(np.float32)
    assert bool((np.diff(curv, axis=-1) >= 0).all()) and bool((np.diff(curv, axis=-1)[~equal] > 0).all())
    g_curv, g_frames = _signed(8720 + P, (N, P, 3)), _signed(8730 + P, (N, P, 3, 3))
    got = _n(_C().local_frames_backward(_t(curv, dev), _t(q, dev), _t(g_curv, dev), _t(g_frames, dev), _t(lengths, dev),
                                        disambiguate)).astype(np.float64)
    want, wabs = dr.local_frames_backward_f64(curv, q, g_curv, g_frames, lengths, disambiguate)
    valid = dr.valid_rows(lengths, P)
    assert bool((got[~valid] == 0).all())
    check = valid & ~equal
    if check.any():
        assert bool(np.isfinite(got[check]).all()) and bool(np.isfinite(want[check]).all())
        ratio = np.abs(got[check] - want[check]).max((-1, -2)) / (32 * U * wabs[check])
        print(f"local_frames_backward N={N} P={P} disambiguate={disambiguate}: worst error / bound = {ratio.max():.3f}")
        assert float(ratio.max()) <= 1.0


# ================================================================================================ 4. normals gradients
@pytest.mark.parametrize("disambiguate", [True, False])
@pytest.mark.parametrize("K", [21, 22, 50, 64, 65])
def test_normals_gradients_where_the_chain_changes_kernels(dev, K, disambiguate):
    """estimate_pointcloud_local_coord_frames end to end at K = 21 / 22 (the covariance backward leaves the staged form
    at K * 3 > 64), 50 (upstream's default neighbourhood) and 64 / 65 (the frames kernel leaves its staged form),
    against the float64 autograd reference of test_points_normals_gpu, with its masking of ill-conditioned rows and
    its bar: 1e-3 of the largest reference gradient entry."""
    import test_points_normals_gpu as tn
    from pytorch3d_pointops_amd.functions import knn_points, points_normals
    from pytorch3d_pointops_amd.structures import Pointclouds

    P = 130
    base = torch.from_numpy(cases.cloud(8800 + K, (2, P, 3))).to(dev)
    leaves = [base[0].clone().requires_grad_(True), base[1, :97].clone().requires_grad_(True)]
    pc = Pointclouds(leaves)
    lengths = pc.num_points_per_cloud()
    curv, frames = points_normals.estimate_pointcloud_local_coord_frames(pc, K, disambiguate)
    c = points_normals.centre_clouds(pc.points_padded().detach(), lengths)
    idx = knn_points(c, c, lengths, lengths, K=K).idx
    g = torch.Generator().manual_seed(17 + K)
    g_curv = torch.randn(curv.shape, generator=g, dtype=torch.float64)
    g_frames = torch.randn(frames.shape, generator=g, dtype=torch.float64)
    gap, lmax = tn._gaps(curv.detach().double().cpu())
    ill = (gap.amin(-1) < 1e-2 * lmax[..., 0]) | ~tn._valid(lengths, P)
    assert float((~ill).float().mean()) > 0.3
    g_curv[ill] = 0
    g_frames[ill] = 0
    want, _ = tn._reference_grads(leaves, lengths, idx, K, disambiguate, frames.detach(), g_curv, g_frames)
    got = torch.autograd.grad((curv * g_curv.float().to(dev)).sum() + (frames * g_frames.float().to(dev)).sum(), leaves)
    for a, b in zip(got, want):
        assert bool(torch.isfinite(a).all())
        scale = float(b.abs().max())
        err = float((a.double().cpu() - b).abs().max())
        print(f"normals gradient K={K} disambiguate={disambiguate}: error / (1e-3 largest entry) = {err / (1e-3 * scale):.4f}")
        assert scale > 0 and err <= 1e-3 * scale


# ================================================================================================ 5. alignment moments
@pytest.mark.parametrize("P", [1, 255, 256, 257, 2048, 2049, 4097, 65536, 65537])
def test_alignment_moments_at_launch_plan_boundaries(dev, P):
    """The fp64 moments against long-double sums of the same terms: a second block appears at P = 2049, the grid-stride
    loop at P = 65537 (more than 32 blocks of 2048 rows).  Per slot |got - ref| <= 2 L 2^-53 sum |terms| for a cloud of
    L rows (any summation order of L fp64 terms is within (L - 1) 2^-53 of the exact sum, to first order), so an empty
    cloud gives exact zeros.  d in {2, 3}; weights none and random, lengths none and {P, 1, 0}, no table and a table
    into P2 != P rows with entries outside [0, P2) (clamped to 0 and P2 - 1)."""
    C = _C()
    N = 2 if P > 4097 else 3
    worst = 0.0
    # (table with P2 != P, weights, lengths)
    for d, (use_idx, use_w, use_len) in [(d, c) for d in (3, 2) for c in ((False, False, False), (True, True, True),
                                                                         (True, False, False), (False, True, True))]:
        X = _signed(8900 + d + P, (N, P, d)) + np.float32(2.0)
        P2 = P + 3 if use_idx else P
        Y = _signed(8910 + d + P, (N, P2, d)) - np.float32(1.0)
        lengths = np.array([P, 1, 0][:N], np.int64) if use_len else None
        w = synth.uniform_f32(8920 + d + P, (N, P)) if use_w else None
        idx = synth.randint(8930 + d + P, -2, P2 + 1, (N, P)) if use_idx else None
        assert idx is None or P < 8 or (bool((idx < 0).any()) and bool((idx >= P2).any()))
        out = C.points_alignment(_t(X, dev), _t(Y, dev), _t(idx, dev), _t(lengths, dev), _t(w, dev), True, False, 1e-9,
                                 want_moments=True)
        got = _n(out[4])
        want, mabs, rows = dr.alignment_moments_f64(X, Y, idx, lengths, w)
        assert got.shape == want.shape and got.dtype == np.float64
        bound = 2.0 * rows[:, None] * 2.0 ** -53 * mabs
        err = np.abs(got - want)
        what = (d, use_idx, use_w, use_len)
        assert bool((err <= bound).all()), (what, float((err / np.maximum(bound, 1e-300)).max()))
        assert bool((got[rows == 0] == 0).all()), what
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        if not use_w:  # sums of ones are exact in any order: the count of rows, twice
            assert bool((got[:, 0] == rows).all()) and bool((got[:, 1] == rows).all()), what
    print(f"alignment moments P={P}: worst error / bound = {worst:.4f}")


# ================================================================================================ 6. alignment optimality
def _residual(X, Y, w, R, T, s):
    """sum_i w_i |s x_i R + T - y_i|^2 and sum_i w_i (|s x_i R|^2 + |y_i|^2), float64, per cloud."""
    xr = s[:, None, None] * (X @ R)
    e = xr + T[:, None, :] - Y
    return (w * (e * e).sum(-1)).sum(1), (w * ((xr * xr).sum(-1) + (Y * Y).sum(-1))).sum(1)


def _optimality_inputs():
    """name -> (X, Y, weights or None): the inputs of test_alignment_ragged_and_degenerate and crafted line, plane and
    coincident clouds.  Weights are masks: the definition forms C with w^2 and the means with w, so its transform
    minimises the weighted residual only where w^2 = w."""
    import test_points_alignment_gpu as ta

    P = 300
    lens = [300, 0, 1, 2, 3, 50, 299, 4]
    X = ta._cloud("uniform", len(lens), P, 6100)
    Y = ta._moved(X, 6200)
    mask = ref.valid_mask(lens, P).float()
    holes = mask * (torch.rand((len(lens), P), generator=ta._gen(3)) < 0.6).float()
    line = torch.linspace(0, 1, P)[:, None] * torch.tensor([0.3, -0.5, 0.8])
    Xd = torch.stack([line + 0.1, torch.full((P, 3), 0.25), X[0], torch.zeros(P, 3)])
    Yd = torch.stack([line @ ref.rotation([0.0, 0.0, 1.0], 0.4).float() - 0.2, torch.full((P, 3), -0.5), X[0] * 0 + 0.5,
                      torch.zeros(P, 3)])
    g = ta._gen(9001)
    plane = torch.rand((P, 3), generator=g) * torch.tensor([1.0, 1.0, 0.0])
    plane = (plane.double() @ ref.rotation([1.0, 2.0, 3.0], 0.7)).float()
    Xc = torch.stack([line, plane, torch.full((P, 3), 0.7), line * 0 + torch.tensor([1.0, 0.0, 0.0]) * line[:, :1]])
    Yc = ta._moved(Xc, 9002, noise=0.02)  # noisy targets: C has the rank of the source cloud
    Ym = ta._moved(Xc, 9003, noise=0.02, mirror=True)
    return {"ragged": (X, Y, mask), "ragged with holes": (X, Y, holes), "degenerate": (Xd, Yd, None),
            "crafted": (Xc, Yc, None), "crafted mirrored": (Xc, Ym, None)}


def test_alignment_is_optimal_on_every_cloud(dev):
    """Rank-deficient clouds leave R free, so R cannot be compared with the checker's; the residual can: evaluated in
    float64 from the returned fp32 (R, T, s), it must not exceed the checker's optimum by more than
    16 u sum_i w_i (|s x_i R|^2 + |y_i|^2) -- the first-order cost of rounding the 13 outputs to fp32: each rounding
    moves a residual vector by at most u / 2 of |s x R| or |T| <= |s x R| + |y|, and the cross term with the residual
    itself is at most of that size.  All four (estimate_scale, allow_reflection)."""
    C = _C()
    worst = 0.0
    for name, (X, Y, w) in _optimality_inputs().items():
        for estimate_scale, allow_reflection in [(False, False), (True, False), (False, True), (True, True)]:
            R, T, s, _, _ = C.points_alignment(X.to(dev), Y.to(dev), None, None, None if w is None else w.to(dev),
                                               estimate_scale, allow_reflection, 1e-9)
            R, T, s = (t.double().cpu() for t in (R, T, s))
            assert bool(torch.isfinite(R).all() and torch.isfinite(T).all() and torch.isfinite(s).all()), name
            R64, T64, s64, _ = ref.alignment(X, Y, w, estimate_scale, allow_reflection)
            w64 = torch.ones(X.shape[:2], dtype=torch.float64) if w is None else w.double()
            got, size = _residual(X.double(), Y.double(), w64, R, T, s)
            best, _ = _residual(X.double(), Y.double(), w64, R64, T64, s64)
            bound = 16 * U * size
            over = got - best
            ratio = float((over / bound.clamp(min=1e-300)).max())
            print(f"optimality {name} scale={estimate_scale} reflection={allow_reflection}: "
                  f"(residual - optimum) / bound = {ratio:.4f}")
            assert bool((over <= bound).all()), (name, estimate_scale, allow_reflection, over.tolist(), bound.tolist())
            worst = max(worst, ratio)
    print(f"alignment optimality: worst (residual - optimum) / bound = {worst:.4f}")


# ================================================================================================ 7. alignment backward
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("N,P,lengths", [(1, 255, [200]), (1, 256, [256]), (1, 257, [257]), (3, 171, [171, 100, 0])])
def test_alignment_backward_per_entry(dev, N, P, lengths, d):
    """points_alignment_backward against the float64 closed form: the kernel computes in fp64 and rounds once, so
    |got - ref| <= 2 u |ref| + 1e-30 per entry.  With and without weights; rows past the length are zero."""
    C = _C()
    X = _signed(9100 + P + d, (N, P, d)) + np.float32(1.5)
    Y = _signed(9110 + P + d, (N, P, d)) - np.float32(0.5)
    gm = _signed(9120 + P + d, (N, 3 + 4 * d + d * d)).astype(np.float64)
    lengths = np.array(lengths, np.int64)
    valid = dr.valid_rows(lengths, P)
    worst = 0.0
    for w in (None, synth.uniform_f32(9130 + P + d, (N, P)) + np.float32(0.1)):
        for lens in (lengths, None):
            got = C.points_alignment_backward(_t(X, dev), _t(Y, dev), _t(lens, dev), _t(w, dev), _t(gm, dev))
            want = dr.alignment_backward_f64(X, Y, lens, w, gm)
            assert (got[2] is None) == (w is None)
            for a, b in zip(got, want):
                if a is None:
                    continue
                a = _n(a).astype(np.float64)
                if lens is not None:
                    assert bool((a[~valid] == 0).all())
                err, bound = np.abs(a - b), 2 * U * np.abs(b) + 1e-30
                assert bool((err <= bound).all()), float((err / bound).max())
                worst = max(worst, float((err / bound).max()))
    print(f"alignment backward N={N} P={P} d={d}: worst error / bound = {worst:.4f}")
