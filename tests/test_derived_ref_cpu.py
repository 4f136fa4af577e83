"""The restatements of tests/derived_ref.py against independent float64 evaluations (numpy and torch autograd of the
plain definitions) on small inputs.  No GPU."""
import numpy as np
import pytest
import torch

import derived_ref as dr
from pytorch3d_pointops_amd import synth

U32 = 2.0 ** -24


def _signed(seed, shape):
    return (synth.uniform_f32(seed, shape) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)


@pytest.mark.parametrize("D,K", [(3, 1), (3, 2), (3, 22), (3, 50), (2, 33), (1, 65), (8, 9), (5, 7)])
def test_fp32_covariance_restatements_against_float64(D, K):
    """Standard running-error bound of a length-K fp32 sum of products, gamma_K ~ K u, plus the roundings of the mean
    (two: its own sum is another gamma_K on |x|, counted in the terms below), of v = x - m, of the product and of the
    final * inv_k: (K + 4) u times the sum of the absolute terms, where a term is taken with |x_k| + mean|x| in place of
    |x_k - m| so that the error of the fp32 mean is covered as well:
        forward   |c32 - c64|[a][b]   <= (K + 4) u  mean_k (|x_ka| + M_a)(|x_kb| + M_b),   M = mean_k |x_k|
        backward  |g32 - g64|[k][a]   <= (K + 4) u  sum_b |S_ab| (|x_kb| + M_b) / K,        S = G + G^T"""
    knn = _signed(100 + K, (37, K, D)) + np.float32(0.5 if K % 2 else 0.0)  # off-centre: the mean matters
    G = _signed(200 + K, (37, D, D))
    c32, c64 = dr.cov_fp32(knn), dr.cov_f64(knn)
    assert c32.dtype == np.float32 and c32.shape == (37, D, D)
    ax = np.abs(knn.astype(np.float64))
    t = ax + ax.mean(1, keepdims=True)
    bound = (K + 4) * U32 * np.einsum("rka,rkb->rab", t, t) / K
    err = np.abs(c32.astype(np.float64) - c64)
    print(f"D={D} K={K}: forward worst error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    g32, g64 = dr.cov_backward_fp32(knn, G), dr.cov_backward_f64(knn, G)
    assert g32.dtype == np.float32 and g32.shape == knn.shape
    S = np.abs(G.astype(np.float64) + G.astype(np.float64).transpose(0, 2, 1))
    bound = (K + 4) * U32 * np.einsum("rab,rkb->rka", S, t) / K
    err = np.abs(g32.astype(np.float64) - g64)
    print(f"D={D} K={K}: backward worst error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # the float64 evaluations themselves: torch autograd of the plain definition
    x = torch.from_numpy(knn).double().requires_grad_(True)
    v = x - x.mean(1, keepdim=True)
    cov = torch.einsum("rka,rkb->rab", v, v) / K
    assert np.allclose(cov.detach().numpy(), c64, rtol=0, atol=1e-14)
    (gx,) = torch.autograd.grad((cov * torch.from_numpy(G).double()).sum(), x)
    assert np.allclose(gx.numpy(), g64, rtol=0, atol=1e-14)


def test_covariance_restatement_is_sequential_fp32():
    """Order and operations are the documented ones, by hand on inputs where they matter: k ascending
    ((2^24 + 1) + 1 = 2^24 in fp32, 2^24 + (1 + 1) is not), and * float32(1 / K), not / K (1 / 3 rounds)."""
    f = np.float32
    inv3 = f(1.0) / f(3.0)
    for col in ([2.0 ** 24, 1.0, 1.0], [1.0, 0.0, 0.0], [0.9, 0.7, 0.3]):
        x = [f(t) for t in col]
        m = f(f(f(f(0.0) + x[0]) + x[1]) + x[2]) * inv3
        c = f(0.0)
        for k in range(3):
            v = f(x[k] - m)
            c = f(c + f(v * v))
        got = dr.cov_fp32(np.array(col, np.float32).reshape(1, 3, 1))[0, 0, 0]
        assert got == f(c * inv3), col
        s = f(f(f(2.5) + f(2.5)) * inv3)
        back = dr.cov_backward_fp32(np.array(col, np.float32).reshape(1, 3, 1), np.full((1, 1, 1), 2.5, np.float32))
        assert [back[0, k, 0] for k in range(3)] == [f(f(0.0) + f(s * f(x[k] - m))) for k in range(3)], col
    assert f(f(2.0 ** 24) + f(1.0)) + f(1.0) != f(2.0 ** 24) + f(f(1.0) + f(1.0))


def test_gather_rule():
    pts = _signed(300, (3, 6, 3))
    idx = np.array([[0, 5, -1, 6], [2, 2, 7, 1], [-3, 0, 0, 0], [5, 4, 3, 2], [1, 1, 1, 1], [0, 6, -1, 5]], np.int64)
    idx = np.stack([idx, idx[::-1], idx])
    lengths = np.array([6, 2, 0])
    got = dr.gather_neighbourhoods(pts, idx, lengths)
    for n in range(3):
        for i in range(6):
            for k in range(4):
                j = int(idx[n, i, k])
                want = pts[n, j] if (0 <= j < 6 and k < lengths[n]) else np.zeros(3, np.float32)
                assert np.array_equal(got[n, i, k], want), (n, i, k)
    assert bool((got[2] == 0).all()) and bool((got[1][:, 2:] == 0).all())
    assert np.array_equal(dr.valid_rows(lengths, 6), np.arange(6)[None] < lengths[:, None])


@pytest.mark.parametrize("disambiguate", [False, True])
def test_local_frames_backward_closed_form_against_autograd(disambiguate):
    """torch float64 autograd through eigh and the frame assembly.  eigh reads a symmetrised matrix, so its gradient is
    the symmetric part of the closed form -- the part the rest of the chain uses (covariance backward reads G + G^T)."""
    g = torch.Generator().manual_seed(31)
    A = torch.randn((2, 9, 3, 3), generator=g, dtype=torch.float64)
    C = (A @ A.transpose(-1, -2)).requires_grad_(True)
    lam, V = torch.linalg.eigh((C + C.transpose(-1, -2)) / 2)
    F = V
    if disambiguate:
        n, z = V[..., :, 0], V[..., :, 2]
        F = torch.stack([n, torch.cross(n, z, dim=-1), z], -1)
    gl = torch.randn(lam.shape, generator=g, dtype=torch.float64)
    gF = torch.randn(F.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad((lam * gl).sum() + (F * gF).sum(), C)
    lengths = np.array([9, 4])
    got, wabs = dr.local_frames_backward_f64(lam.detach().numpy(), F.detach().numpy(), gl.numpy(), gF.numpy(), lengths,
                                             disambiguate)
    sym = (got + got.transpose(0, 1, 3, 2)) / 2
    valid = dr.valid_rows(lengths, 9)
    err = np.abs(sym - want.numpy())[valid]
    assert float(err.max()) <= 1e-10 * float(wabs.max()), float(err.max())
    assert bool((got[~valid] == 0).all()) and bool((wabs[~valid] == 0).all()) and bool((wabs[valid] > 0).all())
    # equal eigenvalues: non-finite there, as documented, and nowhere else
    lam2 = lam.detach().numpy().copy()
    lam2[0, 3, 1] = lam2[0, 3, 0]
    got2, _ = dr.local_frames_backward_f64(lam2, F.detach().numpy(), gl.numpy(), gF.numpy(), lengths, disambiguate)
    assert not np.isfinite(got2[0, 3]).all()
    keep = np.ones((2, 9), bool)
    keep[0, 3] = False
    assert bool(np.isfinite(got2[keep]).all())


def _moments_torch(X, Y, w, lengths):
    """The plain definition in torch float64: sums over the valid rows of a cloud about its (constant) pivots."""
    N, P, D = X.shape
    out = []
    for n in range(N):
        L = int(lengths[n])
        if L == 0:
            out.append(torch.zeros(3 + 4 * D + D * D, dtype=torch.float64) + 0.0 * (X[n].sum() + Y[n].sum() + w[n].sum()))
            continue
        x = X[n, :L] - X[n, 0].detach()
        y = Y[n, :L] - Y[n, 0].detach()
        ww = w[n, :L]
        w2 = ww * ww
        out.append(torch.cat([ww.sum()[None], w2.sum()[None], (ww[:, None] * x).sum(0), (ww[:, None] * y).sum(0),
                              (w2[:, None] * x).sum(0), (w2[:, None] * y).sum(0),
                              torch.einsum("p,pa,pb->ab", w2, x, y).reshape(-1), (w2 * (x * x).sum(1)).sum()[None]]))
    return torch.stack(out)


@pytest.mark.parametrize("D", [2, 3])
def test_alignment_moments_and_backward_against_autograd(D):
    N, P = 3, 41
    lengths = np.array([41, 17, 0])
    X = torch.from_numpy(_signed(400 + D, (N, P, D)) + np.float32(3.0)).double().requires_grad_(True)
    Y = torch.from_numpy(_signed(410 + D, (N, P, D)) - np.float32(2.0)).double().requires_grad_(True)
    w = torch.from_numpy(synth.uniform_f32(420 + D, (N, P))).double().requires_grad_(True)
    want = _moments_torch(X, Y, w, lengths)
    Xn, Yn, wn = (t.detach().numpy().astype(np.float32) for t in (X, Y, w))
    mom, mabs, rows = dr.alignment_moments_f64(Xn, Yn, None, lengths, wn)
    assert np.array_equal(rows, lengths)
    assert bool((np.abs(mom - want.detach().numpy()) <= 1e-15 * P * mabs + 1e-300).all())
    assert bool((mom[2] == 0).all()) and bool((mabs >= np.abs(mom)).all())
    gm = torch.randn(want.shape, generator=torch.Generator().manual_seed(D), dtype=torch.float64)
    gX, gY, gw = torch.autograd.grad((want * gm).sum(), (X, Y, w))
    got = dr.alignment_backward_f64(Xn, Yn, lengths, wn, gm.numpy())
    for a, b in zip(got, (gX, gY, gw)):
        assert np.allclose(a, b.numpy(), rtol=1e-13, atol=1e-13)
    # no weights, no lengths
    ones = torch.ones((N, P), dtype=torch.float64)
    want = _moments_torch(X, Y, ones, np.array([P] * N))
    mom, _, rows = dr.alignment_moments_f64(Xn, Yn)
    assert np.array_equal(rows, [P] * N) and np.allclose(mom, want.detach().numpy(), rtol=1e-13, atol=1e-13)
    gX, gY = torch.autograd.grad((want * gm).sum(), (X, Y))
    got = dr.alignment_backward_f64(Xn, Yn, None, None, gm.numpy())
    assert np.allclose(got[0], gX.numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(got[1], gY.numpy(), rtol=1e-13, atol=1e-13)
    # a neighbour table with entries outside [0, P2): clamped to 0 and P2 - 1; P2 != P.  idx[n, 0] = -1 clamps to row 0,
    # the pivot of Y, so the gathered cloud's own row 0 is the pivot as well and the plain definition applies to it
    Y2 = _signed(430 + D, (N, 7, D))
    idx = np.tile(np.arange(P) % 9 - 1, (N, 1)).astype(np.int64)  # -1 .. 7
    mom, _, _ = dr.alignment_moments_f64(Xn, Y2, idx, lengths, wn)
    Yg = torch.from_numpy(np.stack([Y2[n][np.clip(idx[n], 0, 6)] for n in range(N)])).double()
    want = _moments_torch(X, Yg, w, lengths).detach().numpy()
    assert int(idx[0, 0]) == -1 and int(idx.max()) == 7 and np.allclose(mom, want, rtol=1e-13, atol=1e-13)
