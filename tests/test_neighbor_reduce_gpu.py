"""neighbor_reduce / knn_interpolate on the device against the float64 loops of tests/neighbor_reduce_ref.py, u = 2^-24:
forward (K + 2) u sum |w x|, max and arg exact; grad_x (s + 2) u sum |w g| (s: the target row's segment length), grad_w
(C + 2) u sum |g x|, byte-equal twice and in deterministic mode; knn_interpolate (2 K + 6) u max |x_k| and 1e-5 for its
gradients; a short and a null workspace rejected.  C: dword variant (1, 3, 7), vector variant (4, 64), chunks + tail (260)."""
import functools

import numpy as np
import pytest
import torch

import buffers
import neighbor_reduce_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N, L, M = 3, 37, 29
CS, KS = (1, 3, 4, 7, 64, 260), (1, 3, 20)
MODES = {"sum": ("sum", False), "sum_w": ("sum", True), "mean": ("mean", False), "max": ("max", False)}
HUB, LONELY = 11, 7


@functools.lru_cache(maxsize=None)
def _table(K):
    """idx, lengths, weights: -1 padding as ball_query writes it, a cloud with lengths < K, a query row without a valid
    slot, a cloud of length 0, target LONELY that nobody references, target HUB that every query of cloud 0 references."""
    rng = np.random.default_rng(100 + K)
    idx = rng.integers(0, M, (N, L, K))
    idx[idx == LONELY] = LONELY + 1
    idx[0, 5:9, max(1, K // 2):] = -1
    idx[0, :, 0] = HUB
    idx[1, 3, :] = -1
    lengths = np.array([M, K - 1, 0])
    weights = rng.standard_normal((N, L, K)).astype(np.float32)
    for a in (idx, lengths, weights):
        a.setflags(write=False)
    return idx, lengths, weights


@functools.lru_cache(maxsize=None)
def _features(C):
    rng = np.random.default_rng(200 + C)
    x = (np.round(rng.standard_normal((N, M, C)) * 4) / 4).astype(np.float32)  # quarter steps: ties for max
    g = rng.standard_normal((N, L, C)).astype(np.float32)
    x.setflags(write=False), g.setflags(write=False)
    return x, g


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _same_bytes(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C", CS)
def test_forward(C, K, mode):
    from pytorch3d_pointops_amd.functions import neighbor_reduce

    reduce, weighted = MODES[mode]
    (idx, lengths, weights), (x, _) = _table(K), _features(C)
    weights = weights if weighted else None
    want, want_arg, mag = ref.forward(x, idx, lengths, weights, reduce)
    t = _dev(x, idx, lengths, weights)
    out, arg = neighbor_reduce(t[0], t[1], t[2], reduce, t[3], return_arg=True)
    again, arg2 = neighbor_reduce(t[0], t[1], t[2], reduce, t[3], return_arg=True)
    assert out.dtype == torch.float32 and out.shape == (N, L, C) and _same_bytes(out, again)
    got = out.cpu().numpy().astype(np.float64)
    if reduce == "max":
        assert arg.dtype == torch.uint8 and _same_bytes(arg, arg2)
        assert np.array_equal(got, want) and np.array_equal(arg.cpu().numpy(), want_arg)
        assert (arg[2] == 255).all() and (arg[1, 3] == 255).all()
    else:
        assert arg is None
        err = np.abs(got - want)
        print(f"C={C} K={K} {mode}: max err / bound = {np.max(err / np.maximum((K + 2) * U * mag, 1e-300)):.3f}")
        assert (err <= (K + 2) * U * mag).all()
    assert not out[2].any() and not out[1, 3].any()  # the cloud of length 0, the row without a valid slot


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C", CS)
def test_backward(C, K, mode):
    from pytorch3d_pointops_amd.functions import neighbor_reduce

    reduce, weighted = MODES[mode]
    (idx, lengths, weights), (x, g) = _table(K), _features(C)
    weights = weights if weighted else None
    _, arg, _ = ref.forward(x, idx, lengths, weights, reduce)
    gx, gx_mag, seg, gw, gw_mag = ref.backward(x, idx, lengths, weights, reduce, g, arg)
    tx, ti, tl, tw, tg = _dev(x, idx, lengths, weights, g)
    leaves = [tx.requires_grad_(True)] + ([tw.requires_grad_(True)] if weighted else [])

    def grads():
        return torch.autograd.grad(neighbor_reduce(tx, ti, tl, reduce, tw), leaves, tg)

    first, second = grads(), grads()
    torch.use_deterministic_algorithms(True)
    try:
        third = grads()
    finally:
        torch.use_deterministic_algorithms(False)
    for a, b, c in zip(first, second, third):
        assert _same_bytes(a, b) and _same_bytes(a, c)
    got = first[0].cpu().numpy().astype(np.float64)
    assert got.shape == (N, M, C) and not got[:, LONELY].any() and seg[0, HUB] >= L - 1
    bound = (seg[:, :, None] + 2) * U * gx_mag
    print(f"C={C} K={K} {mode}: grad_x max err / bound = {np.max(np.abs(got - gx) / np.maximum(bound, 1e-300)):.3f}")
    assert (np.abs(got - gx) <= bound).all()
    if weighted:
        got_w = first[1].cpu().numpy().astype(np.float64)
        assert got_w.shape == (N, L, K) and (np.abs(got_w - gw) <= (C + 2) * U * gw_mag).all()
        assert not got_w[~ref.valid_slots(idx, lengths, M)].any()


@pytest.mark.parametrize("K", [3, 8])
def test_knn_interpolate(K):
    from pytorch3d_pointops_amd.functions import knn_interpolate, knn_points

    rng = np.random.default_rng(300 + K)
    Mx, Ly, C = 300, 257, 6
    lx, ly = np.array([300, 211]), np.array([257, 100])
    x = rng.standard_normal((2, Mx, C)).astype(np.float32)
    px, py = rng.random((2, Mx, 3)).astype(np.float32), rng.random((2, Ly, 3)).astype(np.float32)
    g = rng.standard_normal((2, Ly, C)).astype(np.float32)
    tx, tpx, tpy, tlx, tly, tg = _dev(x, px, py, lx, ly, g)
    leaves = [t.requires_grad_(True) for t in (tx, tpx, tpy)]
    out = knn_interpolate(tx, tpx, tpy, tlx, tly, K=K)
    got = torch.autograd.grad(out, leaves, tg)
    nn = knn_points(tpy.detach(), tpx.detach(), tly, tlx, K=K)
    want, top = ref.interpolate(x, nn.idx.cpu().numpy(), nn.dists.cpu().numpy(), lx, ly)
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - want)
    print(f"K={K}: max err / bound = {np.max(err / np.maximum((2 * K + 6) * U * top, 1e-300)):.3f}")
    assert (err <= (2 * K + 6) * U * top).all() and not out[1, 100:].any()
    # the float64 torch composition on the same idx
    dx, dpx, dpy = [t.detach().double().requires_grad_(True) for t in (tx, tpx, tpy)]
    n = torch.arange(2, device="cuda")[:, None, None]
    valid = (torch.arange(K, device="cuda")[None, None, :] < tlx[:, None, None]) & \
            (torch.arange(Ly, device="cuda")[None, :, None] < tly[:, None, None])
    d2 = ((dpy[:, :, None] - dpx[n, nn.idx]) ** 2).sum(-1)
    w = valid.double() / d2.clamp(min=1e-16)
    w = w / w.sum(2, keepdim=True).clamp(min=1e-300)
    wants = torch.autograd.grad((w[..., None] * dx[n, nn.idx]).sum(2), [dx, dpx, dpy], tg.double())
    for name, a, b in zip(("x", "pos_x", "pos_y"), got, wants):
        rel = float((a.double() - b).abs().max() / b.abs().max())
        print(f"K={K}: grad {name} max error relative to the largest magnitude = {rel:.2e}")
        assert rel <= 1e-5, name


def test_boundary_rejects_a_short_and_a_null_workspace(monkeypatch):
    from pytorch3d_pointops_amd import _C_neighbor_reduce

    (idx, lengths, weights), (x, g) = _table(3), _features(4)
    gx, _, _, gw, _ = ref.backward(x, idx, lengths, weights, "sum", g)
    t = dict(zip(("x", "idx", "lengths", "weights", "g"), _dev(x, idx, lengths, weights, g)))
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=declared_prototypes()) as k:
        k.watch(**t)
        grad_x, grad_w = _C_neighbor_reduce.neighbor_reduce_backward(t["g"], t["x"], t["idx"], t["lengths"], t["weights"],
                                                                     None, "sum", need_x=True, need_w=True)
    k.assert_all_clear()
    entry = "pointops_neighbor_reduce_backward"
    assert {(n, how) for n, _, how in k.rejections} == {(entry, "short"), (entry, "null")}
    assert [b.kind for b in k.buffers] == ["out", "out", "workspace"]
    # (the accepted call ran: test_backward holds these to their bounds)
    assert np.allclose(grad_x.cpu().numpy(), gx, rtol=1e-3, atol=1e-3)
    assert np.allclose(grad_w.cpu().numpy(), gw, rtol=1e-3, atol=1e-3)
