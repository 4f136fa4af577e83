"""neighbor_mlp_max with a second hidden layer without a GPU: the entries and their binding, `supported2_16` against both
sizers, the reference helper against a plain loop, the torch route CPU tensors take, and the unchanged one-layer call."""
import numpy as np
import pytest
import torch

import neighbor_mlp2_ref as ref
from test_boundary_cpu import declared_prototypes

ENTRIES = ("pointops_neighbor_mlp2_max16", "pointops_neighbor_mlp2_max16_workspace_bytes",
           "pointops_neighbor_mlp2_max16_backward", "pointops_neighbor_mlp2_max16_backward_workspace_bytes")


def test_the_header_declares_the_entries_and_they_are_bound():
    from pytorch3d_pointops_amd import _C

    protos = declared_prototypes()
    assert set(ENTRIES) <= set(protos) and set(ENTRIES) <= set(_C.exported_symbols())
    for name in (ENTRIES[0], ENTRIES[2]):
        ret, params = protos[name]
        assert ret == "int" and params[0] == "const void*" and params.count("int") == 2  # (dtype and relu_out)
        assert params[-3:] == ["void*", "size_t", "void*"] and hasattr(_C._call, name[len("pointops_"):])


@pytest.mark.parametrize("dims,ok", [
    ((3, 37, 29, 20, 64, 64, 128), True), ((1, 8, 8, 8, 8, 8, 8), True), ((8, 65536, 65536, 16, 128, 128, 256), True),
    ((1, 8, 8, 8, 136, 8, 8), False), ((1, 8, 8, 8, 8, 136, 8), False), ((1, 8, 8, 8, 8, 8, 264), False),
    ((1, 8, 8, 8, 8, 12, 8), False), ((1, 8, 8, 8, 8, 8, 4), False), ((1, 8, 8, 0, 8, 8, 8), False),
    ((1, 8, 8, 256, 8, 8, 8), False), ((1 << 20, 1 << 11, 8, 1, 8, 8, 8), False)])
def test_supported2_16_agrees_with_the_sizers(dims, ok):
    from pytorch3d_pointops_amd import _C, _C_neighbor_mlp

    N, L, M, K, C1, C2, C3 = dims
    fwd = _C._lib.pointops_neighbor_mlp2_max16_workspace_bytes(N, L, K, M, C1, C2, C3)
    bwd = _C._lib.pointops_neighbor_mlp2_max16_backward_workspace_bytes(N, L, K, M, C1, C2, C3)
    assert _C_neighbor_mlp.supported2_16(*dims) is ok and (fwd > 0) is ok and (bwd > 0) is ok
    if ok:  # the backward holds the table and e1 (N,L,K,C1) of T
        assert bwd > _C._lib.pointops_backward_det_workspace_bytes(N, L, K, M) + 2 * N * L * K * C1


def test_the_reference_helper_follows_the_definition():
    N, L, M, K, C1, C2, C3, dtype = 2, 3, 4, 2, 3, 4, 2, torch.bfloat16
    rng = np.random.default_rng(3)
    r16 = lambda s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dtype).float().numpy()  # noqa: E731
    x, w, b, w2, b2, c, g = (r16(s) for s in ((N, M, C1), (C1, C2), (C2,), (C2, C3), (C3,), (N, L, C1), (N, L, C3)))
    idx, lengths = rng.integers(-1, M, (N, L, K)), np.array([M, 1])
    y, mag, ok, amb = ref.forward(x, idx, w, b, w2, b2, c, lengths, dtype)
    rnd = lambda v: float(torch.tensor(v, dtype=torch.float32).to(dtype))  # noqa: E731
    h1, h2 = np.zeros((N, L, K, C1)), np.zeros((N, L, K, C2))
    for n, l, k in np.ndindex(N, L, K):
        assert ok[n, l, k] == (0 <= idx[n, l, k] < M and k < lengths[n])
        if ok[n, l, k]:
            h1[n, l, k] = [rnd(max(np.float32(x[n, idx[n, l, k], i]) + np.float32(c[n, l, i]), 0)) for i in range(C1)]
            h2[n, l, k] = [max(b[o] + sum(h1[n, l, k, i] * float(w[i, o]) for i in range(C1)), 0) for o in range(C2)]
            for d in range(C3):
                assert np.isclose(y[n, l, k, d], b2[d] + sum(h2[n, l, k, o] * float(w2[o, d]) for o in range(C2)), atol=1e-12)
    assert not amb.any() and (mag >= np.abs(y) - 1e-12)[ok].all()
    arg = np.where(ok.any(2)[..., None], np.where(ok[..., None], y, -np.inf).argmax(2), 255)
    back, s = ref.backward(x, idx, w, b, w2, c, lengths, g, np.ones((N, L, C3)), arg, True, dtype)
    gw, gw2, gc = np.zeros((C1, C2)), np.zeros((C2, C3)), np.zeros((N, L, C1))
    for n, l, d in np.ndindex(N, L, C3):
        if arg[n, l, d] != 255:
            k = arg[n, l, d]
            gw2[:, d] += g[n, l, d] * h2[n, l, k]
            e2 = g[n, l, d] * w2[:, d] * (h2[n, l, k] > 0)
            gw += np.outer(h1[n, l, k], e2)
            gc[n, l] += (w @ e2) * (h1[n, l, k] > 0)
    for name, want in (("weight", gw), ("weight2", gw2), ("center", gc)):
        assert np.allclose(back[name][0], want, atol=1e-12) and (back[name][1] >= np.abs(want) - 1e-12).all(), name
    assert s.sum() == ok.sum() and np.allclose(back["bias2"][0], np.where(arg != 255, g, 0).sum((0, 1)))


def test_cpu_tensors_take_the_torch_route_and_the_one_layer_call_is_unchanged():
    from pytorch3d_pointops_amd import _C_neighbor_mlp, functions as f

    rng = np.random.default_rng(5)
    r = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    x, w, b, w2, b2 = r(2, 5, 8).bfloat16().requires_grad_(True), r(8, 16), r(16), r(16, 24).requires_grad_(True), r(24)
    idx = torch.from_numpy(rng.integers(-1, 5, (2, 3, 2)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_mlp.neighbor_mlp2_max16(x.detach(), idx, w.bfloat16(), None, w2.detach().bfloat16())
    out, arg = f.neighbor_mlp_max(x, idx, w, b, return_arg=True, weight2=w2, bias2=b2)
    assert out.dtype == torch.bfloat16 and out.shape == (2, 3, 24) and arg.dtype == torch.uint8 and arg.shape == out.shape
    gx, gw2 = torch.autograd.grad(out.float().sum(), (x, w2))
    assert gx.dtype == torch.bfloat16 and gw2.dtype == torch.float32 and gw2.shape == (16, 24)
    h = torch.relu(torch.relu(x.detach()[:, :, None, :]) @ w.bfloat16() + b.bfloat16())  # idx to the row itself:
    own = torch.arange(5).reshape(1, 5, 1).expand(2, 5, 1)
    assert torch.equal(f.neighbor_mlp_max(x.detach(), own, w, b, weight2=w2.detach(), bias2=b2),
                       torch.relu(h @ w2.detach().bfloat16() + b2.bfloat16()).squeeze(2))
    assert f.edge_mlp_max(r(2, 5, 4), r(2, 3, 4), idx, r(4, 8), r(4, 8), r(8), w, b, w3=w2.detach(), b3=b2).shape == (2, 3, 24)
    one = f.neighbor_mlp_max(x.detach(), idx, w, b, return_arg=True)
    again = f.neighbor_mlp_max(x.detach(), idx, w, b, None, None, True, True, None, None)
    assert all(torch.equal(p, q) for p, q in zip(one, again)) and one[0].shape == (2, 3, 16)
    with pytest.raises(ValueError, match="bias2 needs weight2"):
        f.neighbor_mlp_max(x, idx, w, b, bias2=b2)
