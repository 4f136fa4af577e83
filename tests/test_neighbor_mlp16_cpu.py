"""The bfloat16 / float16 neighbor_mlp_max without a GPU: the entries and their binding, `supported16` against both
sizers, what the workspaces hold, the reference helper against a float64 loop, and the torch route CPU tensors still take."""
import numpy as np
import pytest
import torch

import neighbor_mlp16_ref as ref
from test_boundary_cpu import declared_prototypes

ENTRIES = ("pointops_neighbor_mlp_max16", "pointops_neighbor_mlp_max16_workspace_bytes",
           "pointops_neighbor_mlp_max16_backward", "pointops_neighbor_mlp_max16_backward_workspace_bytes")


def test_the_header_declares_the_entries_and_they_are_bound():
    from pytorch3d_pointops_amd import _C

    protos = declared_prototypes()
    assert set(ENTRIES) <= set(protos) and set(ENTRIES) <= set(_C.exported_symbols())
    for name in (ENTRIES[0], ENTRIES[2]):  # 16-bit buffers are void*, the type an int, the workspace a (void*, size_t) pair
        ret, params = protos[name]
        assert ret == "int" and params[0] == "const void*" and params.count("int") == 2  # (dtype and relu_out)
        assert params[-3:] == ["void*", "size_t", "void*"] and hasattr(_C._call, name[len("pointops_"):])


@pytest.mark.parametrize("dims,ok", [
    ((3, 37, 29, 20, 64, 32), True), ((1, 8, 8, 8, 8, 8), True), ((8, 65536, 65536, 16, 256, 256), True),
    ((1, 8, 8, 8, 4, 8), False), ((1, 8, 8, 8, 8, 12), False), ((1, 8, 8, 8, 264, 8), False),
    ((1, 8, 8, 0, 8, 8), False), ((1, 8, 8, 256, 8, 8), False), ((1 << 20, 1 << 11, 8, 1, 8, 8), False)])
def test_supported16_agrees_with_the_sizers(dims, ok):
    from pytorch3d_pointops_amd import _C, _C_neighbor_mlp

    N, L, M, K, C1, C2 = dims
    fwd = _C._lib.pointops_neighbor_mlp_max16_workspace_bytes(N, L, K, M, C1, C2)
    bwd = _C._lib.pointops_neighbor_mlp_max16_backward_workspace_bytes(N, L, K, M, C1, C2)
    assert _C_neighbor_mlp.supported16(*dims) is ok and (fwd > 0) is ok and (bwd > 0) is ok
    if ok:  # the pack: columns padded to 32, k to 16; the backward adds the table and at most the float32 partial plane
        pack = 2 * -(-C2 // 32) * 32 * -(-C1 // 16) * 16
        table = _C._lib.pointops_backward_det_workspace_bytes(N, L, K, M)
        assert pack <= fwd < pack + 256 and table + pack < bwd <= table + pack + 4 * 1024 * 129 * 128 + 512


def test_the_backward_workspace_ignores_K_beyond_the_table():
    from pytorch3d_pointops_amd import _C

    sizer = _C._lib.pointops_neighbor_mlp_max16_backward_workspace_bytes
    table = _C._lib.pointops_backward_det_workspace_bytes
    for C1, C2 in ((8, 256), (256, 64)):
        extra = {K: sizer(3, 37, K, 29, C1, C2) - table(3, 37, K, 29) for K in (3, 20)}
        assert extra[3] == extra[20] > 0


def test_the_reference_helper_follows_the_definition():
    N, L, M, K, C1, C2, dtype = 2, 3, 4, 2, 3, 2, torch.bfloat16
    rng = np.random.default_rng(3)
    r16 = lambda s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dtype).float().numpy()  # noqa: E731
    x, w, b, c, g = (r16(s) for s in ((N, M, C1), (C1, C2), (C2,), (N, L, C1), (N, L, C2)))
    idx, lengths = rng.integers(-1, M, (N, L, K)), np.array([M, 1])
    y, mag, ok = ref.forward(x, idx, w, b, c, lengths, dtype)
    rnd = lambda v: float(torch.tensor(v, dtype=torch.float32).to(dtype))  # noqa: E731
    h = np.zeros((N, L, K, C1))
    for n, l, k in np.ndindex(N, L, K):
        assert ok[n, l, k] == (0 <= idx[n, l, k] < M and k < lengths[n])
        if ok[n, l, k]:
            h[n, l, k] = [rnd(max(np.float32(x[n, idx[n, l, k], i]) + np.float32(c[n, l, i]), 0)) for i in range(C1)]
            for o in range(C2):
                assert np.isclose(y[n, l, k, o], b[o] + sum(h[n, l, k, i] * float(w[i, o]) for i in range(C1)), atol=1e-12)
    arg = np.where(ok.any(2)[..., None], np.where(ok[..., None], y, -np.inf).argmax(2), 255)
    back, s = ref.backward(x, idx, w, c, lengths, g, np.ones((N, L, C2)), arg, True, dtype)
    gw, gc = np.zeros((C1, C2)), np.zeros((N, L, C1))
    for n, l, o in np.ndindex(N, L, C2):
        if arg[n, l, o] != 255:
            gw[:, o] += g[n, l, o] * h[n, l, arg[n, l, o]]
            gc[n, l] += g[n, l, o] * w[:, o] * (h[n, l, arg[n, l, o]] > 0)
    assert np.allclose(back["weight"][0], gw, atol=1e-12) and np.allclose(back["center"][0], gc, atol=1e-12)
    assert s.sum() == ok.sum() and (back["weight"][1] >= np.abs(gw) - 1e-12).all()


def test_direct_calls_have_no_cpu_fallback_and_cpu_tensors_take_the_torch_route():
    from pytorch3d_pointops_amd import _C_neighbor_mlp, functions as f

    x, w = torch.zeros(2, 5, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16)
    idx = torch.zeros(2, 3, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_mlp.neighbor_mlp_max16(x, idx, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_mlp.neighbor_mlp_max16_backward(torch.zeros(2, 3, 8, dtype=torch.bfloat16), x, idx, w, None, None,
                                                    torch.zeros(2, 3, 8, dtype=torch.bfloat16),
                                                    torch.zeros(2, 3, 8, dtype=torch.uint8))
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((2, 5, 8)).astype(np.float32)).bfloat16().requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((8, 8)).astype(np.float32)).requires_grad_(True)  # cast to x.dtype
    out, arg = f.neighbor_mlp_max(x, torch.from_numpy(rng.integers(-1, 5, (2, 3, 2))), w, return_arg=True)
    assert out.dtype == torch.bfloat16 and arg.dtype == torch.uint8
    gx, gw = torch.autograd.grad(out.float().sum(), (x, w))
    assert gx.dtype == torch.bfloat16 and gw.dtype == torch.float32
