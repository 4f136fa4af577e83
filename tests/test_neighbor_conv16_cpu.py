"""The bfloat16 / float16 neighbor_conv without a GPU: the entries and their binding, `supported16` against the sizers, the
argument errors, and the torch route that CPU tensors still take."""
import numpy as np
import pytest
import torch

from test_boundary_cpu import declared_prototypes

ENTRIES = ("pointops_neighbor_conv16", "pointops_neighbor_conv16_workspace_bytes", "pointops_neighbor_conv16_backward",
           "pointops_neighbor_conv16_backward_workspace_bytes")


def test_the_header_declares_the_entries_and_they_are_bound():
    from pytorch3d_pointops_amd import _C

    protos = declared_prototypes()
    assert set(ENTRIES) <= set(protos) and set(ENTRIES) <= set(_C.exported_symbols())
    for name in (ENTRIES[0], ENTRIES[2]):  # 16-bit buffers are void*, the type an int, the workspace a (void*, size_t) pair
        ret, params = protos[name]
        assert ret == "int" and params[0] == "const void*" and params.count("int") == 1
        assert params[-3:] == ["void*", "size_t", "void*"] and hasattr(_C._call, name[len("pointops_"):])


@pytest.mark.parametrize("dims,ok", [
    ((3, 37, 29, 20, 15, 64, 32), True), ((1, 8, 8, 8, 1, 8, 8), True), ((8, 65536, 65536, 16, 32, 256, 256), True),
    ((1, 8, 8, 8, 1, 4, 8), False), ((1, 8, 8, 8, 1, 8, 12), False), ((1, 8, 8, 8, 1, 264, 8), False),
    ((1, 8, 8, 0, 1, 8, 8), False), ((1, 8, 8, 256, 1, 8, 8), False), ((1, 8, 8, 8, 33, 8, 8), False),
    ((1 << 20, 1 << 11, 8, 1, 1, 8, 8), False)])
def test_supported16_agrees_with_the_sizers(dims, ok):
    from pytorch3d_pointops_amd import _C, _C_neighbor_conv

    N, L, M, K, P, Cin, Cout = dims
    fwd = _C._lib.pointops_neighbor_conv16_workspace_bytes(N, L, K, M, P, Cin, Cout)
    bwd = _C._lib.pointops_neighbor_conv16_backward_workspace_bytes(N, L, K, M, P, Cin, Cout)
    assert _C_neighbor_conv.supported16(*dims) is ok and (fwd > 0) is ok and (bwd > 0) is ok
    if ok:  # the pack: k padded to 16, columns to 32; the backward adds the table and the partial sums to its own
        pack = lambda k, o: 2 * P * -(-k // 16) * 16 * -(-o // 32) * 32  # noqa: E731
        assert pack(Cin, Cout) <= fwd < pack(Cin, Cout) + 256 and fwd <= 4 << 20
        assert bwd >= _C._lib.pointops_backward_det_workspace_bytes(N, L, K, M) + pack(Cout, Cin)


def test_the_argument_errors_need_no_device_and_cpu_tensors_take_the_torch_route():
    from pytorch3d_pointops_amd import _C_neighbor_conv, functions as f

    x, w = torch.zeros(2, 5, 8, dtype=torch.bfloat16), torch.zeros(2, 8, 8, dtype=torch.bfloat16)
    idx = torch.zeros(2, 3, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_conv.neighbor_conv16(x, idx, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_conv.neighbor_conv16_backward(torch.zeros(2, 3, 8, dtype=torch.bfloat16), x, idx, w, None, None)
    with pytest.raises(ValueError, match="P == K"):
        f.neighbor_conv(x, idx, w[:1])
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((2, 5, 8)).astype(np.float32)).bfloat16().requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((2, 8, 8)).astype(np.float32)).requires_grad_(True)  # cast to x.dtype
    idx = torch.from_numpy(rng.integers(-1, 5, (2, 3, 2)))
    out = f.neighbor_conv(x, idx, w)
    want = torch.nn.functional.pad(x.detach().double(), (0, 0, 0, 1))[torch.arange(2)[:, None, None], idx]  # -1: the zero row
    want = torch.einsum("nlkc,kco->nlo", want, w.detach().bfloat16().double())
    assert out.dtype == torch.bfloat16 and torch.allclose(out.double(), want, rtol=2.0 ** -6, atol=2.0 ** -6)
    gx, gw = torch.autograd.grad(out.float().sum(), (x, w))
    assert gx.dtype == torch.bfloat16 and gw.dtype == torch.float32
