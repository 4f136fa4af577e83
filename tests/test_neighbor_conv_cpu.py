"""neighbor_conv without a GPU: the float64 torch route against tests/neighbor_conv_ref.py, the entries, the sizer and the
errors; voxel_neighbors against a brute-force lookup."""
import numpy as np
import pytest
import torch

import neighbor_conv_ref as ref


@pytest.mark.parametrize("with_coeff", [False, True], ids=["onehot", "coeff"])
def test_the_torch_composition_follows_the_definition(with_coeff):
    from pytorch3d_pointops_amd.functions import neighbor_conv

    rng = np.random.default_rng(7)
    N, L, M, K, Cin, Cout = 2, 9, 7, 4, 5, 3
    P = 6 if with_coeff else K
    idx = rng.integers(0, M, (N, L, K))
    idx[0, 2, 2:] = -1
    idx[0, 4, :] = -1  # an empty row
    lengths = np.array([M, 3])  # a short cloud
    x, w, g = (rng.standard_normal(s) for s in ((N, M, Cin), (P, Cin, Cout), (N, L, Cout)))
    coeff = rng.standard_normal((N, L, K, P)) if with_coeff else None
    fwd = ref.forward(x, idx, w, lengths, coeff)
    want, _ = ref.backward(x, idx, w, lengths, coeff, g, fwd)
    names = ("x", "weight", "coeff") if with_coeff else ("x", "weight")
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in ((x, w, coeff) if with_coeff else (x, w))]
    out = neighbor_conv(leaves[0], torch.from_numpy(idx), leaves[1], torch.from_numpy(lengths),
                        leaves[2] if with_coeff else None)
    assert out.dtype == torch.float64 and np.allclose(out.detach().numpy(), fwd["out"], rtol=0, atol=1e-12)
    assert not out[0, 4].any()
    for name, a in zip(names, torch.autograd.grad(out, leaves, torch.from_numpy(g))):
        assert np.allclose(a.numpy(), want[name][0], rtol=0, atol=1e-12), name
    if with_coeff:
        assert not a.numpy()[~ref.valid_slots(idx, lengths, M)].any()


def test_the_boundary_declares_the_entries_and_errors_need_no_device():
    from pytorch3d_pointops_amd import _C, _C_neighbor_conv, functions as f

    names = {"pointops_neighbor_conv", "pointops_neighbor_conv_backward", "pointops_neighbor_conv_backward_workspace_bytes"}
    assert names <= set(_C.exported_symbols()) and {"neighbor_conv", "voxel_neighbors"} <= set(f.__all__)
    sizer = _C._lib.pointops_neighbor_conv_backward_workspace_bytes
    det = _C._lib.pointops_backward_det_workspace_bytes
    assert sizer(3, 37, 20, 29, 15, 64, 32) >= det(3, 37, 20, 29) + 4 * 4 * 15 * 64 * 32  # the table, then 4 chunks
    for bad in ((-1, 8, 8, 8, 1, 8, 8), (1, 8, 0, 8, 1, 8, 8), (1, 8, 256, 8, 1, 8, 8), (1, 8, 8, 8, 33, 8, 8),
                (1, 8, 8, 8, 1, 6, 8), (1, 8, 8, 8, 1, 8, 132), (1 << 20, 1 << 11, 1, 8, 1, 8, 8)):
        assert sizer(*bad) == 0
    assert _C_neighbor_conv.supported(8, 65536, 65536, 16, 15, 64, 64)
    assert not _C_neighbor_conv.supported(1, 8, 8, 8, 1, 6, 8) and not _C_neighbor_conv.supported(1, 8, 8, 256, 1, 8, 8)
    x, w, idx = torch.zeros(2, 5, 8), torch.zeros(3, 8, 4), torch.zeros(2, 3, 2, dtype=torch.int64)
    for match, args, kw in (("idx must have", (x, idx[:1], w), dict(coeff=torch.zeros(1, 3, 2, 3))),
                            ("idx must have", (x, idx, w[:, :4]), dict(coeff=torch.zeros(2, 3, 2, 3))),
                            ("idx must be int64", (x, idx.int(), w), dict(coeff=torch.zeros(2, 3, 2, 3))),
                            ("lengths must be of shape", (x, idx, w[:2]), dict(lengths=torch.zeros(3, dtype=torch.int64))),
                            ("P == K", (x, idx, w), {}),
                            ("coeff must be of shape", (x, idx, w), dict(coeff=torch.zeros(2, 3, 2, 2)))):
        with pytest.raises(ValueError, match=match):
            f.neighbor_conv(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_conv.neighbor_conv(x, idx, w[:2])


@pytest.mark.parametrize("kernel_size", [1, 3])
def test_voxel_neighbors_finds_the_voxel_at_every_offset(kernel_size):
    from pytorch3d_pointops_amd.functions import voxel_neighbors

    rng = np.random.default_rng(3)
    P, r = 256, kernel_size // 2
    clouds = [np.unique(rng.integers(-3, 4, (n, 3)), axis=0) for n in (300, 20)]  # about 200 and 20 distinct cells
    clouds = [c[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))] for c in clouds]  # ascending (z, y, x)
    num = np.array([len(c) for c in clouds])
    assert num.max() <= P and num[1] < 27  # padded rows in both clouds
    coords = np.zeros((2, P, 3), dtype=np.int64)
    for n, c in enumerate(clouds):
        coords[n, :len(c)] = c
    got = voxel_neighbors(torch.from_numpy(coords), torch.from_numpy(num), kernel_size).numpy()
    want = np.full((2, P, kernel_size ** 3), -1)
    for n, c in enumerate(clouds):
        where = {tuple(v): i for i, v in enumerate(c)}
        for i, v in enumerate(c):
            offsets = [(dx, dy, dz) for dz in range(-r, r + 1) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
            want[n, i] = [where.get((v[0] + dx, v[1] + dy, v[2] + dz), -1) for dx, dy, dz in offsets]
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (got[1, num[1]:] == -1).all() and (got[0, :num[0], kernel_size ** 3 // 2] == np.arange(num[0])).all()
    with pytest.raises(ValueError, match="odd"):
        voxel_neighbors(torch.from_numpy(coords), torch.from_numpy(num), 2)
