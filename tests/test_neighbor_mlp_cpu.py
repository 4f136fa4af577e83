"""neighbor_mlp_max without a GPU: the float64 torch route against tests/neighbor_mlp_ref.py (arg is exact there: seeded
normals do not tie in float64), the entries, the sizer and the errors; edge_mlp_max against concatenate-and-MLP."""
import numpy as np
import pytest
import torch

import neighbor_mlp_ref as ref


def _inputs(rng, N, L, M, K, C1, C2):
    idx = rng.integers(0, M, (N, L, K))
    idx[0, 2, 2:] = -1
    idx[0, 4, :] = -1  # an empty row
    lengths = np.array([M, 3])  # a short cloud
    x, w, b, c, g = (rng.standard_normal(s) for s in ((N, M, C1), (C1, C2), (C2,), (N, L, C1), (N, L, C2)))
    return idx, lengths, x, w, b, c, g


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_the_torch_composition_follows_the_definition(full):
    from pytorch3d_pointops_amd.functions import neighbor_mlp_max

    N, L, M, K, C1, C2 = 2, 9, 7, 4, 5, 3
    idx, lengths, x, w, b, c, g = _inputs(np.random.default_rng(11), N, L, M, K, C1, C2)
    if not full:
        b = c = None
    y, _, ok = ref.forward(x, idx, w, b, c, lengths)
    want = np.where(ok.any(2)[..., None], np.where(ok[..., None], y, -np.inf).max(2), 0)
    want_arg = np.where(ok.any(2)[..., None], np.where(ok[..., None], y, -np.inf).argmax(2), 255)
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in ((x, w, b, c) if full else (x, w))]
    out, arg = neighbor_mlp_max(leaves[0], torch.from_numpy(idx), leaves[1], *(leaves[2:] if full else (None, None)),
                                lengths=torch.from_numpy(lengths), relu_out=full, return_arg=True)
    assert out.dtype == torch.float64 and arg.dtype == torch.uint8 and np.array_equal(arg.numpy(), want_arg)
    assert np.allclose(out.detach().numpy(), np.maximum(want, 0) if full else want, rtol=0, atol=1e-12)
    assert not out[0, 4].any() and (arg[0, 4] == 255).all()
    back, _ = ref.backward(x, idx, w, c, lengths, g, out.detach().numpy(), arg.numpy(), full)
    names = ("x", "weight", "bias", "center") if full else ("x", "weight")
    for name, a in zip(names, torch.autograd.grad(out, leaves, torch.from_numpy(g))):
        assert np.allclose(a.numpy(), back[name][0], rtol=0, atol=1e-12), name


def test_the_boundary_declares_the_entries_and_errors_need_no_device():
    from pytorch3d_pointops_amd import _C, _C_neighbor_mlp, functions as f
    from test_boundary_cpu import declared_prototypes

    names = {"pointops_neighbor_mlp_max", "pointops_neighbor_mlp_max_backward",
             "pointops_neighbor_mlp_max_backward_workspace_bytes"}
    assert names <= set(_C.exported_symbols()) and names <= set(declared_prototypes())
    assert {"neighbor_mlp_max", "edge_mlp_max"} <= set(f.__all__)
    sizer = _C._lib.pointops_neighbor_mlp_max_backward_workspace_bytes
    table = _C._lib.pointops_neighbor_reduce_backward_workspace_bytes
    for C1, C2 in ((8, 128), (128, 64)):  # no edge-sized plane: what is added to the table's workspace ignores K
        extra = {K: sizer(3, 37, K, 29, C1, C2) - table(3, 37, K, 29) for K in (3, 20)}
        assert extra[3] == extra[20] > 0
    for args in ((-1, 8, 8, 8, 8, 8), (1, 8, 0, 8, 8, 8), (1, 8, 256, 8, 8, 8), (1, 8, 8, 8, 6, 8), (1, 8, 8, 8, 8, 132),
                 (1, 8, 8, 8, 0, 8), (1 << 20, 1 << 11, 1, 8, 8, 8), (1, 8, 8, 8, 8, 8), (8, 65536, 16, 65536, 64, 128)):
        N, L, K, M, C1, C2 = args
        assert (sizer(*args) > 0) == (N >= 0 and _C_neighbor_mlp.supported(N, L, M, K, C1, C2)), args
    x, w, idx = torch.zeros(2, 5, 8), torch.zeros(8, 4), torch.zeros(2, 3, 2, dtype=torch.int64)
    for match, args, kw in (("x must be of shape", (x, idx, w[0]), {}),
                            ("idx must have", (x, idx[:1], w), {}),
                            ("idx must have", (x, idx, w[:4]), {}),
                            ("idx must be int64", (x, idx.int(), w), {}),
                            ("lengths must be of shape", (x, idx, w), dict(lengths=torch.zeros(3, dtype=torch.int64))),
                            ("bias must be of shape", (x, idx, w), dict(bias=torch.zeros(8))),
                            ("center must be of shape", (x, idx, w), dict(center=torch.zeros(2, 5, 8)))):
        with pytest.raises(ValueError, match=match):
            f.neighbor_mlp_max(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_mlp.neighbor_mlp_max(x, idx, w)


@pytest.mark.parametrize("kind", ["edgeconv", "pointnet2"])
def test_edge_mlp_max_is_the_concatenated_two_layer_mlp(kind):
    from pytorch3d_pointops_amd.functions import edge_mlp_max

    N, L, M, K, C1, C2, D = 2, 9, 7, 4, 5, 3, 6
    rng = np.random.default_rng(5)
    idx, lengths, _, w2, b2, _, _ = _inputs(rng, N, L, M, K, C1, C2)
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    b1, w2, b2, lengths = t(rng.standard_normal(C1)), t(w2), t(b2), t(lengths)
    if kind == "edgeconv":  # [x_i, x_j - x_i] with L == M rows
        xq = xt = t(rng.standard_normal((N, M, D)))
        idx = idx[:, :M]
        w1 = t(rng.standard_normal((2 * D, C1)))
        edge = lambda n, l, j: torch.cat([xq[n, l], xt[n, j] - xq[n, l]])  # noqa: E731
        got = edge_mlp_max(xt, xq, t(idx), w1[D:], w1[:D] - w1[D:], b1, w2, b2, lengths)
    else:  # [p_j - p_i, f_j]
        pt, pq, ft = (t(rng.standard_normal(s)) for s in ((N, M, 3), (N, L, 3), (N, M, D)))
        w1 = t(rng.standard_normal((3 + D, C1)))
        edge = lambda n, l, j: torch.cat([pt[n, j] - pq[n, l], ft[n, j]])  # noqa: E731
        got = edge_mlp_max(torch.cat([pt, ft], 2), pq, t(idx), w1, -w1[:3], b1, w2, b2, lengths)
    want = torch.zeros_like(got)
    for n, l in np.ndindex(*idx.shape[:2]):
        ys = [torch.relu(edge(n, l, int(j)) @ w1 + b1) @ w2 + b2
              for k, j in enumerate(idx[n, l]) if 0 <= j < M and k < int(lengths[n])]
        if ys:
            want[n, l] = torch.relu(torch.stack(ys).amax(0))
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
