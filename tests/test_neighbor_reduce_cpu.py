"""neighbor_reduce without a GPU: the torch route (CPU, float64) against tests/neighbor_reduce_ref.py; the host program over
csrc/neighbor_reduce.h (tests/native/neighbor_reduce_main.cpp), plain and with the host sanitizers as a program of its
own -- no sanitized code is loaded into Python; the boundary's entries, the sizer and the errors that need no device."""
import os
import subprocess

import numpy as np
import pytest
import torch

import neighbor_reduce_ref as ref
from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "neighbor_reduce_main.cpp")


def _small_table():
    rng = np.random.default_rng(5)
    N, L, M, K, C = 2, 9, 7, 4, 5
    idx = rng.integers(0, M, (N, L, K))
    idx[0, 2, 2:] = -1
    idx[0, 4, :] = -1
    lengths = np.array([M, 3])
    x = np.round(rng.standard_normal((N, M, C)) * 4) / 4
    return x, idx, lengths, rng.standard_normal((N, L, K)), rng.standard_normal((N, L, C))


@pytest.mark.parametrize("mode", ["sum", "sum_w", "mean", "max"])
def test_the_torch_composition_follows_the_definition(mode):
    from pytorch3d_pointops_amd.functions import neighbor_reduce

    reduce = mode.split("_")[0]
    x, idx, lengths, weights, g = _small_table()
    weights = weights if mode == "sum_w" else None
    want, want_arg, _ = ref.forward(x, idx, lengths, weights, reduce)
    gx, gx_mag, _, gw, _ = ref.backward(x, idx, lengths, weights, reduce, g, want_arg)
    tx = torch.from_numpy(x).requires_grad_(True)
    tw = torch.from_numpy(weights).requires_grad_(True) if weights is not None else None
    out, arg = neighbor_reduce(tx, torch.from_numpy(idx), torch.from_numpy(lengths), reduce, tw, return_arg=True)
    assert out.dtype == torch.float64 and np.allclose(out.detach().numpy(), want, rtol=0, atol=1e-13)
    if reduce == "max":
        assert arg.dtype == torch.uint8 and np.array_equal(arg.numpy(), want_arg)
    else:
        assert arg is None
    grads = torch.autograd.grad(out, [tx] + ([tw] if tw is not None else []), torch.from_numpy(g))
    # (the definition's factor of the mean backward is the fp32 fl(1 / count): 2^-24 relative to the float64 quotient)
    assert (np.abs(grads[0].numpy() - gx) <= 1e-12 + (2.0 ** -24 * gx_mag if reduce == "mean" else 0.0)).all()
    if tw is not None:
        assert np.allclose(grads[1].numpy(), gw, rtol=0, atol=1e-12)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_the_header_deals_every_channel_to_one_lane(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "neighbor_reduce")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout


def test_the_boundary_declares_the_entries_and_errors_need_no_device():
    from pytorch3d_pointops_amd import _C, _C_neighbor_reduce, functions as f

    names = {"pointops_neighbor_reduce", "pointops_neighbor_reduce_backward",
             "pointops_neighbor_reduce_backward_workspace_bytes"}
    assert names <= set(_C.exported_symbols()) and {"neighbor_reduce", "knn_interpolate"} <= set(f.__all__)
    sizer = _C._lib.pointops_neighbor_reduce_backward_workspace_bytes
    det = _C._lib.pointops_backward_det_workspace_bytes
    assert sizer(3, 37, 20, 29) >= det(3, 37, 20, 29) + 4 * 3 * 37  # the inverted table, then a factor per query row
    for bad in ((-1, 8, 8, 8), (1, 2 ** 31, 1, 8), (1 << 20, 1 << 11, 1, 8), (1 << 16, 1, 1, 1 << 15)):
        assert sizer(*bad) == 0
    x, idx = torch.zeros(2, 5, 4), torch.zeros(2, 3, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="same batch dimension"):
        f.neighbor_reduce(x, idx[:1])
    with pytest.raises(ValueError, match="reduce must be one of"):
        f.neighbor_reduce(x, idx, reduce="min")
    with pytest.raises(ValueError, match="weights go with"):
        f.neighbor_reduce(x, idx, reduce="max", weights=torch.zeros(2, 3, 2))
    with pytest.raises(ValueError, match="K has to be"):
        f.knn_interpolate(x, torch.zeros(2, 5, 3), torch.zeros(2, 3, 3), K=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_reduce.neighbor_reduce(x, idx)
