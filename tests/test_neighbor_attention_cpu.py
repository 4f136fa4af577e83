"""neighbor_attention without a GPU: the float64 torch route against tests/neighbor_attention_ref.py; the host program over
csrc/neighbor_attention.h, plain and with the host sanitizers as a program of its own; the entries, the sizer, the errors."""
import os
import subprocess

import numpy as np
import pytest
import torch

import neighbor_attention_ref as ref
from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "neighbor_attention_main.cpp")


@pytest.mark.parametrize("with_bias", [False, True], ids=["no_bias", "bias"])
def test_the_torch_composition_follows_the_definition(with_bias):
    from pytorch3d_pointops_amd.functions import neighbor_attention

    rng = np.random.default_rng(7)
    N, L, M, K, heads, D = 2, 9, 7, 4, 3, 5
    idx = rng.integers(0, M, (N, L, K))
    idx[0, 2, 2:] = -1
    idx[0, 4, :] = -1  # an empty row
    lengths = np.array([M, 3])  # a short cloud
    q, k, v = (rng.standard_normal(s) for s in ((N, L, heads * D), (N, M, heads * D), (N, M, heads * D)))
    g = rng.standard_normal((N, L, heads * D))
    bias = rng.standard_normal((N, L, K, heads)) if with_bias else None
    if with_bias:
        bias[0, 1, 1:] = -np.inf  # one slot left
        bias[1, 5] = -np.inf      # none left
        bias[1, 6, 2, 1] = -np.inf
    scale = float(np.float32(0.3))
    fwd = ref.forward(q, k, v, idx, lengths, bias, heads, scale)
    want = ref.backward(q, k, v, idx, lengths, heads, scale, g, fwd)
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in ((q, k, v, bias) if with_bias else (q, k, v))]
    out = neighbor_attention(*leaves[:3], torch.from_numpy(idx), torch.from_numpy(lengths), heads,
                             leaves[3] if with_bias else None, 0.3)
    assert out.dtype == torch.float64 and np.allclose(out.detach().numpy(), fwd["out"], rtol=0, atol=1e-12)
    assert not out[0, 4].any() and (not with_bias or not out[1, 5].any())
    grads = torch.autograd.grad(out, leaves, torch.from_numpy(g))
    for name, a, b in zip(("q", "k", "v", "bias"), grads, want):
        assert np.isfinite(a.numpy()).all() and np.allclose(a.numpy(), b, rtol=0, atol=1e-12), name


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_the_header_deals_every_channel_of_every_head_to_one_lane(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "neighbor_attention")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout


def test_the_boundary_declares_the_entries_and_errors_need_no_device():
    from pytorch3d_pointops_amd import _C, _C_neighbor_attention, functions as f

    names = {"pointops_neighbor_attention", "pointops_neighbor_attention_backward",
             "pointops_neighbor_attention_backward_workspace_bytes"}
    assert names <= set(_C.exported_symbols()) and "neighbor_attention" in f.__all__
    sizer = _C._lib.pointops_neighbor_attention_backward_workspace_bytes
    det = _C._lib.pointops_backward_det_workspace_bytes
    assert sizer(3, 37, 20, 29, 8) >= det(3, 37, 20, 29) + 2 * 4 * 3 * 37 * 20 * 8  # the inverted table, then two planes
    for bad in ((-1, 8, 8, 8, 1), (1, 2 ** 31, 1, 8, 1), (1 << 20, 1 << 11, 1, 8, 1), (1, 1 << 20, 1 << 8, 8, 8),
                (1, 8, 8, 8, 0), (1, 8, 8, 8, (1 << 14) + 1)):
        assert sizer(*bad) == 0
    q, kv, idx = torch.zeros(2, 3, 8), torch.zeros(2, 5, 8), torch.zeros(2, 3, 2, dtype=torch.int64)
    for match, args, kw in (("k and v must be of one shape", (q, kv, kv[:, :4], idx), {}),
                            ("idx must be of shape", (q, kv, kv, idx[:1]), {}),
                            ("idx must be int64", (q, kv, kv, idx.int()), {}),
                            ("heads must divide", (q, kv, kv, idx), dict(heads=3)),
                            ("lengths must be of shape", (q, kv, kv, idx), dict(lengths=torch.zeros(3, dtype=torch.int64))),
                            ("bias must be of shape", (q, kv, kv, idx), dict(heads=2, bias=torch.zeros(2, 3, 2)))):
        with pytest.raises(ValueError, match=match):
            f.neighbor_attention(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_neighbor_attention.neighbor_attention(q, kv, kv, idx)
