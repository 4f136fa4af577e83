"""neighbor_mlp_max on the device against tests/neighbor_mlp_ref.py; u = 2^-24, every bound is (1 + 2^-6) (t + 2) u mag
with t the rounded operations of the result's chain (the NEIGHBOUR MLP-MAX block of include/pointops_amd.h):
  out          t = C1 + 1: the add of a, the C1 fmaf of y; against the float64 max_k y, the bound the maximum over the
               row's valid slots (|max a - max b| <= max |a - b|)
  arg          255 exactly where no slot is valid, else a valid slot whose float64 y is within twice that bound of the maximum
  grad_x       t = s + C2: at most C2 fmaf in e, the s adds over the target row's entries
  grad_center  t = K + C2
  grad_weight, grad_bias  t = N L + ceil(N L / 32): one fmaf (add) per row, one add per partial block
The backward reference takes the device's out and arg, so a near-tie cannot fail a gradient.
The table is test_neighbor_conv_gpu's: L = 37 is a 5-row tail behind a full tile, N L = 111 a tail for the 64- and 128-row
workgroups; K = 40 re-stages the slots (32 at a time) with the running best carried over.  (C1, C2): one k-step pair with 28 padded columns, a column block with a tail, one or two blocks, four row
tiles per workgroup, four column blocks."""
import functools

import numpy as np
import pytest
import torch

import buffers
import neighbor_mlp_ref as ref
from test_boundary_cpu import declared_prototypes
from test_neighbor_conv_gpu import HUB, LONELY, L, M, N, U, _dev, _same_bytes, _table

pytestmark = pytest.mark.gpu

SHAPES, KS, VARIANTS = ((4, 4), (24, 40), (64, 64), (128, 32), (32, 128)), (1, 3, 20, 40), ("plain", "full")
GRADS = ("x", "weight", "bias", "center")


@functools.lru_cache(maxsize=None)
def _case(C1, C2, K, variant):
    """The inputs and the reference's forward, computed once."""
    idx, lengths = _table(K)
    rng = np.random.default_rng(1000 * C1 + C2 + K)
    x, w, b, c, g = (rng.standard_normal(s).astype(np.float32)
                     for s in ((N, M, C1), (C1, C2), (C2,), (N, L, C1), (N, L, C2)))
    if variant == "plain":
        b = c = None
    for a in (x, w, b, c, g):
        if a is not None:
            a.setflags(write=False)
    y, mag, ok = ref.forward(x, idx, w, b, c, lengths)
    return dict(x=x, weight=w, bias=b, center=c, g=g, idx=idx, lengths=lengths, y=y, mag=mag, ok=ok,
                relu_out=variant == "full")


def _tensors(c):
    names = ("x", "idx", "weight", "bias", "center", "lengths", "g")
    return dict(zip(names, _dev(*[c[n] for n in names])))


def _run(t, relu_out):
    from pytorch3d_pointops_amd.functions import neighbor_mlp_max

    return neighbor_mlp_max(t["x"], t["idx"], t["weight"], t["bias"], t["center"], t["lengths"], relu_out, return_arg=True)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C1,C2", SHAPES)
def test_forward(C1, C2, K, variant):
    from pytorch3d_pointops_amd import _C_neighbor_mlp

    c = _case(C1, C2, K, variant)
    t = _tensors(c)
    out, arg = _run(t, c["relu_out"])
    assert out.dtype == torch.float32 and out.shape == (N, L, C2) and arg.dtype == torch.uint8 and arg.shape == out.shape
    for other in (_run(t, c["relu_out"]), _C_neighbor_mlp.neighbor_mlp_max(
            t["x"], t["idx"], t["weight"], t["bias"], t["center"], t["lengths"], c["relu_out"])):
        assert _same_bytes(out, other[0]) and _same_bytes(arg, other[1])
    got, slot = out.cpu().numpy().astype(np.float64), arg.cpu().numpy().astype(np.int64)
    ok, none = c["ok"][..., None], ~c["ok"].any(2)
    y = np.where(ok, c["y"], -np.inf)
    want = np.where(none[..., None], 0, y.max(2))
    bound = (1 + 2.0 ** -6) * (C1 + 1 + 2) * U * np.where(ok, c["mag"], 0).max(2)
    err = np.abs(got - (np.maximum(want, 0) if c["relu_out"] else want))
    print(f"C1={C1} C2={C2} K={K} {variant}: out max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert none[2].all() and none[1, 3] and not got[none].any() and (slot[none] == 255).all()
    chosen = np.take_along_axis(y, np.minimum(slot, K - 1)[:, :, None, :], 2)[:, :, 0]
    assert ((slot < K) & (chosen >= want - 2 * bound))[~none].all()
    assert K <= 32 or ((slot >= 32) & (slot < K)).any()  # (winners in the second window of staged slots)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C1,C2", SHAPES)
def test_backward(C1, C2, K, variant):
    c = _case(C1, C2, K, variant)
    names = [n for n in GRADS if c[n] is not None]

    def grads():
        t = _tensors(c)
        out, arg = _run({**t, **{n: t[n].requires_grad_(True) for n in names}}, c["relu_out"])
        return (out, arg) + torch.autograd.grad(out, [t[n] for n in names], t["g"])

    first, second = grads(), grads()
    torch.use_deterministic_algorithms(True)
    try:
        third = grads()
    finally:
        torch.use_deterministic_algorithms(False)
    back, s = ref.backward(c["x"], c["idx"], c["weight"], c["center"], c["lengths"], c["g"], first[0].detach().cpu().numpy(),
                           first[1].cpu().numpy(), c["relu_out"])
    assert s[0, HUB] >= L and not s[:, LONELY].any()  # (the hub: every row of cloud 0 refers to it)
    rows = N * L + -(-N * L // 32)
    ts = dict(x=s[..., None] + C2, center=K + C2, weight=rows, bias=rows)
    got = {}
    for name, a, b, d in zip(names, first[2:], second[2:], third[2:]):
        assert _same_bytes(a, b) and _same_bytes(a, d), name
        got[name] = a.cpu().numpy()
        want, mag = back[name]
        bound = (1 + 2.0 ** -6) * (ts[name] + 2) * U * mag
        err = np.abs(got[name].astype(np.float64) - want)
        print(f"C1={C1} C2={C2} K={K} {variant}: grad {name} max err / bound = "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert got[name].shape == want.shape and (err <= bound).all(), name
    assert not got["x"][:, LONELY].any() and not got["x"][2].any()


def test_boundary_rejects_a_short_and_a_null_workspace(monkeypatch):
    from pytorch3d_pointops_amd import _C_neighbor_mlp

    c = _case(24, 40, 3, "full")
    t = _tensors(c)
    out, arg = _C_neighbor_mlp.neighbor_mlp_max(t["x"], t["idx"], t["weight"], t["bias"], t["center"], t["lengths"], True)
    args = (t["g"], t["x"], t["idx"], t["weight"], t["center"], t["lengths"], out, arg, True)
    plain = _C_neighbor_mlp.neighbor_mlp_max_backward(*args)
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=declared_prototypes()) as ct:
        ct.watch(out=out, arg=arg, **{n: v for n, v in t.items() if n != "bias"})
        got = _C_neighbor_mlp.neighbor_mlp_max_backward(*args)
    ct.assert_all_clear()
    entry = "pointops_neighbor_mlp_max_backward"
    assert {(n, how) for n, _, how in ct.rejections} == {(entry, "short"), (entry, "null")}
    assert [b.kind for b in ct.buffers] == ["out", "out", "out", "out", "workspace"]
    assert all(_same_bytes(a, b) for a, b in zip(got, plain))  # (test_backward holds these to their bar)
