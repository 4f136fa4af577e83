"""neighbor_mlp_max on bfloat16 / float16 features (csrc/neighbor_mlp16.hip) against tests/neighbor_mlp16_ref.py, on the
table of test_neighbor_conv_gpu.py.  The inputs are rounded to T BEFORE they go to the reference.  Every bound is the
16-bit kernels' own (test_neighbor_conv16_gpu.py), (1 + 2^-6) (2 u_T + (t + 2) 2^-23) mag with u_T = 2^-9 (bf16) or 2^-11
(fp16), and t the chain length of test_neighbor_mlp_gpu.py: out C1 + 1 (against the maximum of the bound over the row's
valid slots), grad_x s + C2, grad_center K + C2, grad_weight and grad_bias N L + ceil(N L / 32).  arg is 255 exactly
where no slot is valid, else a valid slot whose float64 y is within twice the bound of the maximum; the backward
reference takes the device's out and arg.
(C1, C2): a half-filled 16-deep step with padded columns, k and column tails, two slots per barrier pair, the largest
resident B and the small tile, two column slices and the 8-ballot path; K = 1, 3: partial groups; K = 40 re-stages the
window with the running best carried over."""
import functools

import numpy as np
import pytest
import torch

import buffers
import neighbor_mlp16_ref as ref
from test_boundary_cpu import declared_prototypes
from test_neighbor_conv_gpu import HUB, LONELY, L, M, N, _same_bytes, _table

pytestmark = pytest.mark.gpu

UNIT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
SHAPES, KS, VARIANTS = ((8, 8), (24, 40), (64, 64), (256, 32), (32, 256)), (1, 3, 20, 40), ("plain", "full")
GRADS = ("x", "weight", "bias", "center")
DTYPES = pytest.mark.parametrize("dtype", list(UNIT), ids=["bf16", "fp16"])


@functools.lru_cache(maxsize=None)
def _case(dtype, C1, C2, K, variant):
    """The inputs (CPU tensors of `dtype`), their exact values as float32 arrays and the reference's forward, once."""
    idx, lengths = _table(K)
    rng = np.random.default_rng(1000 * C1 + C2 + K)
    shapes = dict(x=(N, M, C1), weight=(C1, C2), bias=(C2,), center=(N, L, C1), g=(N, L, C2))
    t = {n: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dtype) for n, s in shapes.items()}
    if variant == "plain":
        t["bias"] = t["center"] = None
    a = {n: None if v is None else v.float().numpy() for n, v in t.items()}
    y, mag, ok = ref.forward(a["x"], idx, a["weight"], a["bias"], a["center"], lengths, dtype)
    t.update(idx=torch.from_numpy(np.array(idx)), lengths=torch.from_numpy(np.array(lengths)))
    return dict(t=t, a=a, idx=idx, lengths=lengths, y=y, mag=mag, ok=ok, relu_out=variant == "full")


def _tensors(c):
    return {n: None if v is None else v.cuda() for n, v in c["t"].items()}


def _run(t, relu_out):
    from pytorch3d_pointops_amd.functions import neighbor_mlp_max

    return neighbor_mlp_max(t["x"], t["idx"], t["weight"], t["bias"], t["center"], t["lengths"], relu_out, return_arg=True)


def _bound(dtype, t, mag):
    return (1 + 2.0 ** -6) * (2 * UNIT[dtype] + (t + 2) * 2.0 ** -23) * mag


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C1,C2", SHAPES)
@DTYPES
def test_forward(dtype, C1, C2, K, variant):
    from pytorch3d_pointops_amd import _C_neighbor_mlp

    c = _case(dtype, C1, C2, K, variant)
    t = _tensors(c)
    out, arg = _run(t, c["relu_out"])
    assert out.dtype == dtype and out.shape == (N, L, C2) and arg.dtype == torch.uint8 and arg.shape == out.shape
    for other in (_run(t, c["relu_out"]), _C_neighbor_mlp.neighbor_mlp_max16(
            t["x"], t["idx"], t["weight"], t["bias"], t["center"], t["lengths"], c["relu_out"])):
        assert _same_bytes(out, other[0]) and _same_bytes(arg, other[1])
    got, slot = out.float().cpu().numpy().astype(np.float64), arg.cpu().numpy().astype(np.int64)
    ok, none = c["ok"][..., None], ~c["ok"].any(2)
    y = np.where(ok, c["y"], -np.inf)
    want = np.where(none[..., None], 0, y.max(2))
    bound = _bound(dtype, C1 + 1, np.where(ok, c["mag"], 0).max(2))
    err = np.abs(got - (np.maximum(want, 0) if c["relu_out"] else want))
    print(f"{dtype} C1={C1} C2={C2} K={K} {variant}: out max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert none[2].all() and none[1, 3] and not got[none].any() and (slot[none] == 255).all()
    chosen = np.take_along_axis(y, np.minimum(slot, K - 1)[:, :, None, :], 2)[:, :, 0]
    assert ((slot < K) & (chosen >= want - 2 * bound))[~none].all()
    assert K <= 32 or ((slot >= 32) & (slot < K)).any()  # (winners in the second window of staged slots)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C1,C2", SHAPES)
@DTYPES
def test_backward(dtype, C1, C2, K, variant):
    c = _case(dtype, C1, C2, K, variant)
    names = [n for n in GRADS if c["t"][n] is not None]

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
    a = c["a"]
    back, s = ref.backward(a["x"], c["idx"], a["weight"], a["center"], c["lengths"], a["g"],
                           first[0].detach().float().cpu().numpy(), first[1].cpu().numpy(), c["relu_out"], dtype)
    assert s[0, HUB] >= L and not s[:, LONELY].any()  # (the hub: every row of cloud 0 refers to it)
    rows = N * L + -(-N * L // 32)
    ts = dict(x=s[..., None] + C2, center=K + C2, weight=rows, bias=rows)
    got = {}
    for name, ga, gb, gd in zip(names, first[2:], second[2:], third[2:]):
        assert ga.dtype == dtype and _same_bytes(ga, gb) and _same_bytes(ga, gd), name
        got[name] = ga.float().cpu().numpy()
        want, mag = back[name]
        bound = _bound(dtype, ts[name], mag)
        err = np.abs(got[name].astype(np.float64) - want)
        print(f"{dtype} C1={C1} C2={C2} K={K} {variant}: grad {name} max err / bound = "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert got[name].shape == want.shape and (err <= bound).all(), name
    assert not got["x"][:, LONELY].any() and not got["x"][2].any()


def test_boundary_rejects_a_short_and_a_null_workspace(monkeypatch):
    from pytorch3d_pointops_amd import _C_neighbor_mlp as nm

    t = _tensors(_case(torch.bfloat16, 24, 40, 3, "full"))
    fwd = (t["x"], t["idx"], t["weight"], t["bias"], t["center"], t["lengths"], True)
    out, arg = nm.neighbor_mlp_max16(*fwd)
    bwd = (t["g"], t["x"], t["idx"], t["weight"], t["center"], t["lengths"], out, arg, True)
    want = (out, arg, *nm.neighbor_mlp_max16_backward(*bwd))
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=declared_prototypes()) as ct:
        ct.watch(out=out, arg=arg, **t)
        got = (*nm.neighbor_mlp_max16(*fwd), *nm.neighbor_mlp_max16_backward(*bwd))
    ct.assert_all_clear()
    entries = ("pointops_neighbor_mlp_max16", "pointops_neighbor_mlp_max16_backward")
    assert {(n, how) for n, _, how in ct.rejections} == {(e, how) for e in entries for how in ("short", "null")}
    assert [b.kind for b in ct.buffers] == ["out", "out", "workspace", "out", "out", "out", "out", "workspace"]
    assert all(_same_bytes(a, b) for a, b in zip(got, want))  # the accepted calls ran
