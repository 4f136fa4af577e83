"""neighbor_mlp_max with a second hidden layer (weight2; csrc/neighbor_mlp2_16.hip) against tests/neighbor_mlp2_ref.py on
the table of test_neighbor_conv_gpu.py.  The inputs are rounded to T BEFORE they go to the reference; u_T = 2^-9 (bf16) or
2^-11 (fp16); every bound is (1 + 2^-6) (c u_T + (t + 2) 2^-23) mag.

Forward: the one-layer 16-bit bound has 2 u_T (h1's rounding is exact in the reference; the terms are the rounding of the
result and the slack of comparing against a maximum of rounded candidates) and the chain C1 + 1.  Here h2 is rounded to T
once more, and its error passes through weight2 with magnitude at most mag: c = 3; the fp32 chains of the two stages add:
t + 2 = (C1 + 1) + (C2 + 1) + 2.  mag = (|h1| @ |weight| + |bias|) @ |weight2| + |bias2|, maximised over the row's valid
slots.
Backward: c counts the roundings to T the header states on the gradient's path as the forward bound does: 2 u_T for the
result (the one-layer tests' term: a single bfloat16 rounding is 2^-8 = 2 u_T relative, so no implementation can meet
1 u_T -- two addends of one sign already miss it), plus one u_T for each intermediate that passes through a 16-bit matrix
operand or the 16-bit workspace -- grad_x 4 (the result, e2 as a matrix operand, e1 in the workspace), grad_center and
grad_weight 3 (the result, e2), grad_weight2 3 (the result, h2), grad_bias and grad_bias2 2 (fp32 sums, the result): at
most 5 -- and t the longest fp32 chain: grad_x s + C2 + C3 (s entries of the target row, the two dot products),
grad_center K + C2 + C3, grad_weight and grad_bias N L K + P (every pair once, then the P partial sums), grad_weight2 and
grad_bias2 N L + P (one non-zero e3 per row and column).  P = 4 ceil(N L / 32): a workgroup per 32 rows here, and at most
4 partial planes each.  The hidden mask h2 > 0 must be determined: `amb` of the reference is empty for every case (a
condition on the inputs, asserted; never a reason to widen a bound).  With normal inputs an entry is ambiguous with
probability about (C1 + 2) 2^-23 sqrt(C1): ~1.4e-4 at C1 = 128, i.e. ~0.4 per column of weight and tens per case at the
large shapes, so no seed of a whole case is clean; `_case` instead redraws, from the case's own generator, exactly the
columns of weight that have an ambiguous entry until none has one (two or three rounds).
(C1, C2, C3): a half-filled 16-deep step with padded columns; tails in all three dimensions; the PointNet++ shape; the
largest resident fragments with two column blocks per wave; wide to narrow (C3 <= 64: the 64-row tile).  K = 1, 3: partial
groups; K = 40 re-stages the window with the running best carried over."""
import functools

import numpy as np
import pytest
import torch

import buffers
import neighbor_mlp2_ref as ref
from test_boundary_cpu import declared_prototypes
from test_neighbor_conv_gpu import HUB, LONELY, L, M, N, _same_bytes, _table

pytestmark = pytest.mark.gpu

UNIT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
SHAPES, KS, VARIANTS = ((8, 8, 8), (24, 40, 72), (64, 64, 128), (128, 128, 256), (128, 32, 8)), (1, 3, 20, 40), ("plain", "full")
GRADS = ("x", "weight", "bias", "weight2", "bias2", "center")
ROUNDINGS = dict(x=4, center=3, weight=3, bias=2, weight2=3, bias2=2)
PARTS = 4 * -(-N * L // 32)
DTYPES = pytest.mark.parametrize("dtype", list(UNIT), ids=["bf16", "fp16"])


@functools.lru_cache(maxsize=None)
def _case(dtype, C1, C2, C3, K, variant):
    """The inputs (CPU tensors of `dtype`), their exact values as float32 arrays and the reference's forward, once."""
    idx, lengths = _table(K)
    rng = np.random.default_rng(1000 * C1 + 10 * C2 + C3 + K)
    shapes = dict(x=(N, M, C1), weight=(C1, C2), bias=(C2,), weight2=(C2, C3), bias2=(C3,), center=(N, L, C1),
                  g=(N, L, C3))
    t = {n: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dtype) for n, s in shapes.items()}
    if variant == "plain":
        t["bias"] = t["bias2"] = t["center"] = None
    for _ in range(64):  # redraw the columns of weight that leave a hidden pre-activation ambiguous (see the docstring)
        a = {n: None if v is None else v.float().numpy() for n, v in t.items()}
        cols = ref._layers(a["x"], idx, a["weight"], a["bias"], a["center"], lengths, dtype)[5].any((0, 1, 2))
        if not cols.any():
            break
        t["weight"][:, cols] = torch.from_numpy(rng.standard_normal((C1, int(cols.sum()))).astype(np.float32)).to(dtype)
    y, mag, ok, amb = ref.forward(a["x"], idx, a["weight"], a["bias"], a["weight2"], a["bias2"], a["center"], lengths, dtype)
    t.update(idx=torch.from_numpy(np.array(idx)), lengths=torch.from_numpy(np.array(lengths)))
    return dict(t=t, a=a, idx=idx, lengths=lengths, y=y, mag=mag, ok=ok, amb=amb, relu_out=variant == "full")


def _tensors(c):
    return {n: None if v is None else v.cuda() for n, v in c["t"].items()}


def _run(t, relu_out):
    from pytorch3d_pointops_amd.functions import neighbor_mlp_max

    return neighbor_mlp_max(t["x"], t["idx"], t["weight"], t["bias"], t["center"], t["lengths"], relu_out, return_arg=True,
                            weight2=t["weight2"], bias2=t["bias2"])


def _bound(dtype, c, t, mag):
    return (1 + 2.0 ** -6) * (c * UNIT[dtype] + (t + 2) * 2.0 ** -23) * mag


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C1,C2,C3", SHAPES)
@DTYPES
def test_forward(dtype, C1, C2, C3, K, variant):
    from pytorch3d_pointops_amd import _C_neighbor_mlp

    c = _case(dtype, C1, C2, C3, K, variant)
    assert not c["amb"].any()
    t = _tensors(c)
    out, arg = _run(t, c["relu_out"])
    assert out.dtype == dtype and out.shape == (N, L, C3) and arg.dtype == torch.uint8 and arg.shape == out.shape
    for other in (_run(t, c["relu_out"]), _C_neighbor_mlp.neighbor_mlp2_max16(
            t["x"], t["idx"], t["weight"], t["bias"], t["weight2"], t["bias2"], t["center"], t["lengths"], c["relu_out"])):
        assert _same_bytes(out, other[0]) and _same_bytes(arg, other[1])
    got, slot = out.float().cpu().numpy().astype(np.float64), arg.cpu().numpy().astype(np.int64)
    ok, none = c["ok"][..., None], ~c["ok"].any(2)
    y = np.where(ok, c["y"], -np.inf)
    want = np.where(none[..., None], 0, y.max(2))
    bound = _bound(dtype, 3, C1 + C2 + 2, np.where(ok, c["mag"], 0).max(2))
    err = np.abs(got - (np.maximum(want, 0) if c["relu_out"] else want))
    print(f"{dtype} {C1},{C2},{C3} K={K} {variant}: out max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert none[2].all() and none[1, 3] and not got[none].any() and (slot[none] == 255).all()
    chosen = np.take_along_axis(y, np.minimum(slot, K - 1)[:, :, None, :], 2)[:, :, 0]
    assert ((slot < K) & (chosen >= want - 2 * bound))[~none].all()
    assert K <= 32 or ((slot >= 32) & (slot < K)).any()  # (winners in the second window of staged slots)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C1,C2,C3", SHAPES)
@DTYPES
def test_backward(dtype, C1, C2, C3, K, variant):
    c = _case(dtype, C1, C2, C3, K, variant)
    assert not c["amb"].any()
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
    back, s = ref.backward(a["x"], c["idx"], a["weight"], a["bias"], a["weight2"], a["center"], c["lengths"], a["g"],
                           first[0].detach().float().cpu().numpy(), first[1].cpu().numpy(), c["relu_out"], dtype)
    assert s[0, HUB] >= L and not s[:, LONELY].any()  # (the hub: every row of cloud 0 refers to it)
    pairs, rows = N * L * K + PARTS, N * L + PARTS
    ts = dict(x=s[..., None] + C2 + C3, center=K + C2 + C3, weight=pairs, bias=pairs, weight2=rows, bias2=rows)
    got = {}
    for name, ga, gb, gd in zip(names, first[2:], second[2:], third[2:]):
        assert ga.dtype == dtype and _same_bytes(ga, gb) and _same_bytes(ga, gd), name
        got[name] = ga.float().cpu().numpy()
        want, mag = back[name]
        bound = _bound(dtype, ROUNDINGS[name], ts[name], mag)
        err = np.abs(got[name].astype(np.float64) - want)
        print(f"{dtype} {C1},{C2},{C3} K={K} {variant}: grad {name} max err / bound = "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert got[name].shape == want.shape and (err <= bound).all(), name
    assert not got["x"][:, LONELY].any() and not got["x"][2].any()


def test_boundary_rejects_a_short_and_a_null_workspace(monkeypatch):
    from pytorch3d_pointops_amd import _C_neighbor_mlp as nm

    t = _tensors(_case(torch.bfloat16, 24, 40, 72, 3, "full"))
    fwd = (t["x"], t["idx"], t["weight"], t["bias"], t["weight2"], t["bias2"], t["center"], t["lengths"], True)
    out, arg = nm.neighbor_mlp2_max16(*fwd)
    bwd = (t["g"], t["x"], t["idx"], t["weight"], t["bias"], t["weight2"], t["center"], t["lengths"], out, arg, True)
    want = (out, arg, *nm.neighbor_mlp2_max16_backward(*bwd))
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=declared_prototypes()) as ct:
        ct.watch(out=out, arg=arg, **t)
        got = (*nm.neighbor_mlp2_max16(*fwd), *nm.neighbor_mlp2_max16_backward(*bwd))
    ct.assert_all_clear()
    entries = ("pointops_neighbor_mlp2_max16", "pointops_neighbor_mlp2_max16_backward")
    assert {(n, how) for n, _, how in ct.rejections} == {(e, how) for e in entries for how in ("short", "null")}
    assert [b.kind for b in ct.buffers] == ["out", "out", "workspace"] + ["out"] * 6 + ["workspace"]
    assert all(_same_bytes(a, b) for a, b in zip(got, want))  # the accepted calls ran
