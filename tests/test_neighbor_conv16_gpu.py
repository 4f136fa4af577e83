"""neighbor_conv on bfloat16 / float16 features (csrc/neighbor_conv16.hip) against the float64 loops of
tests/neighbor_conv_ref.py, on the tables of test_neighbor_conv_gpu.py.  The inputs are rounded to T BEFORE they go to the
reference: what is tested is the kernel, not the quantisation of its inputs.  Every bound is
(1 + 2^-6) (2 u_T + (t + 2) 2^-23) mag, u_T = 2^-9 (bf16) or 2^-11 (fp16): one rounding of A (or B, or nothing) to T, one
rounding of the result to T, and fp32 accumulation at 2^-23 per addend (the wider unit, because the rounding inside a
16-deep step is not documented); t is the float32 test's chain length: n + P Cin, s + P Cout, K + N L + ceil(N L / 32),
Cout + 9.  (Cin, Cout): one half-filled k-step with padded columns, k and column tails, the 64-row tile, the register /
LDS limits on either side; K = 20 with P = 15: two to four (at 256 channels eight) chunks."""
import functools

import numpy as np
import pytest
import torch

import buffers
import neighbor_conv_ref as ref
import test_neighbor_conv_gpu as f32
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

N, L, M, HUB, LONELY = f32.N, f32.L, f32.M, f32.HUB, f32.LONELY
UNIT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}
SHAPES = ((8, 8), (24, 40), (64, 64), (256, 32), (32, 256))
DTYPES = pytest.mark.parametrize("dtype", list(UNIT), ids=["bf16", "fp16"])


@functools.lru_cache(maxsize=None)
def _case(dtype, Cin, Cout, K, mode):
    """The inputs (CPU tensors of `dtype`) and the reference's forward and backward on their exact values, computed once."""
    idx, lengths = f32._table(K)
    P = {"onehot": K, "p1": 1, "p15": 15}[mode]
    rng = np.random.default_rng(1000 * Cin + Cout + K)
    shapes = dict(x=(N, M, Cin), weight=(P, Cin, Cout), g=(N, L, Cout), coeff=(N, L, K, P))
    t = {n: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dtype) for n, s in shapes.items()}
    if mode == "onehot":
        t["coeff"] = None
    a = {n: None if v is None else v.float().numpy() for n, v in t.items()}
    fwd = ref.forward(a["x"], idx, a["weight"], lengths, a["coeff"])
    back, seg = ref.backward(a["x"], idx, a["weight"], lengths, a["coeff"], a["g"], fwd)
    t.update(idx=torch.from_numpy(np.array(idx)), lengths=torch.from_numpy(np.array(lengths)))
    return dict(t=t, idx=idx, lengths=lengths, P=P, fwd=fwd, back=back, seg=seg)


def _dev(c, *names):
    return [None if c["t"][n] is None else c["t"][n].cuda() for n in names]


def _check(what, got, want, mag, t, dtype):
    bound = (1 + 2.0 ** -6) * (2 * UNIT[dtype] + (t + 2) * 2.0 ** -23) * mag
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("mode", f32.MODES)
@pytest.mark.parametrize("K", f32.KS)
@pytest.mark.parametrize("Cin,Cout", SHAPES)
@DTYPES
def test_forward(dtype, Cin, Cout, K, mode):
    from pytorch3d_pointops_amd import _C_neighbor_conv
    from pytorch3d_pointops_amd.functions import neighbor_conv

    c = _case(dtype, Cin, Cout, K, mode)
    fwd = c["fwd"]
    args = _dev(c, "x", "idx", "weight", "lengths", "coeff")
    out = neighbor_conv(*args)
    assert out.dtype == dtype and out.shape == (N, L, Cout)
    assert f32._same_bytes(out, neighbor_conv(*args))
    assert f32._same_bytes(out, _C_neighbor_conv.neighbor_conv16(*args))
    got = out.float().cpu().numpy()
    _check(f"{dtype} Cin={Cin} Cout={Cout} K={K} {mode}", got, fwd["out"], fwd["mag"],
           fwd["n"][..., None] + c["P"] * Cin, dtype)
    assert not fwd["n"][2].any() and not fwd["n"][1, 3] and not got[fwd["n"] == 0].any()


@pytest.mark.parametrize("mode", f32.MODES)
@pytest.mark.parametrize("K", f32.KS)
@pytest.mark.parametrize("Cin,Cout", SHAPES)
@DTYPES
def test_backward(dtype, Cin, Cout, K, mode):
    from pytorch3d_pointops_amd.functions import neighbor_conv

    c = _case(dtype, Cin, Cout, K, mode)
    names = ("x", "weight") + (("coeff",) if mode != "onehot" else ())

    def grads():
        t = dict(zip(("x", "weight", "coeff", "idx", "lengths", "g"),
                     _dev(c, "x", "weight", "coeff", "idx", "lengths", "g")))
        leaves = [t[n].requires_grad_(True) for n in names]
        return torch.autograd.grad(neighbor_conv(t["x"], t["idx"], t["weight"], t["lengths"], t["coeff"]), leaves, t["g"])

    first, second = grads(), grads()
    torch.use_deterministic_algorithms(True)
    try:
        third = grads()
    finally:
        torch.use_deterministic_algorithms(False)
    seg = c["seg"]
    assert seg[0, HUB] > 32 and seg[0, HUB] == seg[0].max() and not seg[:, LONELY].any()
    ts = dict(x=seg[..., None] + c["P"] * Cout, weight=K + N * L + -(-N * L // 32), coeff=Cout + 9)
    got = {}
    for name, a, b, d in zip(names, first, second, third):
        assert a.dtype == dtype and f32._same_bytes(a, b) and f32._same_bytes(a, d), name
        got[name] = a.float().cpu().numpy()
        _check(f"{dtype} Cin={Cin} Cout={Cout} K={K} {mode}: grad {name}", got[name], *c["back"][name], ts[name], dtype)
    assert not got["x"][:, LONELY].any() and not got["x"][2].any()
    if "coeff" in got:
        assert not got["coeff"][~ref.valid_slots(c["idx"], c["lengths"], M)].any() and not got["coeff"][2].any()


def test_boundary_rejects_a_short_and_a_null_workspace(monkeypatch):
    from pytorch3d_pointops_amd import _C_neighbor_conv as nc

    c = _case(torch.bfloat16, 24, 40, 3, "p15")
    g, x, idx, weight, lengths, coeff = _dev(c, "g", "x", "idx", "weight", "lengths", "coeff")
    want = (nc.neighbor_conv16(x, idx, weight, lengths, coeff),
            *nc.neighbor_conv16_backward(g, x, idx, weight, lengths, coeff))
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=declared_prototypes()) as ct:
        ct.watch(g=g, x=x, idx=idx, weight=weight, lengths=lengths, coeff=coeff)
        got = (nc.neighbor_conv16(x, idx, weight, lengths, coeff),
               *nc.neighbor_conv16_backward(g, x, idx, weight, lengths, coeff))
    ct.assert_all_clear()
    entries = ("pointops_neighbor_conv16", "pointops_neighbor_conv16_backward")
    assert {(n, how) for n, _, how in ct.rejections} == {(e, how) for e in entries for how in ("short", "null")}
    assert [b.kind for b in ct.buffers] == ["out", "workspace", "out", "out", "out", "workspace"]
    assert all(f32._same_bytes(a, b) for a, b in zip(got, want))  # the accepted calls ran
