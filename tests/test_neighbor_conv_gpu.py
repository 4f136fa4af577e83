"""neighbor_conv on the device against the float64 loops of tests/neighbor_conv_ref.py; u = 2^-24, every bound is
(1 + 2^-6) (t + 2) u mag with t the rounded operations of the result's chain (include/pointops_amd.h):
  out          t = n + P Cin: the n fmaf of A over the row's valid slots, the P Cin fmaf of the product
  grad_x       t = s + P Cout: the s fmaf of B over the target row's entries, the P Cout fmaf of the product
  grad_weight  t = K + N L + ceil(N L / 32): at most K fmaf in A, one fmaf per row, one add per chunk
  grad_coeff   t = Cout + 9: the Cout fmaf of T, then a product, three adds in the lane and at most five in the tree
(Cin, Cout): one k-step pair with 28 padded columns, an output block with a tail, one block per wave, the register limits
on either side; K = 20 with P = 15: two to four passes over the lists; the hub's inverted list spans two windows."""
import functools

import numpy as np
import pytest
import torch

import buffers
import neighbor_conv_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N, L, M = 3, 37, 29
SHAPES, KS, MODES = ((4, 4), (12, 40), (64, 64), (128, 32), (32, 128)), (1, 3, 20), ("onehot", "p1", "p15")
HUB, LONELY = 11, 7


@functools.lru_cache(maxsize=None)
def _table(K):
    """-1 padding, a cloud with lengths < K, a row without a valid slot, a cloud of length 0, LONELY unreferenced, a HUB."""
    rng = np.random.default_rng(100 + K)
    idx = rng.integers(0, M, (N, L, K))
    idx[idx == LONELY] = LONELY + 1
    idx[0, 5:9, max(1, K // 2):] = -1
    idx[0, :, 0] = HUB
    idx[1, 3, :] = -1
    lengths = np.array([M, K - 1, 0])
    idx.setflags(write=False), lengths.setflags(write=False)
    return idx, lengths


@functools.lru_cache(maxsize=None)
def _case(Cin, Cout, K, mode):
    """The inputs and the reference's forward and backward, computed once."""
    idx, lengths = _table(K)
    P = {"onehot": K, "p1": 1, "p15": 15}[mode]
    rng = np.random.default_rng(1000 * Cin + Cout + K)
    x, w, g = (rng.standard_normal(s).astype(np.float32) for s in ((N, M, Cin), (P, Cin, Cout), (N, L, Cout)))
    coeff = None if mode == "onehot" else rng.standard_normal((N, L, K, P)).astype(np.float32)
    fwd = ref.forward(x, idx, w, lengths, coeff)
    back, seg = ref.backward(x, idx, w, lengths, coeff, g, fwd)
    for a in (x, w, g, coeff):
        if a is not None:
            a.setflags(write=False)
    return dict(x=x, weight=w, g=g, coeff=coeff, idx=idx, lengths=lengths, P=P, fwd=fwd, back=back, seg=seg)


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _same_bytes(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_forward(Cin, Cout, K, mode):
    from pytorch3d_pointops_amd import _C_neighbor_conv
    from pytorch3d_pointops_amd.functions import neighbor_conv

    c = _case(Cin, Cout, K, mode)
    fwd = c["fwd"]
    tx, ti, tw, tl, tc = _dev(c["x"], c["idx"], c["weight"], c["lengths"], c["coeff"])
    out = neighbor_conv(tx, ti, tw, tl, tc)
    assert out.dtype == torch.float32 and out.shape == (N, L, Cout)
    assert _same_bytes(out, neighbor_conv(tx, ti, tw, tl, tc))
    assert _same_bytes(out, _C_neighbor_conv.neighbor_conv(tx, ti, tw, tl, tc))
    got = out.cpu().numpy()
    bound = (1 + 2.0 ** -6) * (fwd["n"][..., None] + c["P"] * Cin + 2) * U * fwd["mag"]
    err = np.abs(got.astype(np.float64) - fwd["out"])
    print(f"Cin={Cin} Cout={Cout} K={K} {mode}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert not fwd["n"][2].any() and not fwd["n"][1, 3] and not got[fwd["n"] == 0].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("Cin,Cout", SHAPES)
def test_backward(Cin, Cout, K, mode):
    from pytorch3d_pointops_amd.functions import neighbor_conv

    c = _case(Cin, Cout, K, mode)
    names = ("x", "weight") + (("coeff",) if c["coeff"] is not None else ())

    def grads():
        t = dict(zip(("x", "weight", "coeff", "idx", "lengths", "g"),
                     _dev(c["x"], c["weight"], c["coeff"], c["idx"], c["lengths"], c["g"])))
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
        assert _same_bytes(a, b) and _same_bytes(a, d), name
        got[name] = a.cpu().numpy()
        want, mag = c["back"][name]
        bound = (1 + 2.0 ** -6) * (ts[name] + 2) * U * mag
        err = np.abs(got[name].astype(np.float64) - want)
        print(f"Cin={Cin} Cout={Cout} K={K} {mode}: grad {name} max err / bound = "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all(), name
    assert not got["x"][:, LONELY].any() and not got["x"][2].any()
    if "coeff" in got:
        assert not got["coeff"][~ref.valid_slots(c["idx"], c["lengths"], M)].any() and not got["coeff"][2].any()


def test_boundary_rejects_a_short_and_a_null_workspace(monkeypatch):
    from pytorch3d_pointops_amd import _C_neighbor_conv

    c = _case(12, 40, 3, "p15")
    names = ("g", "x", "idx", "weight", "lengths", "coeff")
    t = dict(zip(names, _dev(*[c[n] for n in names])))
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=declared_prototypes()) as ct:
        ct.watch(**t)
        got = _C_neighbor_conv.neighbor_conv_backward(t["g"], t["x"], t["idx"], t["weight"], t["lengths"], t["coeff"])
    ct.assert_all_clear()
    entry = "pointops_neighbor_conv_backward"
    assert {(n, how) for n, _, how in ct.rejections} == {(entry, "short"), (entry, "null")}
    assert [b.kind for b in ct.buffers] == ["out", "out", "out", "workspace"]
    # (the accepted call ran: test_backward holds these to their bar)
    for a, name in zip(got, ("x", "weight", "coeff")):
        assert np.allclose(a.cpu().numpy(), c["back"][name][0], rtol=1e-3, atol=1e-3)
