"""neighbor_attention on the device against the float64 loops of tests/neighbor_attention_ref.py; u = 2^-24, n = the counted
slots.  Forward: |out - ref| <= (1 + 2^-6) [2 E + (4 n + 8) u] sum_k w_k |v_kc| + 2^-120 max |v|, E = max_k ((D + 2) u A_k +
u |s_k - m| + 2 u): an unfused dot of D products, the scale and the bias; one rounding on the shifted logit; expf, documented
2 u; a normalisation and an accumulate of n terms, at most 2 n rescales.  lse within E + (n + 4) u (1 + |lse|).  Backward: 1e-5
of the largest magnitude of each gradient tensor (the README's bar for accumulated gradients).  (heads, D): one lane per head,
idle lanes, several heads per group, one full group, chunks with a tail head, a head that is a wave; K = 20 at (1, 4): two tiles."""
import functools

import numpy as np
import pytest
import torch

import buffers
import neighbor_attention_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N, L, M = 3, 37, 29
SHAPES, KS = ((1, 4), (3, 4), (2, 16), (8, 32), (3, 128), (1, 256)), (1, 3, 20)
HUB, LONELY = 11, 7
ONE_LEFT, NONE_LEFT, WIDE = (0, 20), (0, 21), (0, 22)  # rows of cloud 0: bias -inf but for slot 0 / everywhere; +-60 logits


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
def _case(heads, D, K, with_bias, wide):
    """The inputs, the fp32 scale and the reference's forward and backward, computed once.  `wide`: row WIDE of q is one
    channel per head, scaled so that the row's logits (before the bias) lie in [-120, 120] and, once both signs occur, span
    120: about +-60 (A_k = |s_k| there, so E stays small)."""
    idx, lengths = _table(K)
    rng = np.random.default_rng(1000 * heads + D + K)
    q, k, v, g = (rng.standard_normal(s).astype(np.float32) for s in
                  ((N, L, heads * D), (N, M, heads * D), (N, M, heads * D), (N, L, heads * D)))
    scale = float(np.float32(1.0 / np.sqrt(D)))
    if wide:
        first = k[0][idx[WIDE]].reshape(K, heads, D)[:, :, 0]  # (K, heads): channel 0 of every head of the row's slots
        q[WIDE] = 0.0
        q[WIDE].reshape(heads, D)[:, 0] = 120.0 / (scale * (np.maximum(first.max(0), 0) - np.minimum(first.min(0), 0)))
    bias = None
    if with_bias:
        bias = rng.standard_normal((N, L, K, heads)).astype(np.float32)
        bias[ONE_LEFT][1:] = -np.inf
        bias[NONE_LEFT] = -np.inf
    fwd = ref.forward(q, k, v, idx, lengths, bias, heads, scale)
    back = ref.backward(q, k, v, idx, lengths, heads, scale, g, fwd)
    for a in (q, k, v, g, bias):
        if a is not None:
            a.setflags(write=False)
    return dict(q=q, k=k, v=v, g=g, bias=bias, idx=idx, lengths=lengths, scale=scale, fwd=fwd, back=back)


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _same_bytes(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("with_bias", [False, True], ids=["no_bias", "bias"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("heads,D", SHAPES)
def test_forward(heads, D, K, with_bias):
    from pytorch3d_pointops_amd import _C_neighbor_attention
    from pytorch3d_pointops_amd.functions import neighbor_attention

    c = _case(heads, D, K, with_bias, True)
    fwd = c["fwd"]
    tq, tk, tv, ti, tl, tb = _dev(c["q"], c["k"], c["v"], c["idx"], c["lengths"], c["bias"])
    out = neighbor_attention(tq, tk, tv, ti, tl, heads, tb)  # the default scale
    again, lse = _C_neighbor_attention.neighbor_attention(tq, tk, tv, ti, tl, tb, heads, c["scale"])
    assert out.dtype == torch.float32 and out.shape == (N, L, heads * D) and _same_bytes(out, again)
    n = fwd["counted"].sum(2)  # (N, L, heads)
    E = np.where(fwd["counted"], (D + 2) * U * fwd["A"] + U * np.abs(fwd["shift"]) + 2 * U, 0.0).max(2, initial=0.0)
    assert E.max() <= 2.0 ** -8 and (K < 20 or np.abs(fwd["shift"][WIDE]).max() > 100)
    bound = (1 + 2.0 ** -6) * np.repeat(2 * E + (4 * n + 8) * U, D, axis=2) * fwd["mag"] + 2.0 ** -120 * np.abs(c["v"]).max()
    err = np.abs(out.cpu().numpy().astype(np.float64) - fwd["out"])
    got_lse = lse.cpu().numpy().astype(np.float64)
    has = n > 0
    lse_err = np.abs(got_lse[has] - fwd["lse"][has])
    lse_bound = (E + (n + 4) * U * (1 + np.abs(np.where(has, fwd["lse"], 0.0))))[has]
    print(f"heads={heads} D={D} K={K} bias={with_bias}: max err / bound = {np.max(err / bound):.3f}, "
          f"lse {np.max(lse_err / lse_bound, initial=0.0):.3f}")
    assert (err <= bound).all() and (lse_err <= lse_bound).all()
    # rows and heads without weight: the cloud of length 0, the row without a valid slot, the row whose bias is all -inf
    assert not has[2].any() and not has[1, 3].any() and (not with_bias or not has[NONE_LEFT].any())
    assert (got_lse[~has] == -np.inf).all() and not out.cpu().numpy()[np.repeat(~has, D, axis=2)].any()


@pytest.mark.parametrize("with_bias", [False, True], ids=["no_bias", "bias"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("heads,D", SHAPES)
def test_backward(heads, D, K, with_bias):
    from pytorch3d_pointops_amd.functions import neighbor_attention

    def grads(c):
        tq, tk, tv, ti, tl, tb, tg = _dev(c["q"], c["k"], c["v"], c["idx"], c["lengths"], c["bias"], c["g"])
        leaves = [t.requires_grad_(True) for t in (tq, tk, tv, tb) if t is not None]
        return torch.autograd.grad(neighbor_attention(tq, tk, tv, ti, tl, heads, tb, c["scale"]), leaves, tg)

    c = _case(heads, D, K, with_bias, False)
    first, second = grads(c), grads(c)
    torch.use_deterministic_algorithms(True)
    try:
        third = grads(c)
    finally:
        torch.use_deterministic_algorithms(False)
    *want, seg = c["back"]
    assert seg[0, HUB] >= L - 1 and not seg[:, LONELY].any()
    for name, a, b, d, w in zip(("q", "k", "v", "bias"), first, second, third, want):
        assert _same_bytes(a, b) and _same_bytes(a, d), name
        err, top = np.abs(a.cpu().numpy().astype(np.float64) - w).max(), np.abs(w).max()
        rel = float(err / top) if top > 0 else (0.0 if err == 0 else np.inf)  # (K = 1: ds is 0, and must be exactly so)
        print(f"heads={heads} D={D} K={K} bias={with_bias}: grad {name} max error relative to the largest magnitude = {rel:.2e}")
        assert rel <= 1e-5, name

    def exact_zeros(got):
        gq, gk, gv = (t.cpu().numpy() for t in got[:3])
        assert not gk[:, LONELY].any() and not gv[:, LONELY].any()
        assert not gq[2].any() and not gq[1, 3].any() and (not with_bias or not gq[NONE_LEFT].any())
        if with_bias:
            gb = got[3].cpu().numpy()
            assert not gb[~ref.valid_slots(c["idx"], c["lengths"], M)].any() and not gb[NONE_LEFT].any()
            assert not gb[ONE_LEFT][1:].any()

    exact_zeros(first)
    # the +-60 row: finite, and zero where its weight underflows (float64 weight below 1e-46: exp of less than -105)
    wide = _case(heads, D, K, with_bias, True)
    got = grads(wide)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    exact_zeros(got)
    if with_bias:
        gone = wide["fwd"]["w"][WIDE] < 1e-46
        assert not got[3].cpu().numpy()[WIDE][gone].any() and (K < 20 or gone.any())


def test_boundary_rejects_a_short_and_a_null_workspace(monkeypatch):
    from pytorch3d_pointops_amd import _C_neighbor_attention

    heads = 2
    c = _case(heads, 16, 3, True, False)
    names = ("g", "q", "k", "v", "idx", "lengths", "bias")
    t = dict(zip(names, _dev(*[c[n] for n in names])))
    out, lse = _C_neighbor_attention.neighbor_attention(t["q"], t["k"], t["v"], t["idx"], t["lengths"], t["bias"], heads,
                                                        c["scale"])
    with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=declared_prototypes()) as ct:
        ct.watch(out=out, lse=lse, **t)
        got = _C_neighbor_attention.neighbor_attention_backward(
            t["g"], t["q"], t["k"], t["v"], out, lse, t["idx"], t["lengths"], t["bias"], heads, c["scale"],
            need=(True, True, True, True))
    ct.assert_all_clear()
    entry = "pointops_neighbor_attention_backward"
    assert {(n, how) for n, _, how in ct.rejections} == {(entry, "short"), (entry, "null")}
    assert [b.kind for b in ct.buffers] == ["out", "out", "out", "out", "workspace"]
    # (the accepted call ran: test_backward holds these to their bar)
    for a, w in zip(got, c["back"]):
        assert np.allclose(a.cpu().numpy(), w, rtol=1e-3, atol=1e-3)
