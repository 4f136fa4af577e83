"""The scatter sides of the backward passes -- tiled_scatter.h, knn_backward.hip, the backward half of gather.hip and
backward_det.hip -- under every plan, against the float64 references of tests/scatter_ref.py.

EXACT cases (lattice coordinates, integer gradients, max A < 2^22: scatter_ref's docstring): no addition rounds in any
order, so every plan must return the float64 sum cast to fp32, BIT FOR BIT, hubs included -- one dropped or doubled addend
shows.  FLOAT cases: |result - float64 sum| <= bound(n, A, S) per element, from quantities of the reference alone.  No
tolerance here is measured on the GPU.

Every case is a synthetic neighbour table (scatter_ref.table): a hub, both sides of the first tile boundary, ball-query
padding, an empty cloud, a three-row cloud, a full cloud last, l2 < K on one cloud.  Plans are forced with the
POINTOPS_DEBUG knobs of csrc/debug.h: device atomics; LDS tiles with S = 1, 2, 5 row splits and with S so large that the
three-row cloud's and the FULL last cloud's last split have no rows (scatter_ref.empty_split); deterministic=True.
"""
import numpy as np
import pytest
import torch

import cases
import scatter_ref as R
from conftest import bits

pytestmark = pytest.mark.gpu

N, L = R.N_CLOUDS, R.L_ROWS
S_EMPTY = R.empty_split(L)
TILED = {"tiled_s1": 1, "tiled_s2": 2, "tiled_s5": 5, "tiled_empty_splits": S_EMPTY}
ALL_PLANS = ["atomic"] + list(TILED) + ["deterministic"]
WIDE_PLANS = ["atomic", "deterministic"]  # C > 4 has no LDS-tile form


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def choose(monkeypatch, op, plan):
    """Force `plan` for `op` ('knn' | 'gather'); returns (deterministic, S)."""
    if plan == "deterministic":
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
        return True, 1
    if plan == "atomic":
        monkeypatch.setenv("POINTOPS_DEBUG", f"{op}_bwd_mode=atomic")
        return False, 1
    monkeypatch.setenv("POINTOPS_DEBUG", f"{op}_bwd_mode=tiled,{op}_bwd_split={TILED[plan]}")
    return False, TILED[plan]


def differing(got, want32):
    return int((bits(got) != bits(want32)).sum())


def run_knn(dev, monkeypatch, plan, p1, p2, l1, l2, idx, norm, grad):
    from pytorch3d_pointops_amd import _C

    det, S = choose(monkeypatch, "knn", plan)
    g1, g2 = _C.knn_points_backward(G(p1, dev), G(p2, dev), G(l1, dev), G(l2, dev), G(idx, dev), norm, G(grad, dev),
                                    deterministic=det)
    return g1.cpu().numpy(), g2.cpu().numpy(), S


def run_gather(dev, monkeypatch, plan, go, idx, lengths, M):
    from pytorch3d_pointops_amd import _C

    det, S = choose(monkeypatch, "gather", plan)
    gx = _C.gather_neighbors_backward(G(go, dev), G(idx, dev), None if lengths is None else G(lengths, dev), M,
                                      deterministic=det)
    return gx.cpu().numpy(), S


def exact_knn_failures(dev, monkeypatch, plans, C, M, K, norm):
    p1, p2, l1, l2, idx, grad, r = R.exact_knn_inputs(R.case_seed(C, M, K, norm), N, L, K, M, C, norm)
    w1, w2 = r.g1.astype(np.float32), r.g2.astype(np.float32)
    bad = []
    for plan in plans:
        g1, g2, _ = run_knn(dev, monkeypatch, plan, p1, p2, l1, l2, idx, norm, grad)
        d1, d2 = differing(g1, w1), differing(g2, w2)
        if d1 or d2:
            bad.append(f"knn {plan}: {d1} elements of grad_p1, {d2} of grad_p2 differ (max |err| "
                       f"{np.abs(g1 - r.g1).max():g}, {np.abs(g2 - r.g2).max():g})")
    return bad


def exact_gather_failures(dev, monkeypatch, plans, C, M, K):
    bad = []
    for with_lengths in (True, False):
        go, idx, lengths, r = R.exact_gather_inputs(R.case_seed(C, M, K, 2), N, L, K, M, C, with_lengths)
        want = r.gx.astype(np.float32)
        for plan in plans:
            gx, _ = run_gather(dev, monkeypatch, plan, go, idx, lengths, M)
            d = differing(gx, want)
            if d:
                bad.append(f"gather {plan} lengths={with_lengths}: {d} elements of grad_x differ (max |err| "
                           f"{np.abs(gx - r.gx).max():g})")
    return bad


# ------------------------------------------------------------------ exact matrix
@pytest.mark.parametrize("C,name,K,norm", R.matrix_cases(),
                         ids=[f"C{C}-M={name}-K{K}-L{norm}" for C, name, K, norm in R.matrix_cases()])
def test_exact_matrix(dev, monkeypatch, C, name, K, norm):
    """Every M (1, 63, 64, 65, tile - 1, tile, tile + 1, 2 tile + 1) with every C at K = 8; every K (1: the shift = -1
    branch, 3, 8, 21: longer than two 8-entry vector chunks) and both norms (the lattice makes a == b common: the L1 tie)
    at tile + 1; all six plans; knn (grad_p1 and grad_p2) and gather (with and without lengths)."""
    M = R.target_sizes(C)[name]
    bad = exact_knn_failures(dev, monkeypatch, ALL_PLANS, C, M, K, norm)
    if norm == 2:  # (the gather side has no norm)
        bad += exact_gather_failures(dev, monkeypatch, ALL_PLANS, C, M, K)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("C", [5, 7])
def test_exact_wide_knn(dev, monkeypatch, C):
    """D > 4: knn_backward_kernel<0> with its runtime D, and the deterministic form."""
    bad = []
    for _, M, K, norm in [c for c in R.wide_cases("knn") if c[0] == C]:
        bad += exact_knn_failures(dev, monkeypatch, WIDE_PLANS, C, M, K, norm)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("C", [5, 64])
def test_exact_wide_gather(dev, monkeypatch, C):
    bad = []
    for _, M, K, norm in [c for c in R.wide_cases("gather") if c[0] == C]:
        bad += exact_gather_failures(dev, monkeypatch, WIDE_PLANS, C, M, K)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ float inputs, per-element bound
def float_knn_inputs(seed, n, rows, K, M, D):
    p1 = cases.cloud(seed, (n, rows, D))
    p2 = cases.cloud(seed + 1, (n, M, D))
    grad = cases.grad_for("scatter%d" % seed, (n, rows, K))
    idx = R.table(seed, n, rows, K, M, R.tile_rows(min(D, 4)))
    l1, l2 = R.ragged_lengths(n, rows, K, M)
    return p1, p2, l1, l2, idx, grad


def check_float_knn(dev, oracle, monkeypatch, plans, inputs, norm):
    p1, p2, l1, l2, idx, grad = inputs
    r = R.knn_backward_ref(p1, p2, l1, l2, idx, norm, grad)
    o1, _ = oracle.knn_points_backward(p1, p2, l1, l2, idx, norm, grad)
    bad = []
    for plan in plans:
        g1, g2, S = run_knn(dev, monkeypatch, plan, p1, p2, l1, l2, idx, norm, grad)
        ok, ratio, n_bad = R.within_bound(g2, r.g2, r.n2, r.A2, S)
        print(f"knn {plan} L{norm}: grad_p2 worst |err| / bound = {ratio:.4f}")
        if not np.array_equal(bits(g1), bits(o1)):
            bad.append(f"knn {plan} L{norm}: grad_p1 is not the fp32 k-ordered sum ({differing(g1, o1)} elements)")
        if not ok:
            bad.append(f"knn {plan} L{norm}: {n_bad} elements of grad_p2 outside the bound, worst ratio {ratio:g}")
        if g2[r.n2 == 0].any():
            bad.append(f"knn {plan} L{norm}: a row without addends is not zero")
    return bad


@pytest.mark.parametrize("D", [3, 5])
@pytest.mark.parametrize("Mname", ["65", "tile+1"])
def test_float_knn_within_bound(dev, oracle, monkeypatch, Mname, D):
    M = R.target_sizes(min(D, 4))[Mname]
    plans = ALL_PLANS if D <= 4 else WIDE_PLANS
    bad = []
    for norm in (2, 1):
        bad += check_float_knn(dev, oracle, monkeypatch, plans, float_knn_inputs(5100 + D, N, L, 8, M, D), norm)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("U", [3, 64])
@pytest.mark.parametrize("Mname", ["65", "tile+1"])
def test_float_gather_within_bound(dev, monkeypatch, Mname, U):
    M = R.target_sizes(min(U, 4))[Mname]
    plans = ALL_PLANS if U <= 4 else WIDE_PLANS
    go = cases.grad_for("scatterg%d" % U, (N, L, 8, U))
    idx = R.table(5200 + U, N, L, 8, M, R.tile_rows(min(U, 4)))
    bad = []
    for lengths in (R.ragged_lengths(N, L, 8, M)[1], None):
        r = R.gather_backward_ref(go, idx, lengths, M)
        for plan in plans:
            gx, S = run_gather(dev, monkeypatch, plan, go, idx, lengths, M)
            ok, ratio, n_bad = R.within_bound(gx, r.gx, r.n, r.A, S)
            print(f"gather {plan} lengths={lengths is not None}: worst |err| / bound = {ratio:.4f}")
            if not ok:
                bad.append(f"gather {plan} lengths={lengths is not None}: {n_bad} elements outside the bound, "
                           f"worst ratio {ratio:g}")
            if gx[r.n == 0].any():
                bad.append(f"gather {plan}: a row without addends is not zero")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("K,S", [(16, 16), (15, 1)], ids=["K16-tiles", "K15-atomics"])
def test_default_plan_at_its_threshold(dev, oracle, monkeypatch, K, S):
    """No knob.  N = 2, P1 = 65536, K = 16, P2 = 8193, D = 3 is the smallest shape that selects LDS tiles by itself:
    N P1 K = 2^21 entries, two tiles, and S = min(ceil(256 / 4), 65536 / 4096) = 16 row splits; the same table with
    K = 15 stays below the threshold and takes device atomics (S = 1 in the bound)."""
    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    from pytorch3d_pointops_amd import _C

    p1, p2, l1, l2, idx, grad = float_knn_inputs(5300, 2, 65536, K, 8193, 3)
    r = R.knn_backward_ref(p1, p2, l1, l2, idx, 2, grad)
    o1, _ = oracle.knn_points_backward(p1, p2, l1, l2, idx, 2, grad)
    g1, g2 = _C.knn_points_backward(G(p1, dev), G(p2, dev), G(l1, dev), G(l2, dev), G(idx, dev), 2, G(grad, dev))
    ok, ratio, n_bad = R.within_bound(g2.cpu().numpy(), r.g2, r.n2, r.A2, S)
    print(f"default plan K={K}: grad_p2 worst |err| / bound = {ratio:.4f}, largest n = {int(r.n2.max())}")
    assert np.array_equal(bits(g1.cpu().numpy()), bits(o1))
    assert ok, (n_bad, ratio)
    go = cases.grad_for("scatterdefault", (2, 65536, K, 3))
    gr = R.gather_backward_ref(go, idx, l2, 8193)
    gx = _C.gather_neighbors_backward(G(go, dev), G(idx, dev), G(l2, dev), 8193)
    ok, ratio, n_bad = R.within_bound(gx.cpu().numpy(), gr.gx, gr.n, gr.A, S)
    print(f"default plan K={K}: grad_x worst |err| / bound = {ratio:.4f}")
    assert ok, (n_bad, ratio)


# ------------------------------------------------------------------ deterministic claims
@pytest.mark.parametrize("U", [1, 2, 3, 4, 5, 64])
def test_deterministic_gather_is_the_sequential_sum(dev, monkeypatch, U):
    """grad_x of gather_neighbors_backward(deterministic=True) on float inputs is the fp32 sum in TABLE ORDER, bit for
    bit (np.add.at is sequential), with and without lengths, and two runs are identical."""
    M = 65
    go = cases.grad_for("scatterdet%d" % U, (N, L, 8, U))
    idx = R.table(5400 + U, N, L, 8, M, R.tile_rows(min(U, 4)))
    for lengths in (R.ragged_lengths(N, L, 8, M)[1], None):
        a, _ = run_gather(dev, monkeypatch, "deterministic", go, idx, lengths, M)
        b, _ = run_gather(dev, monkeypatch, "deterministic", go, idx, lengths, M)
        assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(bits(a), bits(R.gather_backward_sequential_f32(go, idx, lengths, M)))


@pytest.mark.parametrize("n,M", [(3, 85), (4, 64), (1, 257), (4, 16384)], ids=["NM=255", "NM=256", "NM=257", "NM=2^16"])
def test_deterministic_key_width(dev, oracle, monkeypatch, n, M):
    """N M at and around a power of two, where det_key_bits changes and the masked key N M needs the extra bit: row 0
    of cloud 0 (the key the masked key aliases without that bit) takes every other query row's first entry, masked
    entries (-1 padding, k >= l2, rows >= l1) in between.  grad_p2 against the oracle's sequential loop and grad_x
    against the sequential fp32 sum, bit for bit."""
    K, D = 8, 3
    p1, p2, l1, l2, idx, grad = float_knn_inputs(5500 + n, n, L, K, M, D)
    idx[0, ::2, 0] = 0
    assert (idx < 0).any() and l2[0] < K
    o1, o2 = oracle.knn_points_backward(p1, p2, l1, l2, idx, 2, grad)
    g1, g2, _ = run_knn(dev, monkeypatch, "deterministic", p1, p2, l1, l2, idx, 2, grad)
    assert np.array_equal(bits(g1), bits(o1)) and np.array_equal(bits(g2), bits(o2))
    go = cases.grad_for("scatterkeys", (n, L, K, D))
    for lengths in (l2, None):
        gx, _ = run_gather(dev, monkeypatch, "deterministic", go, idx, lengths, M)
        assert np.array_equal(bits(gx), bits(R.gather_backward_sequential_f32(go, idx, lengths, M)))


# ------------------------------------------------------------------ through autograd
class _deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(self.on)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.prev)


def _lattice_clouds(seed, P1=700, P2=65, D=3):
    rng = np.random.default_rng(seed)
    p1 = (rng.integers(0, 5, (3, P1, D)) * 0.25).astype(np.float32)
    p2 = (rng.integers(0, 5, (3, P2, D)) * 0.25).astype(np.float32)
    return p1, p2, np.array([P1 - 37, 0, P1]), np.array([5, P2, P2 - 1]), rng


def _upstream(kind, shape, rng, dev):
    """An exact upstream gradient in the given memory layout, and its values."""
    if kind == "contiguous":
        g = rng.integers(-4, 5, shape).astype(np.float32)
        return G(g, dev), g
    if kind == "expanded":  # what .sum().backward() passes: every stride 0
        return torch.ones((), device=dev).expand(shape), np.ones(shape, np.float32)
    wide = rng.integers(-4, 5, shape[:-1] + (shape[-1] + 3,)).astype(np.float32)
    t = G(wide, dev)[..., 2:2 + shape[-1]]
    assert not t.is_contiguous() or shape[-1] == 0
    return t, wide[..., 2:2 + shape[-1]]


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("layout", ["contiguous", "expanded", "slice"])
def test_eager_nodes_on_exact_inputs(dev, monkeypatch, det, layout):
    """knn_points, ball_query, knn_gather and masked_gather through their autograd nodes on exact inputs, by default and
    under torch.use_deterministic_algorithms(True), with the upstream gradient contiguous, expanded with stride 0 (from
    .sum().backward()) and as a non-contiguous slice of a wider tensor: bit equality with the cast float64 reference."""
    from pytorch3d_pointops_amd.functions import ball_query, knn_gather, knn_points
    from pytorch3d_pointops_amd.functions.utils import masked_gather

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    p1, p2, l1, l2, rng = _lattice_clouds(5600)
    K = 8

    def leaves():
        return G(p1, dev).requires_grad_(True), G(p2, dev).requires_grad_(True)

    with _deterministic(det):
        for norm in (2, 1):
            a, b = leaves()
            r = knn_points(a, b, G(l1, dev), G(l2, dev), norm=norm, K=K)
            up, upv = _upstream(layout, tuple(r.dists.shape), rng, dev)
            if layout == "expanded":
                r.dists.sum().backward()
            else:
                r.dists.backward(up)
            ref = R.knn_backward_ref(p1, p2, l1, l2, r.idx.cpu().numpy(), norm, upv)
            assert max(ref.A1.max(), ref.A2.max()) < R.EXACT_LIMIT
            assert np.array_equal(bits(a.grad.cpu().numpy()), bits(ref.g1.astype(np.float32))), ("knn_points", norm)
            assert np.array_equal(bits(b.grad.cpu().numpy()), bits(ref.g2.astype(np.float32))), ("knn_points", norm)

        a, b = leaves()
        q = ball_query(a, b, G(l1, dev), G(l2, dev), K=K, radius=0.3, return_nn=False)
        bidx = q.idx.cpu().numpy()
        assert (bidx < 0).any() and (bidx >= 0).any()
        up, upv = _upstream(layout, tuple(q.dists.shape), rng, dev)
        if layout == "expanded":
            q.dists.sum().backward()
        else:
            q.dists.backward(up)
        ref = R.knn_backward_ref(p1, p2, l1, l2, bidx, 2, upv)
        assert np.array_equal(bits(a.grad.cpu().numpy()), bits(ref.g1.astype(np.float32))), "ball_query"
        assert np.array_equal(bits(b.grad.cpu().numpy()), bits(ref.g2.astype(np.float32))), "ball_query"

        M, U = 65, 3
        table = R.table(5601, 3, 700, K, M, R.tile_rows(U))
        lengths = np.array([5, M, M])
        for name, fn, tab, lens in (("knn_gather", lambda x: knn_gather(x, G(np.maximum(table, 0), dev), G(lengths, dev)),
                                     np.maximum(table, 0), lengths),
                                    ("masked_gather", lambda x: masked_gather(x, G(table, dev)), table, None)):
            x = G(p2, dev).requires_grad_(True)
            out = fn(x)
            up, upv = _upstream(layout, tuple(out.shape), rng, dev)
            if layout == "expanded":
                out.sum().backward()
            else:
                out.backward(up)
            ref = R.gather_backward_ref(upv, tab, lens, M)
            assert ref.A.max() < R.EXACT_LIMIT
            assert np.array_equal(bits(x.grad.cpu().numpy()), bits(ref.gx.astype(np.float32))), name
