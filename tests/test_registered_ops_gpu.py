"""The registered operators (pytorch3d_pointops_amd/ops.py) and every route functions/*.py takes while torch.compile
traces it, on the device: opcheck on every sample of tests/registered_ops_cases.py, fake output == real output, the
registered autograd formulas against plain references (the CPU oracle, float64 torch compositions on the CPU over the
same neighbour table, the float64 checker of test_points_normals_gpu.py), compiled == eager for every
`torch.compiler.is_compiling()` branch with the traced graphs inspected for the operators they must hold, and the host
caches across tracing.  Bars: bit equality where no atomics are involved (and everywhere under
torch.use_deterministic_algorithms(True)), the suite's 1e-5 `close` otherwise."""
import contextlib

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.fx.experimental.symbolic_shapes import ShapeEnv

import cases
import registered_ops_cases as roc
from conftest import bits
from pytorch3d_pointops_amd import synth

pytestmark = pytest.mark.gpu

OPCHECK_UTILS = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic")


def close(a, b, tol=1e-5):  # the suite's rule (test_gpu_parity.close)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    return a.shape == b.shape and (a.size == 0 or float(np.abs(a - b).max()) <= tol * scale)


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def npy(t):
    return t.detach().cpu().numpy()


def _ops():
    from pytorch3d_pointops_amd import ops

    return ops


def _op(name):
    _ops()
    return getattr(torch.ops.pointops_amd, name)


def _samples(name, dev):
    return roc.TABLE[name].samples(lambda a: G(a, dev))


def _with_grad(name, sample, args):
    """The sample with its differentiable arguments as leaves.  `points_alignment` with idx has no backward, and a
    K = 1 neighbourhood has a zero covariance: three coincident eigenvalues, whose gradient is inf / nan by contract."""
    want = roc.TABLE[name].differentiable
    if (name == "points_alignment" and args[2] is not None) or (name == "local_frames" and sample.startswith("k1")):
        want = ()
    return tuple(a.clone().requires_grad_(True) if i in want and a is not None else a for i, a in enumerate(args))


@contextlib.contextmanager
def deterministic(on=True):
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


def _flat(out):
    return [] if out is None else list(out) if isinstance(out, (tuple, list)) else [out]


def test_table_covers_the_registered_ops():
    assert set(roc.TABLE) == set(_ops().registered_ops())


# ------------------------------------------------------------------------------------------------ a. opcheck
@pytest.mark.parametrize("name", sorted(roc.TABLE))
def test_opcheck(dev, name):
    op = _op(name)
    entry = roc.TABLE[name]
    assert set(entry.opcheck_skip) | set(entry.opcheck_forward_only) <= set(OPCHECK_UTILS)
    plain = tuple(u for u in OPCHECK_UTILS if u in entry.opcheck_forward_only)
    utils = tuple(u for u in OPCHECK_UTILS if u not in entry.opcheck_skip and u not in plain)
    for sample, args in _samples(name, dev).items():
        torch.library.opcheck(op, _with_grad(name, sample, args), test_utils=utils, atol=1e-5, rtol=1e-5)
        if plain:
            torch.library.opcheck(op, args, test_utils=plain, atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ b. fake == real
@pytest.mark.parametrize("name", sorted(roc.TABLE))
def test_fake_equals_real(dev, name):
    op = _op(name)
    for sample, args in _samples(name, dev).items():
        mode = FakeTensorMode(shape_env=ShapeEnv())
        convert = lambda a: mode.from_tensor(a) if torch.is_tensor(a) else [mode.from_tensor(t) for t in a] \
            if isinstance(a, list) else a  # noqa: E731
        fake_args = tuple(convert(a) for a in args)
        with mode:
            fake = _flat(op(*fake_args))
        real_args = tuple(a.clone() if torch.is_tensor(a) else a for a in args)
        real = _flat(op(*real_args))
        want = roc.TABLE[name].outputs(*args)
        assert len(fake) == len(real) == (0 if want is None else len(want)), (name, sample)
        for f, r, (shape, dtype) in zip(fake, real, want or []):
            assert r.dtype == f.dtype == dtype and r.device == f.device == args[0].device, (name, sample)
            assert len(r.shape) == len(f.shape), (name, sample)
            for have, size, doc in zip(r.shape, f.shape, shape):
                if doc == roc.UNBACKED:  # FPS: the unbacked dimension is max(K)
                    assert isinstance(size, torch.SymInt) and have == int(args[2].max()), (name, sample)
                else:
                    assert have == size == doc, (name, sample, tuple(r.shape), tuple(f.shape))
            if roc.UNBACKED not in shape and r.numel():  # (a tensor without elements has no layout to compare)
                assert r.stride() == f.stride(), (name, sample)
            assert r.is_contiguous(), (name, sample)


def test_fps_unbacked_dimension_is_max_k(dev, oracle):
    """What opcheck's AOT dispatch utility cannot express for FPS: the real output's second dimension is max(K), and a
    caller-known maximum gives the same rows (checked against the oracle)."""
    args = _samples("sample_farthest_points", dev)["ragged_unknown_max"]
    out = _op("sample_farthest_points")(*args)
    assert tuple(out.shape) == (roc.N, int(args[2].max()))
    known = _op("sample_farthest_points")(*args[:4], int(args[2].max()))
    want = oracle.sample_farthest_points(*(npy(a) for a in args[:4]))
    assert np.array_equal(npy(out), want) and torch.equal(out, known)


# ------------------------------------------------------------------------------------------------ c. autograd
def _search_grads(dev, op_name, args, norm, oracle, eager):
    """Gradients of a random-weighted sum of the raw op's distances: (grad_p1, grad_p2), the neighbour table, the
    weights, and the same through the eager autograd.Function `eager`."""
    p1, p2 = (a.clone().requires_grad_(True) for a in args[:2])
    idx, dists = _op(op_name)(p1, p2, *args[2:])
    w = G(cases.grad_for(op_name, tuple(dists.shape)), dev)
    g1, g2 = torch.autograd.grad((dists * w).sum(), (p1, p2))
    q1, q2 = (a.clone().requires_grad_(True) for a in args[:2])
    e = eager(q1, q2)
    assert torch.equal(e.idx, idx) and torch.equal(e.dists, dists)
    e1, e2 = torch.autograd.grad((e.dists * w).sum(), (q1, q2))
    o1, o2 = oracle.knn_points_backward(*(npy(a) for a in args[:4]), npy(idx), norm, npy(w))
    return (g1, g2), (e1, e2), (o1, o2)


@pytest.mark.parametrize("op_name,sample,norm", [("knn_points_idx", "ragged_l2", 2), ("knn_points_idx", "ragged_l1", 1),
                                                 ("knn_points_idx", "full_l1", 1), ("ball_query", "ragged", 2),
                                                 ("ball_query", "empty_balls", 2)])
def test_search_autograd_against_the_oracle(dev, oracle, op_name, sample, norm):
    from pytorch3d_pointops_amd.functions import ball_query, knn_points

    args = _samples(op_name, dev)[sample]
    if op_name == "knn_points_idx":
        eager = lambda a, b: knn_points(a, b, args[2], args[3], norm=norm, K=args[5])  # noqa: E731
    else:
        eager = lambda a, b: ball_query(a, b, args[2], args[3], K=args[4], radius=args[5], return_nn=False)  # noqa: E731
    if op_name == "ball_query" and sample == "ragged":
        assert bool((_op(op_name)(*args)[0] == -1).any())  # the table carries -1 padding
    (g1, g2), (e1, e2), (o1, o2) = _search_grads(dev, op_name, args, norm, oracle, eager)
    assert np.array_equal(bits(npy(g1)), bits(o1)) and torch.equal(g1, e1)
    assert close(npy(g2), o2) and close(npy(g2), npy(e2))
    empty = npy(args[2]) == 0
    assert not npy(g1)[empty].any() and not npy(g2)[npy(args[3]) == 0].any()  # a cloud of length 0: zero rows
    with deterministic():
        (g1, g2), (e1, e2), (o1, o2) = _search_grads(dev, op_name, args, norm, oracle, eager)
    assert torch.equal(g1, e1) and torch.equal(g2, e2)
    assert np.array_equal(bits(npy(g1)), bits(o1)) and np.array_equal(bits(npy(g2)), bits(o2))


def _gather_reference(x, idx, lengths, w):
    """float64 torch on the CPU: out[n,l,k] = x[n, idx[n,l,k]], zero where k >= lengths[n] or idx < 0."""
    x = x.detach().double().cpu().requires_grad_(True)
    idx = idx.cpu()
    keep = idx >= 0
    if lengths is not None:
        keep = keep & (torch.arange(idx.shape[2])[None, None, :] < lengths.cpu()[:, None, None])
    out = torch.stack([x[n][idx[n].clamp(min=0)] for n in range(x.shape[0])])
    out = torch.where(keep[..., None], out, torch.zeros((), dtype=torch.float64))
    (g,) = torch.autograd.grad((out * w.double().cpu()).sum(), x)
    return out.detach(), g


@pytest.mark.parametrize("sample", ["u1_lengths", "u3_lengths", "u5_lengths", "u1_none", "u3_none", "u5_none", "k1"])
def test_gather_autograd_against_float64(dev, sample):
    from pytorch3d_pointops_amd.functions.knn import _gather_neighbors

    x, idx, lengths = _samples("gather_neighbors", dev)[sample]
    w = G(roc._signed(8101, tuple(idx.shape) + (x.shape[2],)), dev)

    def run(fn):
        leaf = x.clone().requires_grad_(True)
        out = fn(leaf, idx, lengths)
        return out, torch.autograd.grad((out * w).sum(), leaf)[0]

    out, g = run(_op("gather_neighbors"))
    ref_out, ref_g = _gather_reference(x, idx, lengths, w)
    assert np.array_equal(bits(npy(out)), bits(ref_out.float().numpy()))  # copies
    assert close(npy(g), ref_g.numpy())
    if lengths is not None:
        assert not npy(g)[npy(lengths) == 0].any()
    with deterministic():
        (_, g), (_, e) = run(_op("gather_neighbors")), run(_gather_neighbors.apply)
    assert torch.equal(g, e) and close(npy(g), ref_g.numpy())


@pytest.mark.parametrize("name,sample", [(n, s) for n in ("packed_to_padded", "padded_to_packed")
                                         for s in ("u1", "u3", "u5", "short_pad" if n == "packed_to_padded" else
                                                   "unowned_rows")])
def test_ragged_copy_autograd_against_float64(dev, name, sample):
    data, first, size = _samples(name, dev)[sample]
    leaf = data.clone().requires_grad_(True)
    out = _op(name)(leaf, first, size)
    w = G(roc._signed(8201, tuple(out.shape)), dev)
    (g,) = torch.autograd.grad((out * w).sum(), leaf)
    # float64 torch on the CPU: cloud b owns packed rows [first[b], first[b+1]) (the last one up to F)
    x = data.detach().double().cpu().requires_grad_(True)
    f = first.cpu().tolist()
    rows = x.shape[0] if name == "packed_to_padded" else size
    ends = f[1:] + [rows]
    if name == "packed_to_padded":
        ref = torch.zeros((len(f), size, x.shape[1]), dtype=torch.float64)
        parts = [(b, x[s:s + min(max(e - s, 0), size)]) for b, (s, e) in enumerate(zip(f, ends))]
        ref = torch.stack([torch.cat([p, p.new_zeros(size - p.shape[0], x.shape[1])]) for _, p in parts])
    else:
        ref = torch.zeros((size, x.shape[2]), dtype=torch.float64)
        for b, (s, e) in enumerate(zip(f, ends)):
            n = min(max(e - s, 0), x.shape[1])
            ref = ref.index_add(0, torch.arange(s, s + n), x[b, :n])
    (ref_g,) = torch.autograd.grad((ref * w.double().cpu()).sum(), x)
    assert np.array_equal(bits(npy(out)), bits(ref.detach().float().numpy()))  # copies: bit-equal
    assert np.array_equal(bits(npy(g)), bits(ref_g.float().numpy()))


@pytest.mark.parametrize("sample", ["d3_k5", "d1_k8", "d5_k1"])
def test_covariance_autograd_against_float64(dev, sample):
    from pytorch3d_pointops_amd.functions.utils import _point_covariances

    (knn,) = _samples("point_covariances", dev)[sample]
    w = G(roc._signed(8301, tuple(knn.shape[:2]) + (knn.shape[3],) * 2), dev)

    def run(fn):
        leaf = knn.clone().requires_grad_(True)
        out = fn(leaf)
        return out, torch.autograd.grad((out * w).sum(), leaf)[0]

    out, g = run(_op("point_covariances"))
    x = knn.double().cpu().requires_grad_(True)
    d = x - x.mean(2, keepdim=True)
    ref = (d[..., :, None] * d[..., None, :]).mean(2)
    (ref_g,) = torch.autograd.grad((ref * w.double().cpu()).sum(), x)
    assert close(npy(out), ref.detach().numpy()) and close(npy(g), ref_g.numpy())
    e_out, e = run(_point_covariances.apply)
    assert torch.equal(out, e_out) and torch.equal(g, e)  # no atomics: bit-equal to the eager Function


@pytest.mark.parametrize("sample", ["mean_weights", "sum_none", "mean_full"])
def test_chamfer_reduce_autograd_against_float64(dev, sample):
    from pytorch3d_pointops_amd.functions.chamfer import _masked_point_reduce

    dists, lengths, weights, mean = _samples("chamfer_reduce", dev)[sample]
    w = G(roc._signed(8401, (dists.shape[0],)), dev)

    def run(fn):
        leaf = dists.clone().requires_grad_(True)
        out = fn(leaf, lengths, weights, mean)
        return out, torch.autograd.grad((out * w).sum(), leaf)[0]

    out, g = run(_op("chamfer_reduce"))
    x = dists.double().cpu().requires_grad_(True)
    lens = lengths.cpu()
    ref = (x * (torch.arange(x.shape[1])[None] < lens[:, None])).sum(1)
    if weights is not None:
        ref = ref * weights.double().cpu()
    if mean:
        ref = ref / lens.clamp(min=1)
    (ref_g,) = torch.autograd.grad((ref * w.double().cpu()).sum(), x)
    assert close(npy(out), ref.detach().numpy()) and close(npy(g), ref_g.numpy())
    assert not npy(g)[npy(lengths) == 0].any()
    e_out, e = run(_masked_point_reduce.apply)
    assert torch.equal(out, e_out) and torch.equal(g, e)


@pytest.mark.parametrize("disambiguate", [True, False])
def test_local_frames_autograd_against_float64(dev, disambiguate):
    """The float64 checker (and bar) of test_points_normals_gpu.test_gradients_against_float64, on the raw op."""
    import test_points_normals_gpu as normals
    from pytorch3d_pointops_amd.functions.points_normals import _local_frames, centre_clouds

    pts, lens, k = roc.frames_clouds()["ragged"]
    lengths = G(lens, dev)
    leaves = [G(pts[n, :lens[n]], dev).requires_grad_(True) for n in range(len(lens))]

    def run(fn, det=False):
        padded = torch.nn.utils.rnn.pad_sequence(leaves, batch_first=True)
        c = centre_clouds(padded, lengths)
        idx = G(roc.knn_table(npy(c), npy(c), lens, lens, k), dev)
        with deterministic(det):
            curv, frames = fn(c, lengths, idx, disambiguate)
        return c, idx, curv, frames

    c, idx, curv, frames = run(_op("local_frames"))
    g = torch.Generator().manual_seed(17)
    g_curv = torch.randn(curv.shape, generator=g, dtype=torch.float64)
    g_frames = torch.randn(frames.shape, generator=g, dtype=torch.float64)
    gap, lmax = normals._gaps(curv.detach().double().cpu())
    ill = (gap.amin(-1) < 1e-2 * lmax[..., 0]) | ~normals._valid(lengths, pts.shape[1])
    g_curv[ill] = 0
    g_frames[ill] = 0
    ref, _ = normals._reference_grads(leaves, lengths, idx, k, disambiguate, frames.detach(), g_curv, g_frames)

    def grads(curv, frames, det=False):
        with deterministic(det):
            return torch.autograd.grad((curv * g_curv.float().to(dev)).sum() + (frames * g_frames.float().to(dev)).sum(),
                                       leaves, allow_unused=True)

    got = grads(curv, frames)
    for u, v in zip(got[:2], ref[:2]):
        scale = float(v.abs().max())
        assert bool(torch.isfinite(u).all()) and scale > 0
        assert float((u.double().cpu() - v).abs().max()) <= 1e-3 * scale
    assert got[2] is None or got[2].numel() == 0  # the cloud of length 0 has no rows
    assert not npy(curv)[2].any() and not npy(frames)[2].any()
    # deterministic mode: bit-equal to the eager Function
    _, _, curv_d, frames_d = run(_op("local_frames"), det=True)
    _, _, curv_e, frames_e = run(_local_frames.apply, det=True)
    assert torch.equal(curv_d, curv_e) and torch.equal(frames_d, frames_e) and torch.equal(curv_d, curv)
    for u, v in zip(grads(curv_d, frames_d, det=True)[:2], grads(curv_e, frames_e, det=True)[:2]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("sample", ["d3_plain", "d3_lengths_weights_scale", "d2_plain", "d2_lengths_weights_scale"])
def test_alignment_autograd_equals_the_eager_function(dev, sample):
    """No atomics anywhere: the registered formula is bit-equal to the eager `_alignment` Function (which
    test_points_alignment_gpu.py pins against float64)."""
    from pytorch3d_pointops_amd.functions.points_alignment import _alignment

    x, y, _, lengths, weights, scale, reflect, eps = _samples("points_alignment", dev)[sample]
    w = [G(roc._signed(8501 + i, s), dev) for i, s in enumerate([(roc.N, x.shape[2], x.shape[2]), (roc.N, x.shape[2]),
                                                                 (roc.N,)])]

    def run(fn):
        leaves = [t.clone().requires_grad_(True) for t in (x, y, weights) if t is not None]
        wl = leaves[2] if weights is not None else None
        out = fn(leaves[0], leaves[1], wl)
        return out[:4], torch.autograd.grad(sum((o * v).sum() for o, v in zip(out[:3], w)), leaves)

    out, g = run(lambda a, b, c: _op("points_alignment")(a, b, None, lengths, c, scale, reflect, eps))
    e_out, e = run(lambda a, b, c: _alignment.apply(a, b, lengths, c, scale, reflect, eps))
    assert all(torch.equal(u, v) for u, v in zip(out, e_out)) and all(torch.equal(u, v) for u, v in zip(g, e))
    assert all(bool(torch.isfinite(u).all()) for u in g)
    if lengths is not None:
        assert not npy(g[0])[npy(lengths) == 0].any() and not npy(g[2])[npy(lengths) == 0].any()


# ------------------------------------------------------------------------------------------------ d. compiled == eager
class Recorder:
    """aot_eager (eager numerics) behind a wrapper that records every call_function target of the traced graphs."""

    def __init__(self):
        self.graphs = []

    def __call__(self, gm, example_inputs):
        from torch._dynamo.backends.debugging import aot_eager

        self.graphs.append([str(n.target) for n in gm.graph.nodes if n.op == "call_function"])
        return aot_eager(gm, example_inputs)

    def ops(self):
        return {t.split("pointops_amd.")[1].split(".")[0] for g in self.graphs for t in g if "pointops_amd." in t}


def _clouds(dev, d=3):
    a, b = roc._pair(8601, d=d)
    return G(a, dev), G(b, dev), G(roc.L1_RAGGED, dev), G(np.array([roc.P2, 3, 17]), dev)


def _fn_rows():
    """name -> (builder(dev) -> (fn, differentiable inputs, other inputs), ops that must be in a traced graph,
    atomics in eager's backward, fullgraph)"""
    from pytorch3d_pointops_amd.functions import (ball_query, get_point_covariances, knn_gather, knn_points,
                                                  masked_gather, packed_to_padded, padded_to_packed,
                                                  sample_farthest_points)
    from pytorch3d_pointops_amd.functions.points_alignment import corresponding_points_alignment
    from pytorch3d_pointops_amd.functions.points_normals import estimate_pointcloud_local_coord_frames
    from pytorch3d_pointops_amd.functions.sample_pdf import sample_pdf

    rows = {}

    def row(name, build, need, atomics=True, fullgraph=True):
        rows[name] = (build, set(need), atomics, fullgraph)

    def knn(**kw):
        def build(dev):
            a, b, l1, l2 = _clouds(dev)
            if kw.get("no_lengths"):
                l1 = l2 = None
            k = dict(norm=kw.get("norm", 2), K=kw.get("K", roc.K), return_nn=kw.get("return_nn", False))
            if kw.get("self_query"):
                return (lambda p: tuple(t for t in knn_points(p, p, l1, l1, **k) if t is not None)), [a], []
            return (lambda p, q: tuple(t for t in knn_points(p, q, l1, l2, **k) if t is not None)), [a, b], []
        return build

    row("knn_points[l2]", knn(), ["knn_points_idx"])
    row("knn_points[l1]", knn(norm=1), ["knn_points_idx"])
    row("knn_points[return_nn]", knn(return_nn=True), ["knn_points_idx", "gather_neighbors"])
    row("knn_points[lengths=None]", knn(no_lengths=True), ["knn_points_idx"])
    row("knn_points[p1 is p2]", knn(self_query=True, no_lengths=True, return_nn=True), ["knn_points_idx", "gather_neighbors"])
    row("knn_points[K above a target's length]", knn(K=20), ["knn_points_idx"])

    def gather(with_lengths):
        def build(dev):
            a, b, l1, l2 = _clouds(dev)
            idx = G(roc.knn_table(npy(a), npy(b), roc.L1_RAGGED, npy(l2), roc.K), dev)
            feats = G(roc._signed(8611, (roc.N, roc.P2, 5)), dev)
            return (lambda f: knn_gather(f, idx, l2 if with_lengths else None)), [feats], []
        return build

    row("knn_gather[lengths]", gather(True), ["gather_neighbors"])
    row("knn_gather[no lengths]", gather(False), ["gather_neighbors"])

    def masked(three_d):
        def build(dev):
            a, b, l1, l2 = _clouds(dev)
            idx = roc.ball_table(npy(a), npy(b), roc.L1_RAGGED, npy(l2), roc.K, 0.3)
            assert (idx == -1).any()
            idx = G(idx if three_d else idx[:, :, 0], dev)
            return (lambda p: masked_gather(p, idx)), [b], []
        return build

    row("masked_gather[3-D idx]", masked(True), ["gather_neighbors"])
    row("masked_gather[2-D idx]", masked(False), ["gather_neighbors"])

    def ball(return_nn):
        def build(dev):
            a, b, l1, l2 = _clouds(dev)
            return (lambda p, q: tuple(t for t in ball_query(p, q, l1, l2, K=roc.K, radius=0.3, return_nn=return_nn)
                                       if t is not None)), [a, b], []
        return build

    row("ball_query[padded rows]", ball(False), ["ball_query"])
    row("ball_query[return_nn]", ball(True), ["ball_query", "gather_neighbors"])

    def fps(k, with_lengths=False, random_start=False):
        def build(dev):
            a, _, l1, _ = _clouds(dev)
            kk = G(np.array(k), dev) if isinstance(k, np.ndarray) else k
            lengths = G(np.array([roc.P1, 33, 9]), dev) if with_lengths else None

            return (lambda p: sample_farthest_points(p, lengths, kk, random_start_point=random_start)), [a], []
        return build

    row("sample_farthest_points[int K]", fps(7), ["sample_farthest_points", "gather_neighbors"])
    row("sample_farthest_points[list K]", fps([7, 2, 40]), ["sample_farthest_points", "gather_neighbors"])
    # fullgraph=False: max(K) of a tensor K is read back on the host, as the reference does
    # (sample_farthest_points.cu:132); the graph breaks at that read and the op is traced after it
    row("sample_farthest_points[tensor K]", fps(np.array([7, 2, 40])), ["sample_farthest_points", "gather_neighbors"],
        fullgraph=False)
    row("sample_farthest_points[lengths]", fps(7, with_lengths=True), ["sample_farthest_points", "gather_neighbors"])
    # fullgraph=False: one torch.randint(...).item() per cloud, the reference's RNG consumption
    # (functions/sample_farthest_points.py:86-89)
    row("sample_farthest_points[random start]", fps(7, with_lengths=True, random_start=True),
        ["sample_farthest_points", "gather_neighbors"], fullgraph=False)

    def ragged(kind):
        def build(dev):
            lens = np.array([5, 0, 70, 3])
            first = G(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), dev)
            rows_ = int(lens.sum())
            if kind == "pack1":
                return (lambda x: packed_to_padded(x, first, 70)), [G(roc._signed(8621, (rows_,)), dev)], []
            if kind == "pack_trailing":
                return (lambda x: packed_to_padded(x, first, 70)), [G(roc._signed(8622, (rows_, 2, 3)), dev)], []
            if kind == "unpack1":
                return (lambda x: padded_to_packed(x, first, rows_)), [G(roc._signed(8623, (4, 70)), dev)], []
            if kind == "unpack_trailing":
                return (lambda x: padded_to_packed(x, first, rows_)), [G(roc._signed(8624, (4, 70, 2, 3)), dev)], []
            return (lambda x: padded_to_packed(x, first, rows_, max_size_dim=2)), [G(roc._signed(8625, (4, 3, 70)), dev)], []
        return build

    row("packed_to_padded[1-D]", ragged("pack1"), ["packed_to_padded"], atomics=False)
    row("packed_to_padded[trailing dims]", ragged("pack_trailing"), ["packed_to_padded"], atomics=False)
    row("padded_to_packed[1-D]", ragged("unpack1"), ["padded_to_packed"], atomics=False)
    row("padded_to_packed[trailing dims]", ragged("unpack_trailing"), ["padded_to_packed"], atomics=False)
    row("padded_to_packed[max_size_dim=2]", ragged("unpack_dim2"), ["padded_to_packed"], atomics=False)

    def cov(dev):
        a, _, l1, _ = _clouds(dev)
        lens = G(np.array([roc.P1, 33, 9]), dev)
        return (lambda p: get_point_covariances(p, lens, roc.K)), [a], []

    row("get_point_covariances", cov, ["knn_points_idx", "gather_neighbors", "point_covariances"])

    def frames(dev):
        pts = G(roc._signed(8631, (2, roc.FRAMES_P, 3)), dev)
        return (lambda p: estimate_pointcloud_local_coord_frames(p, roc.FRAMES_K)), [pts], []

    row("estimate_pointcloud_local_coord_frames", frames, ["knn_points_idx", "local_frames"])

    def align(d, scale):
        def build(dev):
            x, y = G(roc._signed(8640 + d, (roc.N, roc.P1, d)), dev), G(roc._signed(8650 + d, (roc.N, roc.P1, d)), dev)
            w = G(synth.uniform_f32(8660 + d, (roc.N, roc.P1)), dev) if scale else None
            return (lambda p, q: tuple(corresponding_points_alignment(p, q, w, estimate_scale=scale))), [x, y], []
        return build

    row("corresponding_points_alignment[D=3]", align(3, False), ["points_alignment"], atomics=False)
    row("corresponding_points_alignment[D=2]", align(2, False), ["points_alignment"], atomics=False)
    row("corresponding_points_alignment[scale]", align(3, True), ["points_alignment"], atomics=False)

    def pdf(dev):
        bins, w, _, _ = roc.TABLE["sample_pdf"].samples(lambda a: G(a, dev))["b4_7x33"]
        return (lambda: sample_pdf(bins, w, 33, det=True)), [], []

    row("sample_pdf[det]", pdf, ["sample_pdf"], atomics=False)
    return rows


def _chamfer_rows():
    """One variant per point_reduction x features x single_directional (weights alternating) + the three extra variants
    of cases.chamfer_variants()."""
    out, use_w = [], False
    for pr in ("mean", "sum", "max", None):
        for feats in (False, True):
            if pr == "max" and feats:
                continue
            for single in (False, True):
                out.append(dict(point_reduction=pr, batch_reduction=None if pr is None else "mean",
                                single_directional=single, use_weights=use_w, features=feats, abs_cosine=True, norm=2))
                use_w = not use_w
    return out + cases.chamfer_variants()[-3:]


def _chamfer_call(dev, v):
    from pytorch3d_pointops_amd.functions.chamfer import chamfer_distance

    c = cases.chamfer_inputs(8701, N=3, P1=roc.P1, P2=roc.P2)
    xl, yl, w = G(np.array([roc.P1, 50, 9]), dev), G(np.array([60, roc.P2, 7]), dev), G(c["w"], dev)
    leaves = [G(c[k], dev) for k in (("x", "y", "xn", "yn") if v["features"] else ("x", "y"))]

    def fn(*t):
        kw = dict(x_features={"n": t[2]}, y_features={"n": t[3]}, feature_names=["n"]) if v["features"] else {}
        loss, lf = chamfer_distance(t[0], t[1], x_lengths=xl, y_lengths=yl, weights=w if v["use_weights"] else None,
                                    batch_reduction=v["batch_reduction"], point_reduction=v["point_reduction"],
                                    norm=v["norm"], single_directional=v["single_directional"],
                                    abs_cosine=v["abs_cosine"], **kw)
        flat = list(loss) if isinstance(loss, tuple) else [loss]
        for item in ([] if lf is None else [lf["n"]]):
            flat += list(item) if isinstance(item, tuple) else [item]
        return tuple(t for t in flat if t is not None)

    need = {"knn_points_idx"} | ({"gather_neighbors"} if v["features"] else set()) \
        | ({"chamfer_reduce"} if v["point_reduction"] in ("mean", "sum") else set())
    return fn, leaves, need


def _run(fn, leaves, seed=8801):
    t = [x.clone().requires_grad_(True) for x in leaves]
    torch.manual_seed(11)  # (random_start_point draws from the global generator: the same draws for every run)
    out = fn(*t)
    out = out if isinstance(out, tuple) else (out,)
    floats = [o for o in out if o.is_floating_point() and o.requires_grad]
    grads = []
    if floats:
        loss = sum((o * G(roc._signed(seed + i, tuple(o.shape)), o.device)).sum() for i, o in enumerate(floats))
        grads = torch.autograd.grad(loss, t, allow_unused=True)
    return out, grads


def _assert_compiled_equals_eager(fn, leaves, need, atomics, fullgraph, forward_bitwise=True):
    torch._dynamo.reset()
    rec = Recorder()
    compiled = torch.compile(fn, backend=rec, fullgraph=fullgraph)
    e_out, e_g = _run(fn, leaves)
    c_out, c_g = _run(compiled, leaves)
    assert need <= rec.ops(), (need, rec.graphs)  # not a silent eager run: the ops are in the traced graphs
    assert len(e_out) == len(c_out) and len(e_g) == len(c_g)
    for u, v in zip(e_out, c_out):
        assert torch.equal(u, v) if forward_bitwise else close(npy(v), npy(u))
    for u, v in zip(e_g, c_g):
        assert (u is None) == (v is None)
        if u is not None:
            assert close(npy(v), npy(u)) if atomics else torch.equal(u, v)
    with deterministic():
        e_out, e_g = _run(fn, leaves)
        c_out, c_g = _run(compiled, leaves)
    for u, v in zip(list(e_out) + [g for g in e_g if g is not None], list(c_out) + [g for g in c_g if g is not None]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("name", sorted(_fn_rows()))
def test_compiled_equals_eager(dev, name):
    build, need, atomics, fullgraph = _fn_rows()[name]
    fn, leaves, _ = build(dev)
    _assert_compiled_equals_eager(fn, leaves, need, atomics, fullgraph)


@pytest.mark.parametrize("v", _chamfer_rows(), ids=cases.variant_key)
def test_compiled_chamfer_equals_eager(dev, v):
    """A traced chamfer_distance takes the composed path over the registered ops; eager takes the fused kernels for
    point_reduction "mean" / "sum" by default and the same composed path under deterministic mode, where everything
    is bit-equal.  In the default mode the fused and the composed sums differ in their order: the 1e-5 bar."""
    fn, leaves, need = _chamfer_call(dev, v)
    fused = v["point_reduction"] in ("mean", "sum")
    _assert_compiled_equals_eager(fn, leaves, need, atomics=True, fullgraph=True, forward_bitwise=not fused)


def test_inductor_chamfer_with_features(dev):
    v = dict(point_reduction="mean", batch_reduction="mean", single_directional=False, use_weights=True, features=True,
             abs_cosine=True, norm=2)
    fn, leaves, _ = _chamfer_call(dev, v)
    torch._dynamo.reset()
    e_out, e_g = _run(fn, leaves)
    c_out, c_g = _run(torch.compile(fn, fullgraph=True), leaves)
    for u, w in zip(list(e_out) + list(e_g), list(c_out) + list(c_g)):
        assert close(npy(w), npy(u))


# ------------------------------------------------------------------------------------------------ e. host caches
def test_host_caches_across_tracing(dev):
    from pytorch3d_pointops_amd.functions import _common, knn_points, sample_farthest_points

    a, b, _, _ = _clouds(dev)
    fn = lambda p, q: knn_points(p, q, K=roc.K)[:2]  # noqa: E731
    torch._dynamo.reset()
    compiled = torch.compile(fn, backend=Recorder(), fullgraph=True)
    want = fn(a, b)
    _common._LENGTHS_CACHE.clear()
    got = compiled(a, b)
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    again = fn(a, b)  # eager with the same (n, p)
    assert all(torch.equal(u, v) for u, v in zip(again, want))
    assert _common._LENGTHS_CACHE  # (the eager call above cached its default lengths: the loop below is not empty)
    for (n, p, index, _), t in _common._LENGTHS_CACHE.items():  # key: (n, p, device index, stream)
        assert type(t) is torch.Tensor and t.device == a.device and t.shape == (n,) and bool((t == p).all())
        assert index == a.device.index
    a2, b2 = a[:2, :40].contiguous(), b[:2, :77].contiguous()  # compiled again at another shape
    assert all(torch.equal(u, v) for u, v in zip(compiled(a2, b2), fn(a2, b2)))
    assert all(torch.equal(u, v) for u, v in zip(fn(a2, b2), knn_points(a2, b2, G(np.array([40, 40]), dev),
                                                                        G(np.array([77, 77]), dev), K=roc.K)[:2]))
    # lengths_max: compiled, eager, an in-place change of `lengths`, compiled and eager again
    lengths = G(np.array([roc.P1, 33, 9]), dev)
    fps = lambda p, l: sample_farthest_points(p, l, 7)  # noqa: E731
    c_fps = torch.compile(fps, backend=Recorder(), fullgraph=True)
    first = fps(a, lengths)
    assert all(torch.equal(u, v) for u, v in zip(c_fps(a, lengths), first))
    assert _common.lengths_max(lengths) == roc.P1
    lengths[0] = 20
    assert _common.lengths_max(lengths) == 33
    second = fps(a, lengths)
    assert not torch.equal(second[1], first[1])
    assert all(torch.equal(u, v) for u, v in zip(c_fps(a, lengths), second))
    lengths[1] = roc.P1 + 1  # too large: eager validates on the host
    with pytest.raises(ValueError):
        fps(a, lengths)
