"""The operator table of tests/test_streams_devices_gpu.py: every operator of the package at the smallest shape that
reaches each of its kernel paths, as (inputs, call, expected value).

An entry's inputs come in numbered DATA SETS of one shape (0: the data a test checks, 1: the decoy its buffers hold
before the real data is copied in on the stream under test, 2: the data of the second stream of a two-stream test),
built by the existing tests' builders with the seeds moved by `SEED_STEP` per set.  `data` arrays are what a test copies
into the buffers on its stream; `static` values (lengths, sizes) are ready before the test starts.

Expected values: the CPU oracle, bit for bit, wherever it has the operator (`expect`); for the operators the README
calls bit-reproducible (`expect is None`) the result of the same call on the default stream of cuda:0, which those
operators' own test files pin to float64.  `kinds` names the comparison of each output: "bits", "atomic" (a gradient
accumulated with fp32 atomics: the tolerance of tests/test_graph_capture_gpu.py) or "loss" (its rtol 1e-5).
"""
import contextlib
import os

import numpy as np
import torch

import cases
from oracle import oracle as oracle_module
from pytorch3d_pointops_amd import synth

SEED_STEP = 50000


class Entry:
    def __init__(self, name, build, run, expect=None, kinds=None, grad=(), env=None, syncs=None, prove=None,
                 concurrent=True):
        self.name, self.build, self.run, self.expect, self.kinds = name, build, run, expect, kinds
        self.grad = tuple(grad)  # data keys whose buffers require grad
        self.env = env  # POINTOPS_DEBUG knobs that select the path
        self.syncs = syncs  # why the call reads back from the device by design (then: values only), or None
        self.prove = prove  # prove(t): the entry reaches the path it names (run once, default stream, real data)
        self.concurrent = concurrent  # may run next to another kernel (False: the multi-workgroup FPS exchange)
        self._inputs, self._expected = {}, {}

    def inputs(self, k, oracle):
        if k not in self._inputs:
            self._inputs[k] = self.build(k * SEED_STEP, oracle)
        return self._inputs[k]

    def expected(self, k, oracle):
        """Oracle outputs of data set k (computed once, never modified), or None for a bit-reproducible operator."""
        if self.expect is None:
            return None
        if k not in self._expected:
            data, static = self.inputs(k, oracle)
            self._expected[k] = tuple(np.asarray(v) for v in self.expect(oracle, {**data, **static}))
        return self._expected[k]

    def tensors(self, k, oracle, device):
        """(data, static) of data set k as tensors on `device` (the data buffers of `grad` require grad)."""
        data, static = self.inputs(k, oracle)
        d = {n: torch.from_numpy(v).to(device).requires_grad_(n in self.grad) for n, v in data.items()}
        s = {n: torch.from_numpy(v).to(device) if isinstance(v, np.ndarray) else v for n, v in static.items()}
        return d, s

    @contextlib.contextmanager
    def knobs(self):
        old = os.environ.get("POINTOPS_DEBUG")
        if self.env is not None:
            os.environ["POINTOPS_DEBUG"] = self.env
        try:
            yield
        finally:
            if self.env is not None:
                if old is None:
                    del os.environ["POINTOPS_DEBUG"]
                else:
                    os.environ["POINTOPS_DEBUG"] = old

    def __repr__(self):
        return self.name


def same(got, want, kind):
    """None when `got` matches `want` under the comparison `kind`, else a description of the mismatch."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    if kind == "bits":
        view = np.int32 if got.dtype == np.float32 else got.dtype
        bad = np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view)
        return f"{int(bad.sum())} of {bad.size} elements differ" if bad.any() else None
    if kind == "loss":
        return None if np.allclose(got, want, rtol=1e-5) else f"{got!r} vs {want!r}"
    assert kind == "atomic", kind
    tol = 2e-5 * np.abs(want) + 2e-6 * max(1e-3, float(np.abs(want).max()) if want.size else 0.0)
    bad = ~(np.abs(got - want) <= tol)
    return f"{int(bad.sum())} of {bad.size} elements beyond the atomic tolerance" if bad.any() else None


def _full(n, p):
    return np.full((n,), p, np.int64)


def _lengths(v, key, p):
    """The lengths of an oracle call: the entry's, or full clouds where the call passes None."""
    return v[key] if v.get(key) is not None else _full(p.shape[0], p.shape[1])


# ------------------------------------------------------------------------------------------------------------- knn
def _knn(name, clouds, K, version, norm=2, lengths=None, env=None, prove=None):
    """knn_points on `clouds(seed offset) -> (p1, p2)`; `lengths` = (l1, l2) lists or None (the default lengths)."""
    def build(s, oracle):
        p1, p2 = clouds(s)
        l1, l2 = (None, None) if lengths is None else (np.array(lengths[0]), np.array(lengths[1]))
        return dict(p1=p1, p2=p2), dict(l1=l1, l2=l2)

    def run(t):
        from pytorch3d_pointops_amd.functions import knn_points

        r = knn_points(t["p1"], t["p2"], t["l1"], t["l2"], norm=norm, K=K, version=version)
        return r.idx, r.dists

    def expect(oracle, v):
        return oracle.knn_points_idx(v["p1"], v["p2"], _lengths(v, "l1", v["p1"]), _lengths(v, "l2", v["p2"]), norm, K)

    return Entry(name, build, run, expect, ("bits", "bits"), env=env, prove=prove)


def _uniform(seed1, seed2, shape1, shape2):
    return lambda s: (cases.cloud(seed1 + s, shape1), cases.cloud(seed2 + s, shape2))


def _refined_clouds(s):  # test_knn_refined_cells_and_box_search
    m = 24000
    a = cases.cloud(2601 + s, (3, 5000, 3))
    b = cases.cloud(2602 + s, (3, m, 3))
    a[0, :2500] = a[0, :2500] * np.float32(1e-3) + np.float32(0.5)
    b[0, : m // 2] = b[0, : m // 2] * np.float32(1e-3) + np.float32(0.5)
    a[1], b[1] = (a[1] ** np.float32(5.0)).astype(np.float32), (b[1] ** np.float32(5.0)).astype(np.float32)
    b[2, : m // 3] = b[2, 0]
    return a, b


def _prove_refined(t):
    """Diagnostics column 9 (refined cells) > 0: the refine kernel with its 128 KB of dynamic LDS really ran."""
    from pytorch3d_pointops_amd import _C

    l1 = t["l1"] if t["l1"] is not None else torch.full((3,), 5000, dtype=torch.int64, device=t["p1"].device)
    l2 = t["l2"] if t["l2"] is not None else torch.full((3,), 24000, dtype=torch.int64, device=t["p1"].device)
    st = _C.knn_grid_stats(t["p1"], t["p2"], l1, l2, 2, 8)[2].cpu().numpy()
    assert (st[:2, 9] > 0).all(), st


def _long_list_clouds(s):  # test_knn_grid_long_lists
    p1 = cases.cloud(2501 + s, (4, 2500, 3))
    p2 = cases.cloud(2502 + s, (4, 12000, 3))
    p2[1] = (p2[1] ** np.float32(3.0)).astype(np.float32)
    p2[3, :, :] = p2[3, :1, :]
    return p1, p2


def _wave_sort_clouds(s):  # test_knn_grid_wave_sort_long_lists
    p1 = cases.cloud(3801 + s, (4, 1500, 3))
    p2 = cases.cloud(3802 + s, (4, 30000, 3))
    p2[1, :20000] = p2[1, :20000] * np.float32(3e-3) + np.float32(0.4)
    p2[2, 1::2] = p2[2, ::2]
    return p1, p2


def _wide_lattice(s):  # the d3_k100 row of test_knn_wide_shapes
    return cases.lattice(1703 + s, 3, 200, 3, levels=5), cases.lattice(1702 + s, 3, 1000, 3, levels=5)


def _knn_backward(name, deterministic):
    """Backward of a K = 4 search (the shapes of test_graph_capture_gpu's knn_backward case), with fp32 atomics or
    under torch.use_deterministic_algorithms(True): (grad_p1, grad_p2) of (dists * upstream).sum()."""
    shape = (2, 1024, 4)

    def build(s, oracle):
        return dict(p1=cases.cloud(32 + s, (2, 1024, 3)), p2=cases.cloud(33 + s, (2, 1500, 3)),
                    up=cases.grad_for(name + str(s), shape)), {}

    def run(t):
        from pytorch3d_pointops_amd.functions import knn_points

        was = torch.are_deterministic_algorithms_enabled()
        try:
            torch.use_deterministic_algorithms(deterministic)
            loss = (knn_points(t["p1"], t["p2"], K=4).dists * t["up"]).sum()
            return torch.autograd.grad(loss, [t["p1"], t["p2"]])
        finally:
            torch.use_deterministic_algorithms(was)

    def expect(oracle, v):
        l1, l2 = _full(2, 1024), _full(2, 1500)
        idx, _ = oracle.knn_points_idx(v["p1"], v["p2"], l1, l2, 2, 4)
        return oracle.knn_points_backward(v["p1"], v["p2"], l1, l2, idx, 2, v["up"])

    # grad_p1 is a per-query register sum in the CPU kernel's order; grad_p2 is scattered
    return Entry(name, build, run, expect, ("bits", "bits" if deterministic else "atomic"), grad=("p1", "p2"))


# ------------------------------------------------------------------------------------------------------ ball query
def _ball(name, clouds, K, radius, lengths=None, env=None):
    def build(s, oracle):
        p1, p2 = clouds(s)
        l1, l2 = (None, None) if lengths is None else (np.array(lengths[0]), np.array(lengths[1]))
        return dict(p1=p1, p2=p2), dict(l1=l1, l2=l2)

    def run(t):
        from pytorch3d_pointops_amd.functions import ball_query

        r = ball_query(t["p1"], t["p2"], t["l1"], t["l2"], K=K, radius=radius, return_nn=False)
        return r.idx, r.dists

    def expect(oracle, v):
        return oracle.ball_query(v["p1"], v["p2"], _lengths(v, "l1", v["p1"]), _lengths(v, "l2", v["p2"]), K, radius)

    return Entry(name, build, run, expect, ("bits", "bits"), env=env)


def _ball_grid_clouds(s):  # test_ball_query_grid_vs_oracle
    p1 = cases.cloud(1801 + s, (3, 3000, 3))
    p2 = cases.cloud(1802 + s, (3, 20000, 3))
    p2[1] = (p2[1] ** np.float32(3.0)).astype(np.float32) + np.float32(10.0)
    p1[1] = (p1[1] ** np.float32(3.0)).astype(np.float32) + np.float32(10.0)
    return p1, p2


# -------------------------------------------------------------------------------------------------------------- FPS
def _fps(name, shape, seed, K, lengths=None, env=None, tensor_K=False, concurrent=True):
    """sample_farthest_points with an int K (no device-to-host read) or, `tensor_K`, a device tensor K."""
    def build(s, oracle):
        static = dict(lengths=None if lengths is None else np.array(lengths))
        if tensor_K:
            static["K"] = np.full((shape[0],), K, np.int64)
        return dict(points=cases.cloud(seed + s, shape)), static

    def run(t):
        from pytorch3d_pointops_amd.functions import sample_farthest_points

        return sample_farthest_points(t["points"], t["lengths"], t["K"] if tensor_K else K)

    def expect(oracle, v):
        n = shape[0]
        idx = oracle.sample_farthest_points(v["points"], _lengths(v, "lengths", v["points"]),
                                            np.full((n,), K, np.int64), np.zeros((n,), np.int64))
        return oracle_module.masked_gather(v["points"], idx), idx

    return Entry(name, build, run, expect, ("bits", "bits"), env=env, concurrent=concurrent,
                 syncs="a tensor K is read back for max(K), as in the reference" if tensor_K else None)


# ----------------------------------------------------------------------------------------------------- small operators
def _gather():
    """knn_gather forward and backward (the shapes of test_graph_capture_gpu's gather_backward case)."""
    def build(s, oracle):
        return dict(x=cases.cloud(35 + s, (2, 1500, 3)), idx=synth.randint(34 + s, 0, 1499, (2, 1024, 8)),
                    up=cases.grad_for("gather" + str(s), (2, 1024, 8, 3))), {}

    def run(t):
        from pytorch3d_pointops_amd.functions import knn_gather

        out = knn_gather(t["x"], t["idx"])
        return out.detach(), torch.autograd.grad((out * t["up"]).sum(), [t["x"]])[0]

    def expect(oracle, v):
        grad = np.zeros(v["x"].shape, np.float64)
        for n in range(grad.shape[0]):
            np.add.at(grad[n], v["idx"][n].reshape(-1), v["up"][n].reshape(-1, 3).astype(np.float64))
        return oracle_module.knn_gather(v["x"], v["idx"]), grad.astype(np.float32)

    return Entry("knn_gather", build, run, expect, ("bits", "atomic"), grad=("x",))


def _packed():
    case = cases.packed_cases()["d4_wide_pad"]

    def build(s, oracle):
        x, first, total = cases.packed_inputs(dict(case, seed=case["seed"] + s))
        return dict(x=x), dict(first=first, total=total)

    def run(t):
        from pytorch3d_pointops_amd.functions import packed_to_padded, padded_to_packed

        padded = packed_to_padded(t["x"], t["first"], case["max_size"])
        return padded, padded_to_packed(padded, t["first"], t["total"])

    def expect(oracle, v):
        padded = oracle.packed_to_padded(v["x"], v["first"], case["max_size"])
        return padded, oracle.padded_to_packed(padded, v["first"], v["total"])

    return Entry("packed_padded", build, run, expect, ("bits", "bits"))


def _sample_pdf():
    """The operator boundary (the public wrapper checks the weights' sign on the host first: a device-to-host read)."""
    def build(s, oracle):
        batch, nb, ns = 8, 64, 128
        bins = np.sort(synth.uniform_f32(701 + s, (batch, nb + 1)), axis=1).astype(np.float32)
        w = synth.uniform_f32(711 + s, (batch, nb))
        w[0, : nb // 3] = 0.0
        u = synth.uniform_f32(721 + s, (batch, ns))
        u[0, 0], u[0, -1] = 0.0, 1.0
        return dict(bins=bins, weights=w, u=u), {}

    def run(t):
        from pytorch3d_pointops_amd import _C

        out = t["u"].clone()
        _C.sample_pdf(t["bins"], t["weights"], out, 1e-5)
        return (out,)

    def expect(oracle, v):
        return (oracle.sample_pdf(v["bins"], v["weights"], v["u"], 1e-5),)

    return Entry("sample_pdf", build, run, expect, ("bits",))


# ------------------------------------------------------------------------------- bit-reproducible operators (no oracle)
def _covariances():
    def run(t):
        from pytorch3d_pointops_amd.functions import get_point_covariances

        return get_point_covariances(t["points"], t["lengths"], 8)

    return Entry("point_covariances", lambda s, o: (dict(points=cases.cloud(1601 + s, (2, 600, 3))),
                                                    dict(lengths=np.array([600, 555]))), run, kinds=("bits", "bits"))


def _normals():
    def run(t):
        from pytorch3d_pointops_amd.functions import estimate_pointcloud_normals

        return (estimate_pointcloud_normals(t["points"], 16),)

    return Entry("normals", lambda s, o: (dict(points=cases.cloud(1611 + s, (2, 2048, 3))), {}), run, kinds=("bits",))


def _alignment_inputs(s, oracle):
    from test_points_alignment_gpu import _moved

    X = cases.cloud(1621 + s, (2, 3000, 3))
    return dict(X=X, Y=_moved(torch.from_numpy(X), 1622 + s).numpy()), {}


def _alignment(native):
    def run(t):
        from pytorch3d_pointops_amd import _C
        from pytorch3d_pointops_amd.functions import corresponding_points_alignment

        if native:
            return _C.points_alignment(t["X"], t["Y"], None, None, None, False, False, 1e-9)[:4]
        return tuple(corresponding_points_alignment(t["X"], t["Y"]))

    return Entry("alignment_native" if native else "alignment", _alignment_inputs, run,
                 kinds=("bits",) * (4 if native else 3),
                 syncs=None if native else "the wrapper reads its two warning flags back from the device")


def _icp_inputs(s, oracle):
    from test_points_alignment_gpu import _subset_setup

    X, Y, lx, ly, _ = _subset_setup(1631 + s, [(1500, 2000), (1500, 2000)], noise=0.01)
    return dict(X=X.numpy(), Y=Y.numpy()), dict(lx=lx.numpy(), ly=ly.numpy())


def _icp(native):
    def run(t):
        from pytorch3d_pointops_amd import _C
        from pytorch3d_pointops_amd.functions import iterative_closest_point

        if native:  # the stepping primitive: three iterations enqueued without a read
            state = _C.IcpState(t["X"], t["X"].clone(), t["Y"], t["lx"], t["ly"], 3, False, False, 1e-6)
            for _ in range(3):
                state.step()
            return state.R, state.T, state.s, state.Xt, state.rmse
        sol = iterative_closest_point(t["X"], t["Y"], max_iterations=3)
        return (sol.rmse, sol.Xt) + tuple(sol.RTs)

    return Entry("icp_steps" if native else "icp", _icp_inputs, run, kinds=("bits",) * 5,
                 syncs=None if native else "every iteration reads its convergence flag back")


def _fpfh():
    def build(s, oracle):
        pts = cases.cloud(1641 + s, (2, 2048, 3))
        idx, _ = oracle.knn_points_idx(pts, pts, _full(2, 2048), _full(2, 2048), 2, 16)
        return dict(points=pts, normals=synth.unit_normals(1642 + s, (2, 2048, 3)), idx=idx), {}

    def run(t):
        from pytorch3d_pointops_amd.functions import fpfh_features

        return fpfh_features(t["points"], t["normals"], None, idx=t["idx"], return_spfh=True)

    return Entry("fpfh", build, run, kinds=("bits", "bits"))


# ---------------------------------------------------------------------------------------------------------- chamfer
def _chamfer_expect(oracle, v):
    x, y = v["x"], v["y"]
    n = x.shape[0]
    lx, ly = _lengths(v, "lx", x), _lengths(v, "ly", y)
    i1, d1 = oracle.knn_points_idx(x, y, lx, ly, 2, 1)
    i2, d2 = oracle.knn_points_idx(y, x, ly, lx, 2, 1)
    per_cloud = d1.astype(np.float64).sum((1, 2)) / lx + d2.astype(np.float64).sum((1, 2)) / ly
    g1 = np.broadcast_to((1.0 / (n * lx))[:, None, None], d1.shape).astype(np.float32)
    g2 = np.broadcast_to((1.0 / (n * ly))[:, None, None], d2.shape).astype(np.float32)
    ax, ay = oracle.knn_points_backward(x, y, lx, ly, i1, 2, g1)
    by, bx = oracle.knn_points_backward(y, x, ly, lx, i2, 2, g2)
    return np.float32(per_cloud.sum() / n), ax + bx, ay + by


def _chamfer(name, N, P1, P2, lengths, overlap):
    """chamfer_distance forward and backward (point and batch reduction "mean"): the loss and both gradients against a
    chamfer built from the oracle's two K = 1 searches and their backward.  `overlap`: both searches take the grid, so
    the reverse one runs on the library's side stream -- asserted through pointops_knn_uses_grid."""
    def build(s, oracle):
        lx, ly = (None, None) if lengths is None else (np.array(lengths[0]), np.array(lengths[1]))
        return dict(x=cases.cloud(7 + s, (N, P1, 3)), y=cases.cloud(8 + s, (N, P2, 3))), dict(lx=lx, ly=ly)

    def run(t):
        from pytorch3d_pointops_amd.functions.chamfer import chamfer_distance

        loss, _ = chamfer_distance(t["x"], t["y"], x_lengths=t["lx"], y_lengths=t["ly"])
        return (loss.detach(),) + tuple(torch.autograd.grad(loss, [t["x"], t["y"]]))

    def prove(t):
        from pytorch3d_pointops_amd import _C

        uses_grid = _C._lib.pointops_knn_uses_grid
        grid = (uses_grid(N, P1, P2, 3, 1, -1), uses_grid(N, P2, P1, 3, 1, -1))
        assert grid == ((1, 1) if overlap else (0, 0)), grid

    return Entry(name, build, run, _chamfer_expect, ("loss", "atomic", "atomic"), grad=("x", "y"), prove=prove)


def _table():
    ragged_fps = [500, 120, 33, 1]
    chamfer_small = ([2048, 1500, 1100, 2000], [1500, 800, 1400, 1000])  # test_graph_capture_gpu's lengths
    entries = [
        # knn_points, one entry per kernel family
        _knn("knn_small", _uniform(5101, 5102, (2, 1024, 3), (2, 1024, 3)), 8, -1),  # wave per query
        # (2 x 3000 queries are few enough for the wave-per-query kernel: the knob keeps version 2 on the register
        # scan, with its p2 slices and merge pass)
        _knn("knn_scan", _uniform(5111, 5112, (2, 3000, 3), (2, 3000, 3)), 8, 2, env="knn_small=0"),
        _knn("knn_refined", _refined_clouds, 8, 3, lengths=([5000, 5000, 1234], [24000, 24000, 23995]),
             prove=_prove_refined),
        _knn("knn_refined_full", _refined_clouds, 8, 3, prove=_prove_refined),
        _knn("knn_grid_k40", _long_list_clouds, 40, 3, lengths=([2500, 2500, 900, 300], [12000, 7000, 37, 12000])),
        _knn("knn_grid_k40_full", _long_list_clouds, 40, 3),
        _knn("knn_grid_k100", _wave_sort_clouds, 100, 3, lengths=([1500, 1500, 1500, 40], [30000, 30000, 21000, 93])),
        _knn("knn_grid_k100_full", _wave_sort_clouds, 100, 3),
        _knn("knn_wide_d16_k8", _uniform(1716, 1725, (2, 130, 16), (2, 400, 16)), 8, 0, lengths=([130, 77], [400, 50])),
        _knn("knn_wide_d16_k8_full", _uniform(1716, 1725, (2, 130, 16), (2, 400, 16)), 8, 0),
        _knn("knn_wide_k100", _wide_lattice, 100, 0, lengths=([200, 0, 64], [1000, 900, 0])),
        _knn("knn_wide_k100_full", _wide_lattice, 100, 0),
        # (K = 100 lists fit 52 KB of LDS; the `_WIDE` row that needs the raised limit -- 154 KB -- is K = 300)
        _knn("knn_wide_k300", _uniform(1703, 2004, (1, 64, 3), (1, 700, 3)), 300, 0),
        _knn_backward("knn_backward_atomic", False),
        _knn_backward("knn_backward_deterministic", True),
        # ball_query
        _ball("ball_small", _uniform(201, 202, (3, 120, 3), (3, 400, 3)), 16, 0.2,
              lengths=([120, 33, 0], [400, 250, 10])),
        _ball("ball_small_full", _uniform(201, 202, (3, 120, 3), (3, 400, 3)), 16, 0.2),
        _ball("ball_scan", _uniform(1501, 1502, (2, 3000, 3), (2, 20000, 3)), 16, 0.05,
              lengths=([3000, 1234], [20000, 6000]), env="ball_small=0"),
        _ball("ball_scan_full", _uniform(1501, 1502, (2, 3000, 3), (2, 20000, 3)), 16, 0.05, env="ball_small=0"),
        _ball("ball_grid", _ball_grid_clouds, 16, 0.05, lengths=([3000, 1234, 77], [20000, 6000, 0]),
              env="ball_grid=1"),
        _ball("ball_grid_full", _ball_grid_clouds, 16, 0.05, env="ball_grid=1"),
        # sample_farthest_points
        _fps("fps_small", (4, 500, 3), 301, 32, lengths=ragged_fps),  # four-wave kernel
        _fps("fps_small_full", (4, 500, 3), 301, 32),
        _fps("fps_cluster", (4, 500, 3), 301, 32, lengths=ragged_fps, env="fps_small=0"),  # one workgroup per cloud
        _fps("fps_cluster_full", (4, 500, 3), 301, 32, env="fps_small=0"),
        _fps("fps_multi_workgroup", (2, 10000, 3), 1410, 16, concurrent=False),  # three workgroups per cloud
        _fps("fps_tensor_K", (4, 500, 3), 301, 32, tensor_K=True),
        # the other operators
        _gather(), _packed(), _sample_pdf(), _covariances(), _normals(), _alignment(True), _alignment(False),
        _icp(True), _icp(False), _fpfh(),
        # chamfer_distance
        _chamfer("chamfer_small", 4, 2048, 1500, chamfer_small, overlap=False),
        _chamfer("chamfer_small_full", 4, 2048, 1500, None, overlap=False),
        _chamfer("chamfer_overlap", 1, 14336, 14336, ([13000], [14336]), overlap=True),
        _chamfer("chamfer_overlap_full", 1, 14336, 14336, None, overlap=True),
    ]
    return {e.name: e for e in entries}


TABLE = _table()
