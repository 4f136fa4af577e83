"""Every chamfer_distance route against the float64 reference of tests/chamfer_ref.py.

The routes: the native pair call (chamfer_pair_forward / _backward), the same pair with the grid cache on (two
chamfer_forward calls, the second backward accumulating), the per-direction fused node (weights or
single_directional), the composed path (point_reduction None / max, or _fused_direction_ok forced off) and the
deterministic composed path.  Each run asserts which route it took by counting calls.

The cases reach both fused backward kernels of csrc/chamfer.hip: chamfer_backward4_kernel (D <= 4 and every C <= 4)
and chamfer_backward_kernel (D >= 5, or any feature with C >= 5: d5, d8, d11, d5_c3, d8_c2, d11_c4_c16, c3_c5*,
c16*, c1_3_4_16*, lat_d5_l1_c5, big_c16 and the "generic" near-zero cases).  Five features and C = 17 must fall back
to the composed path on every route.

Tolerances: losses within 1e-5 * max(1, |ref|), gradients |a - b| <= 1e-4 |b| + 1e-5 max(1, max |b|) (the fuzz
test's rule).  Near-zero feature rows have a test of their own, so that their ~1e6 gradients do not widen the
tolerance of ordinary rows.
"""
import contextlib

import numpy as np
import pytest
import torch

from chamfer_ref import CachedKnn, chamfer_distance_ref, flatten_outputs

pytestmark = pytest.mark.gpu


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _feature(rng, shape):
    if shape[-1] == 1:  # one channel: cos = +-1; keep |f| away from 0, where fp32 rounding of f / |f| dominates
        return (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.2, 1.0, shape)).astype(np.float32)
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def _case(name, seed, D, feats=(), N=4, P1=70, P2=90, lattice=False, norm=2, abs_cosine=True, weights=None,
          pr="mean", br="mean", lengths="edges"):
    rng = np.random.default_rng(seed)
    if lattice:  # exact coordinate ties (L1 sign) and duplicate targets (index ties)
        x = (rng.integers(0, 4, (N, P1, D)) * 0.25).astype(np.float32)
        y = (rng.integers(0, 4, (N, P2, D)) * 0.25).astype(np.float32)
    else:
        x, y = rng.random((N, P1, D), dtype=np.float32), rng.random((N, P2, D), dtype=np.float32)
    if lengths == "edges":  # full / partial, x empty, y empty with x > 0, length 1
        xl = np.array([P1, 0, int(rng.integers(2, P1)), 1][:N], np.int64)
        yl = np.array([int(rng.integers(2, P2)), 1, 0, P2][:N], np.int64)
    elif lengths == "full":
        xl, yl = np.full(N, P1, np.int64), np.full(N, P2, np.int64)
    else:
        xl, yl = lengths
    fx = {f"f{i}": _feature(rng, (N, P1, C)) for i, C in enumerate(feats)}
    fy = {f"f{i}": _feature(rng, (N, P2, C)) for i, C in enumerate(feats)}
    w = None if weights is None else np.asarray(weights, np.float32)[:N]
    return dict(name=name, x=x, y=y, xl=xl, yl=yl, fx=fx, fy=fy, norm=norm, abs_cosine=abs_cosine, w=w, pr=pr,
                br=br, lattice=lattice)


W0 = [1.0, 0.0, 0.5, 2.0]  # a zero entry
W1 = [0.7, 1.3, 0.25, 1.0]


def _cases():
    c = []
    # point dimension sweep, no features (D >= 5: chamfer_backward_kernel)
    for i, D in enumerate((1, 2, 3, 4, 5, 8, 11)):
        c.append(_case(f"d{D}", 100 + D, D, norm=1 + i % 2, weights=W0 if i % 2 else None,
                       pr=("mean", "sum")[i % 2], br=("mean", "sum", None)[i % 3]))
    # feature widths at D = 3
    c += [
        _case("c1", 120, 3, (1,), weights=W1),
        _case("c1_noabs_l1", 121, 3, (1,), abs_cosine=False, norm=1, pr="sum", br=None),
        _case("c2", 122, 3, (2,), abs_cosine=False, weights=W0, br="sum"),
        _case("c2_l1", 123, 3, (2,), norm=1),
        _case("c3", 124, 3, (3,), weights=W1, pr="sum"),
        _case("c4", 125, 3, (4,), br=None),
        _case("c4_noabs_l1", 126, 3, (4,), abs_cosine=False, norm=1, weights=W0),
        _case("c3_c5", 127, 3, (3, 5)),
        _case("c3_c5_noabs_l1", 128, 3, (3, 5), abs_cosine=False, norm=1, weights=W1, pr="sum", br="sum"),
        _case("c16", 129, 3, (16,), weights=W0, br=None),
        _case("c16_noabs", 130, 3, (16,), abs_cosine=False, pr="sum"),
        _case("c1_3_4_16", 131, 3, (1, 3, 4, 16)),
        _case("c1_3_4_16_noabs_l1", 132, 3, (1, 3, 4, 16), abs_cosine=False, norm=1, weights=W1, br="sum"),
        _case("c2_2_2_2", 133, 3, (2, 2, 2, 2), abs_cosine=False, pr="sum", br=None),
        # fall-backs to the composed path
        _case("five_feats", 134, 3, (3, 1, 2, 4, 3), weights=W0),
        _case("c17", 135, 3, (17,), abs_cosine=False, pr="sum"),
        # features with other point dimensions
        _case("d1_c4", 136, 1, (4,), norm=1, weights=W1),
        _case("d2_c3", 137, 2, (3,), abs_cosine=False, br="sum"),
        _case("d4_c2_c1", 138, 4, (2, 1), pr="sum", br=None),
        _case("d5_c3", 139, 5, (3,), weights=W0),
        _case("d8_c2", 140, 8, (2,), abs_cosine=False, norm=1, pr="sum"),
        _case("d11_c4_c16", 141, 11, (4, 16), br=None),
        # lattices: coordinate ties, duplicate targets
        _case("lat_d3_l1", 142, 3, (3,), lattice=True, norm=1, weights=W1),
        _case("lat_d3_l2", 143, 3, (3,), lattice=True, abs_cosine=False, pr="sum"),
        _case("lat_d2_l1", 144, 2, lattice=True, norm=1, br=None),
        _case("lat_d1_l1", 145, 1, (2,), lattice=True, norm=1, weights=W0, P1=40, P2=30),
        _case("lat_d5_l1_c5", 146, 5, (5,), lattice=True, norm=1, pr="sum", br="sum"),
        _case("lat_d3_l1_c4", 147, 3, (4,), lattice=True, norm=1, abs_cosine=False, lengths="full", N=2),
        # one full cloud, a single point on each side
        _case("full_n1", 148, 3, (3,), N=1, P1=200, P2=150, lengths="full", weights=W1),
        _case("single_points", 149, 3, (3,), N=2, P1=1, P2=1, lengths="full", norm=1),
    ]
    # the grid K=1 search (D <= 3, P2 >= 4096): B = 3, ragged up to 20 000 points
    big = (np.array([20000, 13000, 4500]), np.array([17000, 20000, 9000]))
    c.append(_case("big_c3", 150, 3, (3,), N=3, P1=20000, P2=20000, lengths=big, weights=W1))
    c.append(_case("big_c16", 151, 3, (16,), N=3, P1=20000, P2=20000, lengths=big, abs_cosine=False, norm=1,
                   pr="sum", br=None))
    return c


CASES = _cases()


def _upstream(tag, shape):
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(tag)))
    return (rng.uniform(0.25, 1.25, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _fused_eligible(c):
    from pytorch3d_pointops_amd import _C

    return len(c["fx"]) <= _C.CHAMFER_MAX_FEATURES and all(
        v.shape[2] <= _C.CHAMFER_MAX_CHANNELS for v in c["fx"].values())


def _routes(c):
    """(route, call kwargs, mode): mode None, "cache", "forced" (fused path off) or "det"."""
    pr, br = c["pr"], c["br"]
    plain = dict(point_reduction=pr, batch_reduction=br)
    one_way = dict(plain, weights=c["w"]) if c["w"] is not None else dict(plain, single_directional=True)
    unreduced = dict(point_reduction=None, batch_reduction=None, weights=c["w"])
    if not c["fx"] and not c["lattice"]:  # (max: no ties in the maximum on continuous coordinates)
        unreduced = dict(point_reduction="max", batch_reduction=br, weights=c["w"])
    return [("pair", plain, None), ("grid_cache", plain, "cache"), ("direction", one_way, None),
            ("composed_unreduced", unreduced, None), ("composed_forced", one_way, "forced"),
            ("deterministic", one_way, "det")]


def _expected_calls(c, route, kw):
    """(chamfer_pair_forward, chamfer_forward, _direction_composed) call counts of the route."""
    dirs = 1 if kw.get("single_directional") else 2
    if not _fused_eligible(c) or route.startswith("composed") or route == "deterministic":
        return (0, 0, dirs)
    return {"pair": (1, 0, 0), "grid_cache": (0, 2, 0), "direction": (0, dirs, 0)}[route]


@contextlib.contextmanager
def _mode(monkeypatch, mode):
    import pytorch3d_pointops_amd.functions.chamfer as ch
    from pytorch3d_pointops_amd import _C

    if mode == "cache":
        prev = (_C.grid_cache_enabled(), _C._GRID_CACHE_MAX)
        _C.set_grid_cache(True)
        try:
            yield
        finally:
            _C.set_grid_cache(False)
            _C.set_grid_cache(*prev)
    elif mode == "det":
        torch.use_deterministic_algorithms(True)
        try:
            yield
        finally:
            torch.use_deterministic_algorithms(False)
    elif mode == "forced":
        with monkeypatch.context() as m:
            m.setattr(ch, "_fused_direction_ok", lambda *args, **kw: False)
            yield
    else:
        yield


def _counting(monkeypatch):
    import pytorch3d_pointops_amd.functions.chamfer as ch
    from pytorch3d_pointops_amd import _C

    calls = {"pair": 0, "forward": 0, "composed": 0}

    def wrap(owner, attr, key):
        fn = getattr(owner, attr)

        def counted(*args, **kw):
            calls[key] += 1
            return fn(*args, **kw)

        monkeypatch.setattr(owner, attr, counted)

    wrap(_C, "chamfer_pair_forward", "pair")
    wrap(_C, "chamfer_forward", "forward")
    wrap(ch, "_direction_composed", "composed")
    return calls


def _run_gpu(dev, c, kw):
    from pytorch3d_pointops_amd.functions.chamfer import chamfer_distance

    names = sorted(c["fx"])
    x, y = G(c["x"], dev).requires_grad_(True), G(c["y"], dev).requires_grad_(True)
    fx = {k: G(c["fx"][k], dev).requires_grad_(True) for k in names}
    fy = {k: G(c["fy"][k], dev).requires_grad_(True) for k in names}
    call = dict(kw)
    if call.get("weights") is not None:
        call["weights"] = G(call["weights"], dev)
    if names:
        call.update(x_features=fx, y_features=fy, feature_names=names)
    loss, lf = chamfer_distance(x, y, x_lengths=G(c["xl"], dev), y_lengths=G(c["yl"], dev), norm=c["norm"],
                                abs_cosine=c["abs_cosine"], **call)
    outs = flatten_outputs(loss, lf)
    total = sum((t * G(_upstream(tag, tuple(t.shape)), dev)).sum() for tag, t in outs)
    total.backward()

    def grad(t):
        return np.zeros(tuple(t.shape), np.float32) if t.grad is None else t.grad.cpu().numpy()

    return dict(outputs=[(tag, t.detach().cpu().numpy()) for tag, t in outs], grad_x=grad(x), grad_y=grad(y),
                grad_xf={k: grad(fx[k]) for k in names}, grad_yf={k: grad(fy[k]) for k in names})


def _run_ref(knn, c, kw):
    names = sorted(c["fx"])
    return chamfer_distance_ref(knn, c["x"], c["y"], c["xl"], c["yl"], x_features=c["fx"], y_features=c["fy"],
                                feature_names=names or None, norm=c["norm"], abs_cosine=c["abs_cosine"],
                                upstream=_upstream, **kw)


def _grad_ok(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    tol = 1e-4 * np.abs(b) + 1e-5 * max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    return a.shape == b.shape and bool((np.abs(a - b) <= tol).all())


def _compare(got, want, what):
    assert [t for t, _ in got["outputs"]] == [t for t, _ in want["outputs"]], what
    for (tag, a), (_, b) in zip(got["outputs"], want["outputs"]):
        assert a.shape == b.shape, (what, tag)
        err = np.abs(a.astype(np.float64) - b)
        assert (err <= 1e-5 * np.maximum(1.0, np.abs(b))).all(), (what, tag, float(err.max()))
    for key in ("grad_x", "grad_y"):
        assert _grad_ok(got[key], want[key]), (what, key, float(np.abs(got[key] - want[key]).max()))
    for key in ("grad_xf", "grad_yf"):
        for k in want[key]:
            assert _grad_ok(got[key][k], want[key][k]), (what, key, k,
                                                         float(np.abs(got[key][k] - want[key][k]).max()))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_chamfer_routes_vs_float64(dev, oracle, monkeypatch, c):
    from pytorch3d_pointops_amd import _C

    knn = CachedKnn(oracle)
    for key, a, b, la, lb in (("xy", c["x"], c["y"], c["xl"], c["yl"]), ("yx", c["y"], c["x"], c["yl"], c["xl"])):
        idx, _ = _C.knn_points_idx(G(a, dev), G(b, dev), G(la, dev), G(lb, dev), c["norm"], 1, -1)
        assert np.array_equal(idx[..., 0].cpu().numpy(), knn(key, a, b, la, lb, c["norm"])), (c["name"], key)
    calls = _counting(monkeypatch)
    refs = {}
    for route, kw, mode in _routes(c):
        for k in calls:
            calls[k] = 0
        with _mode(monkeypatch, mode):
            got = _run_gpu(dev, c, kw)
        assert (calls["pair"], calls["forward"], calls["composed"]) == _expected_calls(c, route, kw), \
            (c["name"], route, calls)
        sig = repr(sorted((k, None if v is None else np.asarray(v).tolist()) for k, v in kw.items()))
        if sig not in refs:
            refs[sig] = _run_ref(knn, c, kw)
        _compare(got, refs[sig], (c["name"], route))


# ------------------------------------------------------------------ near-zero feature vectors
NEAR_ZERO_NORMS = (0.0, 1e-8, 3e-7, 9e-7, 2e-6, 1.0)  # eps = 1e-6; none within 1 % of it


def _near_zero_case(widths):
    rng = np.random.default_rng(160)
    N, P1, P2 = 2, 300, 12  # 12 targets: each y row is the nearest neighbour of ~25 queries

    def feats(P, C, shift):
        v = rng.standard_normal((N, P, C))
        v /= np.linalg.norm(v, axis=2, keepdims=True)
        norms = np.array(NEAR_ZERO_NORMS)[(np.arange(P) + shift) % len(NEAR_ZERO_NORMS)]
        return (v * norms[None, :, None]).astype(np.float32)

    return dict(name="near_zero", x=rng.random((N, P1, 3), dtype=np.float32),
                y=rng.random((N, P2, 3), dtype=np.float32), xl=np.array([P1, 211]), yl=np.array([P2, 9]),
                fx={f"f{i}": feats(P1, C, i) for i, C in enumerate(widths)},
                fy={f"f{i}": feats(P2, C, i + 1) for i, C in enumerate(widths)}, norm=2, lattice=False)


NEAR_ZERO_ROUTES = {  # (call kwargs, fused path off, expected call counts)
    "pair": (dict(point_reduction="sum", batch_reduction=None), None, (1, 0, 0)),
    "direction": (dict(point_reduction="mean", batch_reduction="sum", weights=np.array([1.0, 0.5])), None, (0, 2, 0)),
    "composed_forced": (dict(point_reduction="sum", batch_reduction=None), "forced", (0, 0, 2)),
}


@pytest.mark.parametrize("route", sorted(NEAR_ZERO_ROUTES))
@pytest.mark.parametrize("abs_cosine", [True, False])
@pytest.mark.parametrize("widths", [(3,), (3, 6)], ids=["backward4", "generic"])
def test_chamfer_near_zero_features_vs_float64(dev, oracle, monkeypatch, widths, abs_cosine, route):
    """Feature rows with |f| in {0, 1e-8, 3e-7, 9e-7, 2e-6, 1} on both sides: the fused backward follows ATen's
    cosine_similarity gradient, including the band 0 < |f| <= eps where the clamped norm still passes the term
    through |f| (d cos/dx = y_hat / max(|x|, eps) - cos x_hat / |x|).  Feature gradients within 1e-4 max |ref|."""
    c = dict(_near_zero_case(widths), abs_cosine=abs_cosine)
    kw, mode, expect = NEAR_ZERO_ROUTES[route]
    calls = _counting(monkeypatch)
    with _mode(monkeypatch, mode):
        got = _run_gpu(dev, c, kw)
    assert (calls["pair"], calls["forward"], calls["composed"]) == expect, calls
    want = _run_ref(CachedKnn(oracle), c, kw)
    for (tag, a), (_, b) in zip(got["outputs"], want["outputs"]):
        assert (np.abs(a - b) <= 1e-5 * np.maximum(1.0, np.abs(b))).all(), tag
    assert _grad_ok(got["grad_x"], want["grad_x"]) and _grad_ok(got["grad_y"], want["grad_y"])
    for key in ("grad_xf", "grad_yf"):
        for k, b in want[key].items():
            err = float(np.abs(got[key][k] - b).max())
            assert err <= 1e-4 * float(np.abs(b).max()), (key, k, err, float(np.abs(b).max()))
