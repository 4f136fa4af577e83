"""knn_features on the device (csrc/feature_topk.hip, _C_feature_topk.py, functions/knn_features.py):
    search       _C_feature_topk.feature_topk equals _C.knn_points_idx byte for byte -- and tests/match_ref.py on finite
                 cases -- with POINTOPS_DEBUG unset, topk_screen=0 (the exact search) and topk_screen=1 with topk_split=1
                 and 4, at the block, tile and list edges and on the special cases of tests/match_cases.py
    certificate  the rows the kernel sends to its exact fallback are the rows tests/feature_topk_ref.py predicts: an
                 equality, per cloud
    operator     knn_features equals knn_points field by field; its gradients; twice; from a HIP graph; on a side
                 stream; under the buffer contract
The knobs are read at call time, so every path runs in this process."""
import numpy as np
import pytest
import torch

import buffers
import feature_topk_ref as tref
import match_cases as cases
import match_ref as ref
from test_boundary_cpu import declared_prototypes
from test_match_gpu import _case_tensors, _dev, _same_bytes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
ENTRY = "pointops_feature_topk"
MODES = {"unset": None, "exact": "topk_screen=0", "S1": "topk_screen=1,topk_split=1", "S4": "topk_screen=1,topk_split=4"}
LISTS = {"S1": 2, "S4": 8}
KS = (1, 3, 16, 17, 20, 32)
CASES = cases.build_cases()


def _mode(monkeypatch, mode):
    if MODES[mode] is None:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    else:
        monkeypatch.setenv("POINTOPS_DEBUG", MODES[mode])


def _check_every_mode(monkeypatch, t, arrays, finite, K, what, screened=True, certified_none=False):
    """feature_topk against knn_points_idx (and the checker's search) in the four modes; the stats of each."""
    from pytorch3d_pointops_amd import _C, _C_feature_topk

    f1, f2, l1, l2 = arrays
    _mode(monkeypatch, "unset")
    want_i, want_d = _C.knn_points_idx(*t, 2, K)
    if finite and f1.shape[0]:
        ri, rd = ref.knn(f1, f2, l1, l2, K)
        _same_bytes(want_i, ri, f"{what}: knn_points_idx against the checker (idx)")
        _same_bytes(want_d, rd, f"{what}: knn_points_idx against the checker (dists)")
    live = np.where(np.clip(l2, 0, f2.shape[1]) > 0, np.clip(l1, 0, f1.shape[1]), 0)
    for mode in MODES:
        _mode(monkeypatch, mode)
        idx, dists, stats = _C_feature_topk.feature_topk(*t, K)
        _same_bytes(idx, want_i, f"{what} [{mode}] (idx)")
        _same_bytes(dists, want_d, f"{what} [{mode}] (dists)")
        stats = stats.cpu().numpy()
        assert stats.shape == (f1.shape[0], 4) and stats.dtype == np.int32
        if mode in LISTS and screened and f1.shape[1] and f2.shape[1]:
            assert (stats[:, 0] == 1).all() and (stats[:, 3] == LISTS[mode]).all() and (stats[:, 1] >= 0).all(), what
            assert np.array_equal(stats[:, 1] + stats[:, 2], live), f"{what} [{mode}]: certified + listed = live rows"
            if certified_none:
                assert not stats[:, 1].any(), f"{what} [{mode}]: a row out of the bound's range was certified"
        elif mode != "unset":
            assert not stats.any(), f"{what} [{mode}]: the exact search reports no screen"


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("D", [9, 33, 64, 128])
@pytest.mark.parametrize("P1,P2", [(1, 1), (33, 17), (129, 127), (130, 128), (65, 129), (257, 1037)])
def test_search_equals_knn_points_on_every_path(dev, monkeypatch, P1, P2, D):
    rng = np.random.default_rng(1000 * P1 + D)
    f1, f2 = (rng.standard_normal((2, P, D)).astype(np.float32) for P in (P1, P2))
    l1, l2 = np.array([P1, (P1 + 1) // 2]), np.array([P2, max(P2 - 3, 1)])
    t = _dev(dev, f1, f2, l1, l2)
    for K in KS:
        _check_every_mode(monkeypatch, t, (f1, f2, l1, l2), True, K, f"{P1}x{P2} D={D} K={K}")


@pytest.mark.parametrize("K", [3, 20])
def test_ragged_lengths_around_k_and_the_list_size(dev, monkeypatch, K):
    rng = np.random.default_rng(K)
    f1, f2 = cases.fpfh_like(rng, (7, 40)), cases.fpfh_like(rng, (7, 40))
    l1, l2 = np.array([40, 40, 0, 40, 33, 40, 1]), np.array([0, 1, 40, K - 1, K, 16, 17])
    _check_every_mode(monkeypatch, _dev(dev, f1, f2, l1, l2), (f1, f2, l1, l2), True, K, f"ragged K={K}")


@pytest.mark.parametrize("name", ["N0", "self", "nan-and-inf-rows", "huge", "wide-groups-D33"])
def test_special_cases(dev, monkeypatch, name):
    """An empty batch; p1 is p2; rows of NaN and of +-inf; norms of 2^126, where no row is certified; 64 x 1999 queries
    over 150 ragged targets: every wave has queries and the last workgroup is part full."""
    c = CASES[name]
    _check_every_mode(monkeypatch, _case_tensors(dev, c), (c.f1, c.f2, c.lengths1, c.lengths2), c.finite, 20,
                      f"{name} K=20", certified_none=name == "huge")


@pytest.mark.parametrize("D,K", [(129, 20), (33, 33)])
def test_shapes_outside_the_screen_take_the_exact_search(dev, monkeypatch, D, K):
    rng = np.random.default_rng(D + K)
    f1, f2 = (rng.standard_normal((2, P, D)).astype(np.float32) for P in (70, 90))
    l1, l2 = np.array([70, 5]), np.array([90, 40])
    _check_every_mode(monkeypatch, _dev(dev, f1, f2, l1, l2), (f1, f2, l1, l2), True, K, f"D={D} K={K}", screened=False)


# ------------------------------------------------------------------------------------------------ certificate
def _certificate_inputs():
    rng = np.random.default_rng(2)
    return {"integers-0..15": cases.integer_no_fallback(), "integers-0..3-ties": cases.integer_ties(),
            "duplicates": cases.all_duplicates(),
            "fpfh-like-1000": (cases.fpfh_like(rng, (1, 1000)), cases.fpfh_like(rng, (1, 1000))),
            "unit-rows-1000": (cases.unit_rows(rng, (1, 1000)), cases.unit_rows(rng, (1, 1000)))}


CERTIFICATE = _certificate_inputs()


@pytest.mark.parametrize("K,S", [(2, 1), (16, 1), (20, 1), (20, 4), (32, 4)])
@pytest.mark.parametrize("name", list(CERTIFICATE))
def test_the_certificate_lists_the_rows_the_checker_predicts(dev, monkeypatch, name, K, S):
    """The kernel must list exactly the rows the numpy certificate (M = 16 keys per list, 2 S lists by t(j)) cannot
    cover -- an equality, not a cap -- and return knn_points_idx's bytes either way."""
    from pytorch3d_pointops_amd import _C, _C_feature_topk

    a, b = CERTIFICATE[name]
    predicted = int(tref.uncertified_rows(a, b, K=K, S=S).sum())
    f1, f2 = _dev(dev, a, b)
    l1 = torch.full((1,), a.shape[1], dtype=torch.int64, device=dev)
    l2 = torch.full((1,), b.shape[1], dtype=torch.int64, device=dev)
    _mode(monkeypatch, "unset")
    want_i, want_d = _C.knn_points_idx(f1, f2, l1, l2, 2, K)
    _mode(monkeypatch, f"S{S}")
    idx, dists, stats = _C_feature_topk.feature_topk(f1, f2, l1, l2, K)
    print(name, K, S, stats.cpu().numpy().tolist(), predicted)
    assert stats.cpu().numpy().tolist() == [[1, a.shape[1] - predicted, predicted, 2 * S]]
    _same_bytes(idx, want_i, name + " (idx)")
    _same_bytes(dists, want_d, name + " (dists)")


# ------------------------------------------------------------------------------------------------ operator
def _operator_inputs(D, N=2, P1=40, P2=50, seed=7):
    rng = np.random.default_rng(seed + D)
    return cases.unit_rows(rng, (N, P1), D), cases.unit_rows(rng, (N, P2), D), np.array([P1, 31]), np.array([P2, 19])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("D,K", [(33, 5), (33, 20), (128, 5), (128, 20)])
def test_knn_features_equals_knn_points(dev, monkeypatch, D, K, mode):
    from pytorch3d_pointops_amd import functions as f

    t = _dev(dev, *_operator_inputs(D))
    _mode(monkeypatch, "unset")
    want = f.knn_points(*t, K=K, return_nn=True)
    _mode(monkeypatch, mode)
    got, again = f.knn_features(*t, K=K, return_nn=True), f.knn_features(*t, K=K, return_nn=True)
    assert type(got) is type(want) and got._fields == ("dists", "idx", "knn")
    for key in got._fields:
        _same_bytes(getattr(got, key), getattr(want, key), f"D={D} K={K} [{mode}]: {key}")
        _same_bytes(getattr(again, key), getattr(got, key), f"D={D} K={K} [{mode}]: {key} of a second call")
    assert f.knn_features(t[0], t[1], K=K).knn is None


@pytest.mark.parametrize("mode", ["unset", "S1", "S4"])
def test_gradients(dev, monkeypatch, mode):
    """(N, P1, P2, D, K) = (2, 40, 50, 33, 5): the gradients of dists.sum() within 1e-5 of a float64 torch composition
    over the same indices (the project's bound for atomically accumulated gradients), and bit-equal to knn_points' own
    under torch.use_deterministic_algorithms(True)."""
    from pytorch3d_pointops_amd import functions as f

    a, b, l1, l2 = _dev(dev, *_operator_inputs(33))
    _mode(monkeypatch, mode)
    f1, f2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = f.knn_features(f1, f2, l1, l2, K=5)
    out.dists.sum().backward()
    x, y = a.double().requires_grad_(True), b.double().requires_grad_(True)
    valid = (torch.arange(40, device=dev)[None, :, None] < l1[:, None, None]) & \
        (torch.arange(5, device=dev)[None, None, :] < l2[:, None, None])
    nn = torch.gather(y[:, None].expand(-1, 40, -1, -1), 2, out.idx[..., None].expand(-1, -1, -1, 33))
    (((x[:, :, None] - nn) ** 2).sum(-1) * valid).sum().backward()
    for got, want, name in ((f1.grad, x.grad, "f1"), (f2.grad, y.grad, "f2")):
        err = float((got.double() - want).abs().max())
        print(mode, name, err)
        assert err <= 1e-5, f"grad {name} [{mode}]: {err}"
    torch.use_deterministic_algorithms(True)
    try:
        grads = []
        for op in (f.knn_features, f.knn_points):
            p, r = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
            op(p, r, l1, l2, K=5).dists.sum().backward()
            grads.append((p.grad, r.grad))
    finally:
        torch.use_deterministic_algorithms(False)
    _same_bytes(grads[0][0], grads[1][0], f"deterministic grad f1 [{mode}]")
    _same_bytes(grads[0][1], grads[1][1], f"deterministic grad f2 [{mode}]")


def test_a_hip_graph_replays_the_search(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd import graphs

    _mode(monkeypatch, "S4")  # (the screen, its device-side list and the always-enqueued fallback launch)
    a, b = cases.integer_ties()

    def call(x, y):
        r = f.knn_features(x, y, K=20)
        return r.dists, r.idx

    f1, f2 = _dev(dev, a, b)
    eager = call(f1, f2)
    step = graphs.capture(call, (f1.clone(), f2.clone()))
    for key, got, want in zip(("dists", "idx"), step(), eager):
        _same_bytes(got, want, f"replay: {key}")
    rng = np.random.default_rng(3)
    p1, p2 = (rng.integers(0, 5, a.shape).astype(np.float32) for _ in range(2))
    wi, wd = ref.knn(p1, p2, np.array([1000]), np.array([1000]), 20)
    for replay in range(2):
        got = step(*_dev(dev, p1, p2))
        _same_bytes(got[0], wd, f"other rows, replay {replay}: dists")
        _same_bytes(got[1], wi, f"other rows, replay {replay}: idx")


@pytest.mark.parametrize("mode", ["unset", "S1"])
def test_a_side_stream(dev, monkeypatch, mode):
    from pytorch3d_pointops_amd import functions as f

    arrays = _operator_inputs(33)
    wi, wd = ref.knn(*arrays, 16)
    _mode(monkeypatch, mode)
    t = _dev(dev, *arrays)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        r = f.knn_features(*t, K=16)
    side.synchronize()
    _same_bytes(r.idx, wi, f"side stream [{mode}]: idx")
    _same_bytes(r.dists, wd, f"side stream [{mode}]: dists")


@pytest.mark.parametrize("mode", ["unset", "S4"])
@pytest.mark.parametrize("fill", buffers.FILLS)
def test_buffer_contract(dev, monkeypatch, fill, mode):
    """Guards intact, inputs unchanged, the outputs fully written whatever the buffers held, a short and a null workspace
    rejected with untouched outputs, on either path."""
    from pytorch3d_pointops_amd import _C_feature_topk

    _mode(monkeypatch, mode)
    arrays = _operator_inputs(33)
    wi, wd = ref.knn(*arrays, 20)
    t = _dev(dev, *arrays)
    s = _dev(dev, *_operator_inputs(33, seed=8))
    with buffers.contract(monkeypatch, fill, short_workspace="short", prototypes=PROTOS) as k:
        k.sibling(lambda: _C_feature_topk.feature_topk(*s, 20))
        k.watch(f1=t[0], f2=t[1], lengths1=t[2], lengths2=t[3])
        idx, dists, _ = _C_feature_topk.feature_topk(*t, 20)
    k.assert_all_clear()
    assert {(n, how) for n, _, how in k.rejections} == {(ENTRY, "short"), (ENTRY, "null")}
    assert [b.kind for b in k.buffers] == ["out"] * 3 + ["workspace"] and k.inputs_checked >= 4
    _same_bytes(idx, wi, f"contract [{fill}, {mode}] (idx)")
    _same_bytes(dists, wd, f"contract [{fill}, {mode}] (dists)")
