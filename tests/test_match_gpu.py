"""match_features on the device (csrc/feature_match.hip, _C_match.py, functions/match.py):
    search       _C_match.feature_knn equals _C.knn_points_idx byte for byte -- and tests/match_ref.py on finite cases --
                 for K in {1, 2} with POINTOPS_DEBUG=match_screen unset, 0 (the exact search) and 1 (the screen at every
                 D <= 128), on every case of tests/match_cases.py
    certificate  the rows the kernel sends to its exact fallback are the rows the checker's certificate cannot cover:
                 none on small integers with distinct distances, the tied rows on tied integers, every row of a cloud
                 of duplicates, none on descriptor-like rows
    MFMA stage   pointops_feature_screen_values on quantised rows equals a numpy float32 loop bit for bit: the k order
                 of the chain and the lane maps of both operands and of the accumulator
    operator     match_features equals the checker field by field under every filter, equals mutual_nearest_neighbors
                 at its defaults, twice, from a HIP graph, on a side stream, on 65 540 clouds, under the buffer contract
The knob is read at call time, so every path runs in this process."""
import numpy as np
import pytest
import torch

import buffers
import match_cases as cases
import match_ref as ref
from test_boundary_cpu import declared_prototypes

pytestmark = pytest.mark.gpu

PROTOS = declared_prototypes()
ENTRY = "pointops_feature_knn"
CASES = cases.build_cases()
MODES = (None, 0, 1)
SCREEN_MAX_D = 128
FILTERS = {"none": dict(mutual=False), "mutual": dict(), "ratio": dict(mutual=False, ratio=0.8),
           "cap": dict(mutual=False, max_distance=30.0), "all": dict(ratio=0.8, max_distance=30.0)}


def _mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    else:
        monkeypatch.setenv("POINTOPS_DEBUG", f"match_screen={mode}")


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _same_bytes(got, want, what):
    a = got.detach().cpu().numpy() if torch.is_tensor(got) else np.ascontiguousarray(got)
    b = want.detach().cpu().numpy() if torch.is_tensor(want) else np.ascontiguousarray(want)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype}{a.shape}, want {b.dtype}{b.shape}"
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))
        at = tuple(bad[0][:-1])
        raise AssertionError(f"{what}: differs at {len(bad)} bytes, first at {at}: got {a[at]!r}, want {b[at]!r}")


def _live_rows(c):
    l1 = np.clip(c.lengths1, 0, c.f1.shape[1])
    return np.where(np.clip(c.lengths2, 0, c.f2.shape[1]) > 0, l1, 0)


def _case_tensors(dev, c):
    f1, f2, l1, l2 = _dev(dev, c.f1, c.f2, c.lengths1, c.lengths2)
    return f1, (f1 if c.same else f2), l1, (l1 if c.same else l2)


# ------------------------------------------------------------------------------------------------ search
@pytest.mark.parametrize("name", list(CASES))
def test_search_equals_knn_points_on_every_path(dev, monkeypatch, name):
    from pytorch3d_pointops_amd import _C, _C_match

    c = CASES[name]
    t = _case_tensors(dev, c)
    N, P1, D = c.f1.shape
    for K in (1, 2):
        _mode(monkeypatch, None)
        want_i, want_d = _C.knn_points_idx(*t, 2, K)
        if c.finite:
            ri, rd = ref.knn(c.f1, c.f2, c.lengths1, c.lengths2, K)
            _same_bytes(want_i, ri, f"{name} K={K}: knn_points_idx against the checker (idx)")
            _same_bytes(want_d, rd, f"{name} K={K}: knn_points_idx against the checker (dists)")
        for mode in MODES:
            _mode(monkeypatch, mode)
            idx, dists, stats = _C_match.feature_knn(*t, K)
            what = f"{name} K={K} match_screen={mode}"
            _same_bytes(idx, want_i, what + " (idx)")
            _same_bytes(dists, want_d, what + " (dists)")
            stats = stats.cpu().numpy()
            assert stats.shape == (N, 4) and stats.dtype == np.int32 and not stats[:, 3].any(), what
            if mode != 1 or D > SCREEN_MAX_D or c.f2.shape[1] == 0 or P1 == 0:  # (the default is the exact search)
                assert not stats.any(), what + ": the exact search reports no screen"
            elif mode == 1:
                assert (stats[:, 0] == 1).all() and (stats[:, 1] >= 0).all(), what
                assert np.array_equal(stats[:, 1] + stats[:, 2], _live_rows(c)), what + ": certified + listed = live rows"
                if name == "huge":  # (every norm is 2^126: n1 + n2max is above the bound's range)
                    assert not stats[:, 1].any(), what + ": a row out of the bound's range was certified"
                if K == 2:  # the listed rows are the checker's, cloud by cloud
                    with np.errstate(all="ignore"):
                        predicted = ref.uncertified_rows(c.f1, c.f2, c.lengths1, c.lengths2, K=2).sum(1)
                    assert np.array_equal(stats[:, 2], predicted), what + f": listed {stats[:, 2]}, predicted {predicted}"


def test_search_rejects_what_the_header_says(dev, monkeypatch):
    from pytorch3d_pointops_amd import _C_match

    _mode(monkeypatch, None)
    f1, f2, l1, l2 = _dev(dev, np.zeros((1, 4, 33), np.float32), np.zeros((1, 5, 33), np.float32), np.array([4]), np.array([5]))
    for K in (0, 3):
        with pytest.raises(RuntimeError, match="1 <= K <= 2"):
            _C_match.feature_knn(f1, f2, l1, l2, K)
    with pytest.raises(RuntimeError, match="lengths"):
        _C_match.feature_knn(f1, f2, None, l2, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_match.feature_knn(f1.cpu(), f2.cpu(), l1.cpu(), l2.cpu(), 1)
    with pytest.raises(RuntimeError, match="1 <= P1, P2 <= 1024"):
        _C_match.feature_screen_values(torch.zeros((1, 1025, 3), device=dev), f2[..., :3].contiguous(),
                                       torch.tensor([1025], device=dev), l2)


# ------------------------------------------------------------------------------------------------ certificate
def _certificate_inputs():
    rng = np.random.default_rng(1)
    return {
        "integers-0..15": cases.integer_no_fallback() + (0,),
        "integers-0..3-ties": cases.integer_ties() + (49,),
        "duplicates": cases.all_duplicates() + (100,),
        "fpfh-like-3000": (cases.fpfh_like(rng, (1, 3000)), cases.fpfh_like(rng, (1, 3000)), 0),
        "unit-rows-1000": (cases.unit_rows(rng, (1, 1000)), cases.unit_rows(rng, (1, 1000)), 0),
    }


CERTIFICATE = _certificate_inputs()


@pytest.mark.parametrize("name", list(CERTIFICATE))
def test_the_certificate_lists_the_rows_the_checker_predicts(dev, monkeypatch, name):
    """`expected` is the checker's count (numpy, K = 2, M = 8 keys per lane: tests/test_match_cpu.py holds the
    integer ones; descriptor-like rows: 0 of 3000 and 0 of 1000); the kernel must list exactly those rows -- an
    equality, not a cap -- and return knn_points_idx's bytes either way."""
    from pytorch3d_pointops_amd import _C, _C_match

    a, b, expected = CERTIFICATE[name]
    predicted = ref.uncertified_rows(a, b, K=2)
    assert int(predicted.sum()) == expected
    f1, f2 = _dev(dev, a, b)
    l1 = torch.full((1,), a.shape[1], dtype=torch.int64, device=dev)
    l2 = torch.full((1,), b.shape[1], dtype=torch.int64, device=dev)
    _mode(monkeypatch, None)
    want_i, want_d = _C.knn_points_idx(f1, f2, l1, l2, 2, 2)
    _mode(monkeypatch, 1)
    idx, dists, stats = _C_match.feature_knn(f1, f2, l1, l2, 2)
    assert stats.cpu().numpy().tolist() == [[1, a.shape[1] - expected, expected, 0]]
    _same_bytes(idx, want_i, name + " (idx)")
    _same_bytes(dists, want_d, name + " (dists)")


# ------------------------------------------------------------------------------------------------ MFMA stage
@pytest.mark.parametrize("D", [2, 33, 128])
def test_the_mfma_stage_is_the_fmaf_chain(dev, monkeypatch, D):
    """Rows of multiples of 2^-8 in [-4, 4): every product is exact in float32, so `acc = acc + a_k * b_k` in float32
    IS the fmaf chain, and n1, n2, s and E of the kernel must equal numpy bit for bit.  The sums are not exact (up to
    27 bits), so a different k order, a swapped operand map or a transposed accumulator shows."""
    from pytorch3d_pointops_amd import _C_match

    _mode(monkeypatch, None)
    rng = np.random.default_rng(D)
    P1, P2 = 257, 203
    a, b = cases.quantised(rng, (2, P1, D)), cases.quantised(rng, (2, P2, D))
    l1, l2 = np.array([P1, 100]), np.array([P2, 77])
    s, n1, n2, n2max, E = (t.cpu().numpy() for t in _C_match.feature_screen_values(*_dev(dev, a, b, l1, l2)))
    w1, w2 = np.zeros((2, P1), np.float32), np.zeros((2, P2), np.float32)
    g = np.zeros((2, P1, P2), np.float32)
    for k in range(D):
        w1 = w1 + a[..., k] * a[..., k]
        w2 = w2 + b[..., k] * b[..., k]
        g = g + a[:, :, None, k] * b[:, None, :, k]
    assert g.dtype == np.float32
    ws = (w1[:, :, None] + w2[:, None, :]) - (g + g)
    rows, cols = np.arange(P1)[None, :, None] < l1[:, None, None], np.arange(P2)[None, None, :] < l2[:, None, None]
    ws = np.where(rows & cols, ws, np.float32(0))
    wmax = np.array([w2[n, :l2[n]].max() for n in range(2)], np.float32)
    wE = np.where(rows[..., 0], np.stack([ref.screen_bound(D, w1[n], wmax[n]) for n in range(2)]), np.float32(0))
    _same_bytes(n1, w1, f"D={D}: n1")
    _same_bytes(n2, w2, f"D={D}: n2")
    _same_bytes(n2max, wmax, f"D={D}: n2max")
    _same_bytes(s, ws, f"D={D}: s")
    _same_bytes(E, wE.astype(np.float32), f"D={D}: E")
    assert len(np.unique(s[0])) > 1000 and not np.array_equal(s[0, :203], s[0, :203].T)  # (nothing symmetric hides a swap)


# ------------------------------------------------------------------------------------------------ operator
def _operator_inputs():
    c = CASES["ragged"]
    f1, f2, truth = cases.replaced_scene()
    b1, b2, bl1, bl2 = cases.ratio_boundary()
    return {"ragged": (c.f1, c.f2, c.lengths1, c.lengths2), "scene": (f1, f2, None, None), "boundary": (b1, b2, bl1, bl2)}


OPERATOR = _operator_inputs()


def _assert_fields(got, want, what):
    assert type(got).__name__ == "FeatureMatches" and got._fields == ref.KEYS
    for key in ref.KEYS:
        _same_bytes(getattr(got, key), want[key], f"{what}: {key}")


@pytest.mark.parametrize("filters", list(FILTERS))
@pytest.mark.parametrize("name", list(OPERATOR))
def test_match_features_equals_the_checker(dev, monkeypatch, name, filters):
    from pytorch3d_pointops_amd import functions as f

    _mode(monkeypatch, None)
    arrays, kw = OPERATOR[name], FILTERS[filters]
    if name == "boundary" and "ratio" in kw:
        kw = dict(kw, ratio=0.5, max_distance=None)
    want = ref.match_features(*arrays, **kw)
    t = _dev(dev, *arrays)
    _assert_fields(f.match_features(*t, **kw), want, f"{name} [{filters}]")
    _mode(monkeypatch, 1)
    _assert_fields(f.match_features(*t, **kw), want, f"{name} [{filters}, match_screen=1]")


def test_defaults_equal_mutual_nearest_neighbors_and_a_second_call(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    for mode in MODES:
        _mode(monkeypatch, mode)
        for name in ("ragged", "scene"):
            t = _dev(dev, *OPERATOR[name])
            first, again = f.match_features(*t), f.match_features(*t)
            _same_bytes(first.corr, f.mutual_nearest_neighbors(*t), f"{name}: corr at the defaults, match_screen={mode}")
            for key in ref.KEYS:
                _same_bytes(getattr(again, key), getattr(first, key), f"{name}: {key} of a second call")
    for N, P1, P2 in ((0, 5, 5), (0, 0, 0), (3, 0, 6), (3, 6, 0)):
        m = f.match_features(torch.zeros((N, P1, 33), device=dev), torch.zeros((N, P2, 33), device=dev), ratio=0.9)
        assert m.corr.shape == (N, P1) and m.dists.shape == (N, P1) and m.second.shape == (N, P1)
        assert m.num_matches.shape == (N,) and not m.num_matches.any() and (m.corr == -1).all() and not m.second.any()


def test_the_ratio_test_removes_wrong_matches_the_mutual_check_keeps(dev, monkeypatch):
    """1200 descriptor rows against a permuted, noisy copy whose first 360 rows describe something else.  From the
    checker: the mutual check alone keeps 883 matches, 43 of them wrong; with ratio = 0.8, 841 and 1; with the cap at
    30 as well, 840 and 0 -- every one of the 840 rows whose partner survived, and nothing else."""
    from pytorch3d_pointops_amd import functions as f

    _mode(monkeypatch, None)
    f1, f2, truth = cases.replaced_scene()
    t = _dev(dev, f1, f2)
    counts = {}
    for key, kw in (("mutual", {}), ("ratio", dict(ratio=0.8)), ("all", dict(ratio=0.8, max_distance=30.0))):
        m = f.match_features(*t, **kw)
        corr = m.corr[0].cpu().numpy()
        found = corr >= 0
        counts[key] = (int(m.num_matches[0]), int((found & (corr != truth)).sum()))
    print(counts)
    assert counts == {"mutual": (883, 43), "ratio": (841, 1), "all": (840, 0)}
    assert np.array_equal(np.nonzero(corr >= 0)[0], np.nonzero(truth >= 0)[0])


def test_a_hip_graph_replays_the_match(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f
    from pytorch3d_pointops_amd import graphs

    _mode(monkeypatch, 1)  # (the screen, its device-side list and the always-enqueued fallback launch)
    a, b = cases.integer_ties()
    kw = dict(ratio=0.9, max_distance=3.0)

    def call(x, y):
        return tuple(f.match_features(x, y, **kw))

    f1, f2 = _dev(dev, a, b)
    eager = call(f1, f2)
    step = graphs.capture(call, (f1.clone(), f2.clone()))
    for key, got, want in zip(ref.KEYS, step(), eager):
        _same_bytes(got, want, f"replay: {key}")
    c = CASES["N1"]
    p1, p2 = np.zeros_like(a), np.zeros_like(b)
    p1[:, :300, :5], p2[:, :257, :5] = c.f1[..., :5], c.f2[..., :5]
    want2 = ref.match_features(p1, p2, **kw)
    for replay in range(2):
        got = step(*_dev(dev, p1, p2))
        for key, g in zip(ref.KEYS, got):
            _same_bytes(g, want2[key], f"other rows, replay {replay}: {key}")


def test_a_side_stream(dev, monkeypatch):
    from pytorch3d_pointops_amd import functions as f

    arrays = OPERATOR["ragged"]
    want = ref.match_features(*arrays, **FILTERS["all"])
    for mode in (None, 1):
        _mode(monkeypatch, mode)
        t = _dev(dev, *arrays)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            m = f.match_features(*t, **FILTERS["all"])
        side.synchronize()
        _assert_fields(m, want, f"side stream, match_screen={mode}")


@pytest.mark.parametrize("mode", [None, 1])
@pytest.mark.parametrize("fill", buffers.FILLS)
def test_buffer_contract(dev, monkeypatch, fill, mode):
    """Guards intact, inputs unchanged, the outputs fully written whatever the buffers held, a short and a null workspace
    rejected with untouched outputs -- for both searches of a match_features call, on either path."""
    from pytorch3d_pointops_amd import functions as f

    _mode(monkeypatch, mode)
    arrays = OPERATOR["ragged"]
    want = ref.match_features(*arrays, **FILTERS["all"])
    t = _dev(dev, *arrays)
    rng = np.random.default_rng(4)
    s1, s2 = _dev(dev, cases.fpfh_like(rng, arrays[0].shape[:2]), cases.fpfh_like(rng, arrays[1].shape[:2]))
    with buffers.contract(monkeypatch, fill, short_workspace="short", prototypes=PROTOS) as k:
        k.sibling(lambda: f.match_features(s1, s2, None, None, **FILTERS["all"]))
        k.watch(f1=t[0], f2=t[1], lengths1=t[2], lengths2=t[3])
        m = f.match_features(*t, **FILTERS["all"])
    k.assert_all_clear()
    assert {(n, how) for n, _, how in k.rejections} == {(ENTRY, "short"), (ENTRY, "null")}
    assert [b.kind for b in k.buffers] == (["out"] * 3 + ["workspace"]) * 2 and k.inputs_checked >= 8
    _assert_fields(m, want, f"contract [{fill}, match_screen={mode}]")


def test_a_batch_of_65540_clouds(dev, monkeypatch):
    from pytorch3d_pointops_amd import _C_match
    from pytorch3d_pointops_amd import functions as f

    N, P, D = 65540, 2, 33
    rng = np.random.default_rng(77)
    a, b = cases.fpfh_like(rng, (N, P)), cases.fpfh_like(rng, (N, P))
    l1, l2 = (rng.integers(0, P + 1, N).astype(np.int64) for _ in range(2))
    l1[[0, 65534, 65535, 65536, N - 1]] = P
    l2[[0, 65534, 65535, 65536, N - 1]] = P
    acc = np.zeros((N, P, P), np.float32)
    for k in range(D):
        diff = a[:, :, None, k] - b[:, None, :, k]
        acc = acc + diff * diff
    acc = np.where(np.arange(P)[None, None, :] < l2[:, None, None], acc, np.float32(np.inf))
    order = np.argsort(acc, axis=2, kind="stable")
    valid = (np.arange(P)[None, :, None] < l1[:, None, None]) & (np.arange(P)[None, None, :] < l2[:, None, None])
    want_i = np.where(valid, order, 0).astype(np.int64)
    want_d = np.where(valid, np.take_along_axis(acc, order, axis=2), np.float32(0)).astype(np.float32)
    t = _dev(dev, a, b, l1, l2)
    for mode in (None, 1):
        _mode(monkeypatch, mode)
        with buffers.contract(monkeypatch, "ones", short_workspace="short", prototypes=PROTOS) as k:
            k.watch(f1=t[0], f2=t[1])
            idx, dists, stats = _C_match.feature_knn(*t, 2)
        k.assert_all_clear()
        _same_bytes(idx, want_i, f"65540 clouds, match_screen={mode} (idx)")
        _same_bytes(dists, want_d, f"65540 clouds, match_screen={mode} (dists)")
        stats = stats.cpu().numpy()
        assert (stats[:, 0] == (1 if mode == 1 else 0)).all() and not stats[:, 3].any()
        if mode == 1:
            assert np.array_equal(stats[:, 1], np.where(l2 > 0, l1, 0)) and not stats[:, 2].any()  # (<= M targets: certified)
    m = f.match_features(*t, mutual=False)
    _same_bytes(m.corr, np.where(valid[..., 0], want_i[..., 0], -1), "65540 clouds: corr")
    assert int(m.num_matches.sum()) == int(valid[..., 0].sum())
