"""The result rows of knn_points_idx under both row writers (knn_common.h, write_row): 16-byte stores when K % 4 == 0 and
both output buffers are 16-byte aligned, element stores otherwise -- and the batched prologue loads of the lane and
radius-2 kernels (knn_grid_search.h), whose clamped indices must list no run for an inactive lane or a row outside the
grid.  The grid family (version 3, radius-2 pass forced on, off, and left to the rule) against the CPU oracle AND the
brute-force family of the library, bit for bit, at the smallest shapes that reach every branch: a last chunk with
inactive lanes (P1 = 130), D = 1 / 2 / 3, both norms, K below, at and between the list capacities, ragged clouds (fewer
points than K: the zero tail; fewer queries than P1: the padded rows; no points at all), a clustered cloud whose
queries reach the box and the wave searches, and outputs that start 8 / 4 bytes into guarded buffers (tests/buffers.py):
the same bits as the aligned call, fills and guards around them untouched."""
import numpy as np
import pytest
import torch

import buffers
import cases
from conftest import bits

pytestmark = pytest.mark.gpu

N, P1, P2 = 3, 130, 257
KS = (1, 2, 3, 4, 8, 12, 16, 20, 32)
KNOBS = ("grid_quad=1", "grid_quad=0", "")
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _env(monkeypatch, knob):
    if knob:
        monkeypatch.setenv("POINTOPS_DEBUG", knob)
    else:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)


def _small(D, K):
    """Three clouds: full; ragged (len1 < P1, len2 < K: K - 3 points, or K - 1 for K <= 4, so that the zero tail starts
    inside a 16-byte piece); no points at all."""
    def make():
        p1, p2 = cases.cloud(4100 + D, (N, P1, D)), cases.cloud(4200 + D, (N, P2, D))
        return p1, p2
    p1, p2 = _cached(("small", D), make)
    l1 = np.array([P1, 70, P1], np.int64)
    l2 = np.array([P2, K - 1 if K <= 4 else K - 3, 0], np.int64)
    return p1, p2, l1, l2


def _clustered():
    """Two clouds of 2000 points, half of cloud 0 inside a cube of edge 1e-3 (one over-full cell: its queries leave the
    lane search for the box search); 300 queries, half of them inside the cluster, twenty far outside the points' box
    (no cube of the lane or the radius-2 pass certifies them: the wave search does), cloud 1 ragged with len2 = 3."""
    def make():
        p1, p2 = cases.cloud(4301, (2, 300, 3)), cases.cloud(4302, (2, 2000, 3))
        p2[0, :1000] = p2[0, :1000] * np.float32(1e-3) + np.float32(0.5)
        p1[0, :150] = p1[0, :150] * np.float32(1e-3) + np.float32(0.5)
        p1[0, 150:170] += np.float32(4.0)
        return p1, p2, np.array([300, 211], np.int64), np.array([2000, 3], np.int64)
    return _cached("clustered", make)


def _gpu(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _same(got, want, what):
    gi, gd = got
    wi, wd = want
    gi, gd = (x.cpu().numpy() if torch.is_tensor(x) else x for x in (gi, gd))
    wi, wd = (x.cpu().numpy() if torch.is_tensor(x) else x for x in (wi, wd))
    assert np.array_equal(gi, wi), what
    assert np.array_equal(bits(gd), bits(wd)), what


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_rows_of_every_family_match_oracle_and_brute_force(dev, oracle, monkeypatch, D, norm):
    from pytorch3d_pointops_amd import _C

    for K in KS:
        p1, p2, l1, l2 = _small(D, K)
        assert l2[1] < K and l1[1] < P1 and l2[2] == 0
        want = oracle.knn_points_idx(p1, p2, l1, l2, norm, K)
        ta, tb, t1, t2 = _gpu(dev, (p1, p2, l1, l2))
        _env(monkeypatch, "")
        brute = _C.knn_points_idx(ta, tb, t1, t2, norm, K, 0)
        _same(brute, want, dict(D=D, norm=norm, K=K, version=0))
        assert _C.knn_check_version(3, D, K)
        for knob in KNOBS:
            _env(monkeypatch, knob)
            for version in (3,) if knob else (3, 2, -1):  # (2: the register scan, -1: the rule's choice -- the other writers)
                got = _C.knn_points_idx(ta, tb, t1, t2, norm, K, version)
                what = dict(D=D, norm=norm, K=K, knob=knob, version=version)
                _same(got, want, what)
                _same(got, brute, what)


@pytest.mark.parametrize("K", [3, 16, 20])
def test_rows_of_the_box_and_wave_searches(dev, oracle, monkeypatch, K):
    """K = 16: K = KC; K = 20: 16-byte stores with K < KC = 32; K = 3: element stores.  The statistics (columns of
    knn_grid_stats: 5 / 6 uncertified after the lane / the radius-2 + box passes, 8 deferred to the box search) confirm
    that cloud 0 really sent queries to the box search and to the wave search."""
    from pytorch3d_pointops_amd import _C

    p1, p2, l1, l2 = _clustered()
    ta, tb, t1, t2 = _gpu(dev, (p1, p2, l1, l2))
    for norm in (1, 2):
        want = _cached(("clustered want", K, norm), lambda: oracle.knn_points_idx(p1, p2, l1, l2, norm, K))
        _env(monkeypatch, "")
        brute = _C.knn_points_idx(ta, tb, t1, t2, norm, K, 0)
        _same(brute, want, dict(K=K, norm=norm, version=0))
        for knob in KNOBS:
            _env(monkeypatch, knob)
            what = dict(K=K, norm=norm, knob=knob)
            _same(_C.knn_points_idx(ta, tb, t1, t2, norm, K, 3), want, what)
            gi, gd, st = _C.knn_grid_stats(ta, tb, t1, t2, norm, K)
            _same((gi, gd), want, what)
            st = st.cpu().numpy()
            assert st[0, 4] == 1 and st[0, 8] > 0, (what, st)  # searched through its grid; queries in the box search
            if knob:
                assert st[0, 6 if knob == "grid_quad=1" else 5] >= 20, (what, st)  # the wave search's list: the far queries


# --------------------------------------------------------------------------------------------- misaligned outputs
def _shifted_outputs(monkeypatch, c, shift):
    """Route `_C._out` through the contract `c` with `shift[dtype]` extra elements in front of and behind every output:
    the call then sees a pointer shift * itemsize bytes into the guarded payload.  Returns the list of (flat payload,
    shift, elements) handed out."""
    from pytorch3d_pointops_amd import _C

    handed = []

    def out(shape, dtype=None, device=None):
        s = shift[dtype]
        n = int(np.prod(shape))
        flat = c.out((n + 2 * s,), dtype=dtype, device=device)
        handed.append((flat, s, n))
        return flat[s:s + n].view(tuple(shape))

    monkeypatch.setattr(_C, "_out", out)
    return handed


@pytest.mark.parametrize("shift_idx,shift_dist", [(1, 1), (1, 0), (0, 1), (0, 2)],
                         ids=["idx+8_dists+4", "idx+8", "dists+4", "dists+8"])
def test_misaligned_outputs_take_the_element_stores(dev, monkeypatch, shift_idx, shift_dist):
    """Through the C ABI with `idxs` 8 bytes and `dists` 4 (or 8) bytes into larger guarded buffers, for the K that would
    otherwise take the 16-byte stores, in every family: the same bits as the aligned call (itself made into guarded
    buffers: a 16-byte store that overshoots the last row shows in the guard behind it), the elements in front of and
    behind the shifted outputs still hold the fill, all guards intact."""
    from pytorch3d_pointops_amd import _C

    assert not _C.grid_cache_enabled()
    D, norm = 3, 2
    for K in (4, 16, 20, 32):
        p1, p2, l1, l2 = _small(D, K)
        ta, tb, t1, t2 = _gpu(dev, (p1, p2, l1, l2))
        for knob, version in (("grid_quad=1", 3), ("grid_quad=0", 3), ("", 3), ("", 2), ("", 0)):
            _env(monkeypatch, knob)
            what = dict(K=K, knob=knob, version=version, shift=(shift_idx, shift_dist))

            def aligned():
                with buffers.contract(monkeypatch, "ones") as c:
                    i, d = _C.knn_points_idx(ta, tb, t1, t2, norm, K, version)
                    assert i.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
                    i, d = i.cpu().numpy(), d.cpu().numpy()
                c.assert_guards_intact()
                return i, d
            want = _cached(("aligned", K, knob, version), aligned)

            with buffers.contract(monkeypatch, "ones") as c:
                handed = _shifted_outputs(monkeypatch, c, {torch.int64: shift_idx, torch.float32: shift_dist})
                i, d = _C.knn_points_idx(ta, tb, t1, t2, norm, K, version)
                assert i.data_ptr() % 16 == 8 * shift_idx and d.data_ptr() % 16 == 4 * shift_dist, what
                got = i.cpu().numpy(), d.cpu().numpy()
            _same(got, want, what)
            c.assert_guards_intact()
            assert len(handed) == 2, what
            for flat, s, n in handed:
                raw = flat.view(torch.uint8).cpu().numpy()
                item = flat.element_size()
                assert (raw[:s * item] == 0xFF).all() and (raw[(s + n) * item:] == 0xFF).all(), \
                    (what, str(flat.dtype), "the fill around a shifted output was written")
