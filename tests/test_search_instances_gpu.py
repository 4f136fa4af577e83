"""Every template instance of the search kernels at its bucket edges, bit-equal to the oracle: `idx` and the uint32 view
of `dists`, every row and slot, padding included, no tolerance.

The matrix -- value lists, K lists, batches -- is tests/search_instance_cases.py; tests/test_search_instances_cpu.py
certifies, without a device, that its lists are the source's and that every batch holds the ties and lengths it is there
for.  Here every KNN call first asks the dispatch (pointops_knn_plan) for the family and the slice count of its shape and
asserts that they are the ones the case is there for, so a later change of a crossover cannot quietly empty the matrix;
the ball query and the grid assert their path from the workspace size, the grid diagnostics and the forcing knob.
"""
import numpy as np
import pytest
import torch

import search_instance_cases as sic
from conftest import bits

pytestmark = pytest.mark.gpu


def G(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the cached inputs are read-only)


def knob(monkeypatch, value):
    monkeypatch.setenv("POINTOPS_DEBUG", value) if value else monkeypatch.delenv("POINTOPS_DEBUG", raising=False)


def device_batch(b, dev, self_query=False):
    if self_query:
        p, lengths = G(b["p2"], dev), G(b["l2"], dev)
        return [p, p, lengths, lengths]  # the same tensors: the entry recognises the self-query by pointer equality
    return [G(b[k], dev) for k in ("p1", "p2", "l1", "l2")]


def assert_equal(got, want, what):
    """`got` (device or numpy idx, dists) equals `want` bit for bit; the message names the first differing
    (cloud, row, slot)."""
    gi, gd = (a.cpu().numpy() if torch.is_tensor(a) else a for a in got)
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, f"{what}: shapes {gi.shape} {gd.shape}, want {wi.shape}"
    bad = (gi != wi) | (bits(gd) != bits(wd))
    if bad.any():
        n, r, s = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} slots differ, first at (cloud, row, slot) = ({n}, {r}, {s}): got idx "
            f"{gi[n, r, s]} dist {gd[n, r, s]!r} (bits {bits(gd)[n, r, s]:#x}), want idx {wi[n, r, s]} dist "
            f"{wd[n, r, s]!r} (bits {bits(wd)[n, r, s]:#x}); row got {gi[n, r].tolist()} want {wi[n, r].tolist()}")


def label(family, D, K, KC, norm, knobs, extra=""):
    return f"{family} D={D} K={K} KC={KC} L{norm} POINTOPS_DEBUG='{knobs}'{extra}"


def planned(monkeypatch, family, b, D, K, version=None, knobs=None):
    """Set the family's knobs and assert that the dispatch takes the family and the slices the case is there for."""
    from pytorch3d_pointops_amd import _C

    _, fknobs, fversion, want, slices, _, _ = sic.KNN[family]
    knobs = fknobs if knobs is None else knobs
    version = fversion if version is None else version
    knob(monkeypatch, knobs)
    N, P1, _ = b["p1"].shape
    got, S = _C.knn_plan(N, P1, b["p2"].shape[1], D, K, version)
    assert got == want and (S == 1 if slices == 1 else 4 <= S <= 8), \
        f"{label(family, D, K, b['KC'], '-', knobs)}: the plan is ({got}, {S} slices), the case is there for {want}"
    wg256 = N * -(-P1 // 256) >= 2048  # the launch's own choice of the workgroup size
    assert wg256 == (sic.KNN[family][0] == "many")
    return version


def run_family(dev, oracle, monkeypatch, family, D, norm, both_versions_at=None):
    from pytorch3d_pointops_amd import _C

    geometry, knobs, _, _, _, _, caps = sic.KNN[family]
    for K in sic.knn_ks(family, D, norm):
        b = sic.batch(geometry, D, K, caps)
        version = planned(monkeypatch, family, b, D, K)
        t = device_batch(b, dev)
        got = _C.knn_points_idx(*t, norm, K, version)
        want = oracle.knn_points_idx(b["p1"], b["p2"], b["l1"], b["l2"], norm, K)
        assert_equal(got, want, label(family, D, K, b["KC"], norm, knobs))
        if K == both_versions_at:  # versions 1 and 2 are one family
            planned(monkeypatch, family, b, D, K, version=1)
            assert_equal(_C.knn_points_idx(*t, norm, K, 1), want, label(family, D, K, b["KC"], norm, knobs, " version 1"))


# ------------------------------------------------------------------ register lists, D = 1..8
@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.SCAN_D)
def test_knn_reg_64_lanes(dev, oracle, monkeypatch, D, norm):
    """knn_reg_kernel<D, KC, NORM>, 64-lane workgroups, the whole cloud in one slice; versions 1 and 2 at one K."""
    run_family(dev, oracle, monkeypatch, "scan64", D, norm, both_versions_at=sic.ROTATING_K[D % len(sic.ROTATING_K)])


@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.SCAN_D)
def test_knn_reg_sliced_and_merged(dev, oracle, monkeypatch, D, norm):
    """S = 4..8 slices of p2 (more with D), partial lists of K out of KC merged by knn_merge_kernel<KC>; the short
    clouds leave slices empty or with fewer than K candidates."""
    run_family(dev, oracle, monkeypatch, "sliced", D, norm)


@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.SCAN_D)
def test_knn_reg_256_lanes(dev, oracle, monkeypatch, D, norm):
    """The same kernel with 256-lane workgroups: 1024 clouds of 257 queries, one K per (D, norm)."""
    run_family(dev, oracle, monkeypatch, "scan256", D, norm)


@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.SCAN_D)
def test_knn_small_one_query_per_wave(dev, oracle, monkeypatch, D, norm):
    """knn_small_kernel<D, KC, NORM, 1>."""
    run_family(dev, oracle, monkeypatch, "small_q1", D, norm)


@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.SCAN_D)
def test_knn_small_four_queries_per_wave(dev, oracle, monkeypatch, D, norm):
    """knn_small_kernel<D, KC, NORM, 4>: lists of one or two slots (longer lists have no such instance)."""
    run_family(dev, oracle, monkeypatch, "small_q2", D, norm)


@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.SCAN_D)
def test_knn_small_refreshed_gates(dev, oracle, monkeypatch, D, norm):
    """Clouds of more than max(512, 128 K) candidates: the wave-uniform gate, the K-th distinct list head out of lists
    of KC slots, is refreshed at least once, and most later candidates of the lattice tie with it."""
    run_family(dev, oracle, monkeypatch, "small_gated_q1", D, norm)
    run_family(dev, oracle, monkeypatch, "small_gated_q2", D, norm)


# ------------------------------------------------------------------ knn_wide (version 0)
@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.WIDE_D)
@pytest.mark.parametrize("family", ["wide64", "wide64_sliced", "wide256"])
def test_knn_wide_register_lists(dev, oracle, monkeypatch, family, D, norm):
    """knn_wide_kernel<KC, NORM, WG> for every KC and WG, the 64-lane ones also with S > 1 and the merge."""
    run_family(dev, oracle, monkeypatch, family, D, norm)


@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.WIDE_D)
@pytest.mark.parametrize("family", ["wide_long", "wide_lds"])
def test_knn_wide_long_and_lds_lists(dev, oracle, monkeypatch, family, D, norm):
    """K = 33, 48, 64: 64-slot register lists; K = 65, 100: lists in LDS.  knn_generic=1 -- the plan then says generic --
    gives the same bytes."""
    from pytorch3d_pointops_amd import _C

    run_family(dev, oracle, monkeypatch, family, D, norm)
    geometry, _, _, _, _, _, caps = sic.KNN[family]
    for K in sic.knn_ks(family, D, norm):
        b = sic.batch(geometry, D, K, caps)
        knob(monkeypatch, "knn_generic=1")
        assert _C.knn_plan(*b["p1"].shape[:2], b["p2"].shape[1], D, K, 0) == ("generic", 1)
        got = _C.knn_points_idx(*device_batch(b, dev), norm, K, 0)
        want = oracle.knn_points_idx(b["p1"], b["p2"], b["l1"], b["l2"], norm, K)
        assert_equal(got, want, label("generic", D, K, K, norm, "knn_generic=1"))


@pytest.mark.parametrize("which", range(6))
def test_knn_wide_lds_budget_edges(dev, oracle, monkeypatch, which):
    """The last shape inside each LDS budget of knn_wide_supported (the wide kernel with all the LDS it may ask for) and
    the first outside it (the generic kernel), derived from the constants of knn_wide.hip."""
    from pytorch3d_pointops_amd import _C

    D, K, inside = sic.wide_budget_edges()[which]
    b = sic.batch(*sic.edge_batch_of(K)[:1], D, K, sic.edge_batch_of(K)[1])
    for norm in sic.NORMS:
        knob(monkeypatch, "")
        family = _C.knn_plan(*b["p1"].shape[:2], b["p2"].shape[1], D, K, 0)[0]
        assert family == ("wide" if inside else "generic"), (D, K, family)
        got = _C.knn_points_idx(*device_batch(b, dev), norm, K, 0)
        want = oracle.knn_points_idx(b["p1"], b["p2"], b["l1"], b["l2"], norm, K)
        assert_equal(got, want, label(family + " at the LDS budget", D, K, b["KC"], norm, ""))


@pytest.mark.parametrize("version,D,K,want", sic.FALL_THROUGH)
def test_knn_version_falls_through(dev, oracle, monkeypatch, version, D, K, want):
    """A version that does not take the shape: the plan reports the automatic choice, the result is the oracle's."""
    from pytorch3d_pointops_amd import _C

    knob(monkeypatch, "")
    b = sic.batch("few", D, K, ())
    shape = (*b["p1"].shape[:2], b["p2"].shape[1], D, K)
    assert not _C.knn_check_version(version, D, K)
    assert _C.knn_plan(*shape, version) == _C.knn_plan(*shape, -1) and _C.knn_plan(*shape, version)[0] == want
    for norm in sic.NORMS:
        got = _C.knn_points_idx(*device_batch(b, dev), norm, K, version)
        want_rows = oracle.knn_points_idx(b["p1"], b["p2"], b["l1"], b["l2"], norm, K)
        assert_equal(got, want_rows, label(f"version {version} -> {want}", D, K, K, norm, ""))


# ------------------------------------------------------------------ the grid family (version 3)
def grid_used(stats, l2, what):
    used = stats.cpu().numpy()[:, 4]
    assert np.array_equal(used, (l2 > 0).astype(used.dtype)), f"{what}: grids used {used.tolist()}, len2 {l2.tolist()}"


@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.GRID_D)
@pytest.mark.parametrize("half", ["short", "long"])
def test_knn_grid_lists(dev, oracle, monkeypatch, half, D, norm):
    """grid_search<D, .> for every KC of kGridKC and the wave sort above 64, with and without the radius-2 quad pass
    (lists of up to 32 slots).  The diagnostics show that every cloud with a target went through its grid.  ("short":
    K <= 16, "long": the rest of the list.)"""
    from pytorch3d_pointops_amd import _C

    for K in [K for K in sic.knn_ks("grid", D, norm) if (K <= 16) == (half == "short")]:
        b = sic.batch("grid", D, K, sic.GRID_KC)
        planned(monkeypatch, "grid", b, D, K)
        t = device_batch(b, dev)
        want = oracle.knn_points_idx(b["p1"], b["p2"], b["l1"], b["l2"], norm, K)
        idx, dists, stats = _C.knn_grid_stats(*t, norm, K)
        assert_equal((idx, dists), want, label("grid", D, K, b["KC"], norm, ""))
        grid_used(stats, b["l2"], label("grid", D, K, b["KC"], norm, ""))
        for quad in ("grid_quad=0", "grid_quad=1") if K <= 32 else ():
            planned(monkeypatch, "grid", b, D, K, knobs=quad)
            assert_equal(_C.knn_points_idx(*t, norm, K, 3), want, label("grid", D, K, b["KC"], norm, quad))


@pytest.mark.parametrize("norm", sic.NORMS)
@pytest.mark.parametrize("D", sic.GRID_D)
@pytest.mark.parametrize("half", ["short", "long"])
def test_knn_grid_self_query(dev, oracle, monkeypatch, half, D, norm):
    """The queries are the points (one sort serves both sides), and the same call with that reuse switched off."""
    from pytorch3d_pointops_amd import _C

    for K in [K for K in sic.knn_ks("grid", D, norm) if (K <= 16) == (half == "short")]:
        b = sic.self_batch(D, K)
        planned(monkeypatch, "grid", b, D, K)
        t = device_batch(b, dev, self_query=True)
        want = oracle.knn_points_idx(b["p1"], b["p2"], b["l1"], b["l2"], norm, K)
        idx, dists, stats = _C.knn_grid_stats(*t, norm, K)
        assert_equal((idx, dists), want, label("grid self-query", D, K, b["KC"], norm, ""))
        grid_used(stats, b["l2"], label("grid self-query", D, K, b["KC"], norm, ""))
        planned(monkeypatch, "grid", b, D, K, knobs="grid_same=0")
        assert_equal(_C.knn_points_idx(*t, norm, K, 3), want, label("grid self-query", D, K, b["KC"], norm, "grid_same=0"))


# ------------------------------------------------------------------ ball query
@pytest.mark.parametrize("family,D", sic.BALL_IDS)
def test_ball_query(dev, oracle, monkeypatch, family, D):
    """ball_query_kernel / ball_small_kernel<1..4 | runtime D>, ball_grid_lane_kernel<D, KC> with its leftovers, and
    ball_query_list_kernel<D> over the lists of every query (K % 4 != 0, or ball_stage=0: the scan kernel reads the
    lists).  The grid is the candidate exactly when the workspace size is not 0."""
    from pytorch3d_pointops_amd import _C

    knobs, _, Ks = sic.BALL[family]
    for K in Ks:
        b = sic.ball_batch(D, K)
        t = device_batch(b, dev)
        N, P1, _ = b["p1"].shape
        for radius in sic.BALL_RADII:
            want = oracle.ball_query(b["p1"], b["p2"], b["l1"], b["l2"], K, radius)
            for value in knobs:
                knob(monkeypatch, value)
                grid = _C._lib.pointops_ball_query_workspace_bytes(N, P1, b["p2"].shape[1], D, K) > 0
                assert grid == ("ball_grid=1" in value), label(family, D, K, b["KC"], "-", value)
                assert_equal(_C.ball_query(*t, K, radius), want,
                             label(family, D, K, b["KC"], 2, value, f" radius {radius}"))
