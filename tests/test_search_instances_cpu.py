"""A certificate of the inputs of tests/test_search_instances_gpu.py, made with the source text, the dispatch's own
plan (pointops_knn_plan launches nothing and needs no device) and the oracle alone:

  * the value lists of tests/search_instance_cases.py are the lists of the source: every with_bucket / with_exact of
    the search files is read out of csrc/ as text and compared, so a new bucket, D or launch site fails here until the
    matrix learns it; every K list holds each bucket's last value and the next bucket's first;
  * the LDS-budget edges follow from kWideLdsMax, kLongKC and kLongQueue read the same way;
  * every (family, D, K) gets the family and the slice count it is there for from the plan;
  * every batch shows what it is there for, asserted from the oracle's output: an exact tie between the K-th and the
    (K+1)-th candidate of a query of the full cloud, clouds with len2 < K, == K and in (K, KC], an empty target and an
    empty query cloud, no valid coordinate equal to the padding; for the ball query a row with more than K points
    inside, a row partly -1 (K > 1), a row all -1 and a candidate at exactly radius^2 that is excluded;
  * the counts written in the docstring of search_instance_cases.py are what its generators yield.
"""
import os
import re

import numpy as np
import pytest

import search_instance_cases as sic

source, constant, CSRC = sic.source, sic.constant, sic.CSRC


def named_list(text, name):
    m = re.search(r"constexpr\s+Ints<([0-9,\s]+)>\s+" + name + r"\{\}", text)
    assert m, f"no Ints<...> {name}"
    return tuple(int(v) for v in m.group(1).split(","))


def dispatch_sites(name):
    """Every with_bucket / with_exact of a file, in order: (helper, fallback or None, list, selector).  A named list
    stays a name."""
    sites = []
    for m in re.finditer(r"with_(bucket|exact)(?:<(\d+)>)?\(\s*(Ints<[0-9,\s]+>\{\}|k\w+)\s*,\s*([^,]+),", source(name)):
        kind, fallback, values, selector = m.groups()
        if values.startswith("Ints<"):
            values = tuple(int(v) for v in values[5:values.index(">")].split(","))
        sites.append((kind, None if fallback is None else int(fallback), values, selector.strip()))
    return sites


NORM = ("exact", 2, sic.NORMS, "norm")

# file: its dispatch sites, in order, in terms of the lists of the matrix
SITES = {
    "knn.hip": [("bucket", None, "kScanKC", "a.K"),  # knn_merge_kernel<KC>
                NORM, ("exact", 0, "kScanD", "a.D"), ("bucket", None, "kScanKC", "a.K"),  # knn_reg_kernel<D, KC, NORM>
                NORM],  # knn_generic_kernel<NORM>
    "knn_small.hip": [NORM, ("exact", 0, "kScanD", "a.D"), ("bucket", None, "kScanKC", "a.K")],
    "knn_wide.hip": [("bucket", None, sic.WIDE_KC, "K"), ("exact", sic.WIDE_WG[1], sic.WIDE_WG[:1], "wg"), NORM,
                     NORM, NORM],  # <kLongKC, NORM, 64> and <0, NORM, 64>
    "knn_grid.hip": [("bucket", None, "kGridKC", "K"), ("exact", 3, sic.GRID_D, "a.D")],
    "knn_grid_search.h": [NORM, ("bucket", None, "kGridKC", "kc")],
    "knn_grid_wsort.hip": [NORM, ("exact", 3, sic.GRID_D, "a.D")],
    "ball_query.hip": [("exact", 3, sic.BALL_LIST_D, "(int)D"), ("exact", 0, sic.BALL_D, "(int)D")],
    "ball_small.hip": [("exact", 0, sic.BALL_D, "(int)D")],
    "ball_grid.hip": [("exact", 3, sic.BALL_LIST_D, "a.D"), ("bucket", None, sic.BALL_GRID_KC, "a.K"),
                      ("exact", 3, sic.BALL_LIST_D, "a.D")],
}


@pytest.mark.parametrize("name", sorted(SITES))
def test_dispatch_sites_are_the_ones_the_matrix_knows(name):
    assert dispatch_sites(name) == SITES[name], name


def test_named_lists_match_the_source():
    assert named_list(source("knn_grid.h"), "kScanD") == sic.SCAN_D
    assert named_list(source("knn_grid.h"), "kScanKC") == sic.SCAN_KC
    assert named_list(source("knn_grid_search.h"), "kGridKC") == sic.GRID_KC
    # every other search file dispatches through the sites above or not at all
    searched = {n for n in os.listdir(CSRC) if n.startswith(("knn", "ball")) and "backward" not in n}
    assert {n for n in searched if dispatch_sites(n)} == set(SITES)


@pytest.mark.parametrize("ks,caps,top", [
    (sic.REG_K, sic.SCAN_KC, 32), (sic.WIDE_K, sic.WIDE_KC, 32), (sic.GRID_K, sic.GRID_KC + (128,), 128),
    (sic.BALL[("ball_grid")][2], sic.BALL_GRID_KC, 64), (sic.ROTATING_K, sic.SCAN_KC, None),
    (sic.WIDE256_K, sic.WIDE_KC, None)], ids=["reg", "wide", "grid", "ball_grid", "rotating", "wide256"])
def test_k_lists_sit_on_the_bucket_edges(ks, caps, top):
    """Each bucket's last value and the next bucket's first (top = None: one value per bucket is all that is asked)."""
    assert tuple(sorted(set(ks))) == tuple(ks)
    assert {sic.bucket(K, caps) for K in ks} == set(caps), "a bucket without a K"
    if top is None:
        assert len(ks) == len(caps)
        return
    assert max(ks) == top
    firsts = {max(1 + c, min(ks)) for c in (0,) + caps[:-1]}
    assert set(caps) <= set(ks) and firsts <= set(ks), (sorted(set(caps) - set(ks)), sorted(firsts - set(ks)))
    assert any(sic.bucket(K, caps) > K for K in ks)


def test_ball_k_list():
    ks = sic.BALL_K
    assert {sic.bucket(K, sic.BALL_GRID_KC) for K in ks if K <= 64} == set(sic.BALL_GRID_KC)
    assert {63, 64, 65} <= set(ks)  # both sides of the grid path's and the staged kernel's limit
    assert {K % 4 for K in ks} == {0, 1, 3} and any(K % 4 == 0 and K <= 64 for K in ks)  # staged and unstaged


def test_long_and_lds_lists():
    text = source("knn_wide.hip")
    long_kc = constant(text, "kLongKC")
    assert min(sic.LONG_K) == max(sic.WIDE_KC) + 1 and max(sic.LONG_K) == long_kc
    assert any(max(sic.WIDE_KC) + 1 < K < long_kc for K in sic.LONG_K)
    assert min(sic.LDS_K) == long_kc + 1
    assert min(sic.WIDE_D) == max(sic.SCAN_D) + 1


def test_budget_edges_follow_from_the_constants():
    text = source("knn_wide.hip")
    lds_max, long_kc, queue = constant(text, "kWideLdsMax"), constant(text, "kLongKC"), constant(text, "kLongQueue")
    edges = sic.wide_budget_edges(lds_max, long_kc, queue)
    assert edges == sic.wide_budget_edges()
    assert edges == [(159, 4, True), (160, 4, False), (604, 40, True), (605, 40, False), (3, 316, True),
                     (3, 317, False)]  # by the constants today

    def lds(D, K):  # knn_wide_supported, term by term
        return D * 256 * 4 if K <= 32 else (D * 4 + (queue if K <= long_kc else K) * 8) * 64

    for D, K, inside in edges:
        assert (lds(D, K) <= lds_max - 1024) == inside, (D, K)
    assert re.search(r"\(size_t\)D \* 256 \* 4 <= kWideLdsMax - 1024", text)
    assert re.search(r"\(\(size_t\)D \* 4 \+ \(size_t\)kLongQueue \* 8\) \* 64 <= kWideLdsMax - 1024", text)
    assert re.search(r"\(\(size_t\)D \* 4 \+ \(size_t\)K \* 8\) \* 64 <= kWideLdsMax - 1024", text)


def test_counts_are_what_the_generators_yield():
    assert set(sic.COUNTS) == set(sic.KNN) | set(sic.BALL)
    for family in sic.KNN:
        inst = sic.grid_instances() if family == "grid" else sic.knn_instances(family)
        merges = len(sic.merge_instances(family)) if sic.KNN[family][4] == "many" else 0
        assert (len(inst) + merges, len(sic.knn_calls(family))) == sic.COUNTS[family], family
    for family in sic.BALL:
        assert (len(sic.ball_instances(family)), len(sic.ball_calls(family))) == sic.COUNTS[family], family
    # the register families reach every instance of the source's lists
    full = {(D, KC, norm) for D in sic.SCAN_D for KC in sic.SCAN_KC for norm in sic.NORMS}
    for family in ("scan64", "sliced", "small_q1", "small_gated_q1"):
        assert sic.knn_instances(family) == full, family
    assert {kc for _, kc, _ in sic.knn_instances("scan256")} == set(sic.SCAN_KC)
    assert sic.knn_instances("small_q2") == {i for i in full if i[1] <= 2} == sic.knn_instances("small_gated_q2")
    for family in ("wide64", "wide64_sliced", "wide256"):
        assert sic.knn_instances(family) == {(0, KC, norm) for KC in sic.WIDE_KC for norm in sic.NORMS}, family
    assert sic.grid_instances() == {(D, KC, norm) for D in sic.GRID_D for KC in (0,) + sic.GRID_KC for norm in sic.NORMS}
    assert sic.ball_instances("ball_grid") == {(D, KC) for D in sic.BALL_LIST_D for KC in sic.BALL_GRID_KC}
    assert sic.ball_instances("ball_scan") == set(sic.BALL_D) | {0} == sic.ball_instances("ball_small")
    assert sic.ball_instances("ball_list") == set(sic.BALL_LIST_D)
    # the docstring's table is COUNTS
    for family, (inst, calls) in sic.COUNTS.items():
        row = re.search(r"^\s+" + family + r"\s+([0-9+ ]+?)\s{2,}(\d+)\s", sic.__doc__, flags=re.M)
        assert row, family
        assert (sum(int(v) for v in row.group(1).split("+")), int(row.group(2))) == (inst, calls), family


# ------------------------------------------------------------------ the plan of every call
def plan(monkeypatch, knob, *shape):
    from pytorch3d_pointops_amd import _C

    monkeypatch.setenv("POINTOPS_DEBUG", knob) if knob else monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    return _C.knn_plan(*shape)


@pytest.mark.parametrize("family", sorted(sic.KNN))
def test_plan_of_every_call(monkeypatch, family):
    geometry, knob, version, want, slices, _, caps = sic.KNN[family]
    N, P1, p2_of = sic.GEOMETRY[geometry]
    seen = set()
    for D, norm, K in sic.knn_calls(family):
        P2 = p2_of(D, sic.bucket(K, caps))
        got, S = plan(monkeypatch, knob, N, P1, P2, D, K, version)
        assert got == want, (family, D, K, got)
        if slices == 1:
            assert S == 1, (family, D, K, S)
        else:
            assert 4 <= S <= 8 and S == min(8, P2 // 128), (family, D, K, S)
            seen.add(S)
        # the workgroup size is the launch's own comparison (launch_knn_bruteforce, launch_knn_wide)
        assert (N * -(-P1 // 256) >= 2048) == (geometry == "many")
    if slices != 1 and len(sic.KNN[family][5]) > 2:
        assert seen == {4, 5, 6, 7, 8}
    text = source("knn.hip") + source("knn_wide.hip")
    assert "a.N * a.tiles < 2048" in text and "a.N * ceil_div(a.P1, 256) < 2048 ? 64 : 256" in text


def test_plan_default_family_of_the_few_geometry(monkeypatch):
    """Without a knob the few-queries geometry takes the wave-per-query kernel: the knob only removes or keeps it."""
    N, P1, p2_of = sic.GEOMETRY["few"]
    assert plan(monkeypatch, "", N, P1, p2_of(3, 8), 3, 8, -1) == ("small", 1)
    assert plan(monkeypatch, "knn_small=0", N, P1, p2_of(3, 8), 3, 8, -1) == ("scan", 1)


def test_plan_reports_the_fall_through(monkeypatch):
    N, P1, p2_of = sic.GEOMETRY["few"]
    P2 = p2_of(0, 0)
    for version, D, K, want in sic.FALL_THROUGH:
        got = plan(monkeypatch, "", N, P1, P2, D, K, version)
        assert got == plan(monkeypatch, "", N, P1, P2, D, K, -1) and got[0] == want, (version, D, K, got)


def test_plan_at_the_budget_edges(monkeypatch):
    for D, K, inside in sic.wide_budget_edges():
        geometry, caps = sic.edge_batch_of(K)
        N, P1, p2_of = sic.GEOMETRY[geometry]
        P2 = p2_of(D, sic.bucket(K, caps))
        assert plan(monkeypatch, "", N, P1, P2, D, K, 0)[0] == ("wide" if inside else "generic"), (D, K)
        assert plan(monkeypatch, "knn_generic=1", N, P1, P2, D, K, 0)[0] == "generic", (D, K)
        assert (N * -(-P1 // 256) >= 2048) == (K <= 32)  # register lists: the 256-lane instance, D * 256 * 4 bytes
        b = sic.batch(geometry, D, K, caps)
        certify_lengths(b, K, ("edge", D, K))


def test_plan_of_nothing(monkeypatch):
    assert plan(monkeypatch, "", 0, 5, 5, 3, 1, -1) == ("none", 1)
    assert plan(monkeypatch, "", 2, 0, 5, 3, 1, -1) == ("none", 1)


def test_plan_agrees_with_its_siblings_and_refuses_null_pointers(monkeypatch):
    import ctypes

    from pytorch3d_pointops_amd import _C

    monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
    for shape in ((6, 131, 333, 3, 8), (2, 9000, 12000, 3, 16), (1, 64, 700, 3, 300), (6, 131, 640, 9, 5)):
        for version in (-1, 0, 2, 3):
            family, S = _C.knn_plan(*shape, version)
            assert (family == "grid") == bool(_C._lib.pointops_knn_uses_grid(*shape, version))
            nbytes = _C._lib.pointops_knn_workspace_bytes(*shape, version)
            assert (nbytes > 0) == (family == "grid" or S > 1), (shape, version, family, S, nbytes)
            if family != "grid":
                assert nbytes == (8 * shape[0] * shape[1] * S * shape[4] if S > 1 else 0)
    out = ctypes.c_int(7)
    assert _C._lib.pointops_knn_plan(6, 131, 333, 3, 8, -1, None, ctypes.byref(out)) == -1  # POINTOPS_EINVAL
    assert _C._lib.pointops_knn_plan(6, 131, 333, 3, 8, -1, ctypes.byref(out), None) == -1
    assert out.value == 7 and b"knn_plan" in _C._lib.pointops_last_error()
    assert "pointops_knn_plan" not in {"pointops_" + n for n in vars(_C._call)}  # host only: no stream, no launch


# ------------------------------------------------------------------ what every batch is there for
def certify_lengths(b, K, what):
    l1, l2, KC = b["l1"], b["l2"], b["KC"]
    P1, P2 = b["p1"].shape[1], b["p2"].shape[1]
    assert (l2 < K).any() and (l2 == K).any() and (l2 == 0).any() and (l1 == 0).any() and l1[0] == P1 and l2[0] == P2, what
    if KC > K:
        assert ((l2 > K) & (l2 <= KC)).any(), what
    assert ((l2 > KC) & (l2 < P2)).any() or KC + 1 >= P2, what
    for pts, lens in ((b["p1"], l1), (b["p2"], l2)):
        for n in range(min(len(lens), 12)):
            assert pts[n, :lens[n]].size == 0 or float(pts[n, :lens[n]].max()) <= 1.0, what
            assert (pts[n, lens[n]:] == sic.PAD).all(), what


def certify_tie(oracle, b, K, norm, what):
    """A query of the full cloud whose K-th and (K+1)-th candidates are at one distance (so at different indices)."""
    one = [b[k][:1] for k in ("p1", "p2", "l1", "l2")]
    idx, d = oracle.knn_points_idx(*one, norm, K + 1)
    tie = (d[0, :, K - 1] == d[0, :, K]) & (idx[0, :, K - 1] != idx[0, :, K])
    assert b["l2"][0] > K and tie.any(), what


@pytest.mark.parametrize("family,only", [
    pytest.param(f, None, id=f) for f in sorted(sic.KNN) if f not in ("small_q1", "small_q2", "small_gated_q2", "grid")
] + [pytest.param("grid", (D, norm), id=f"grid-d{D}-l{norm}") for D in sic.GRID_D for norm in sic.NORMS])
def test_knn_batches_show_what_they_are_there_for(oracle, family, only):
    """(small_q1 and small_q2 run the batches of scan64, small_gated_q2 those of small_gated_q1; the grid's big clouds
    go one (D, norm) at a time.)"""
    geometry, _, _, _, _, _, caps = sic.KNN[family]
    assert sic.KNN["small_q1"][0] == sic.KNN["small_q2"][0] == sic.KNN["scan64"][0]
    assert sic.KNN["small_gated_q2"][0] == sic.KNN["small_gated_q1"][0]
    for D, norm, K in [c for c in sic.knn_calls(family) if only in (None, c[:2])]:
        what = (family, D, norm, K)
        b = sic.batch(geometry, D, K, caps)
        assert b["KC"] == sic.bucket(K, caps) and b["p1"].shape[2] == D
        certify_lengths(b, K, what)
        certify_tie(oracle, b, K, norm, what)
        if geometry == "long":  # the gates of knn_small_kernel are refreshed: its own condition, at its step of 256
            first = -(-max(512, 128 * K) // 256) * 256
            assert first < b["l2"][0], what
        if family == "grid":
            s = sic.self_batch(D, K)
            assert s["p1"] is s["p2"] and s["l1"] is s["l2"]
            certify_tie(oracle, s, K, norm, what)


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5])
def test_ball_batches_show_what_they_are_there_for(oracle, D):
    for K in sic.BALL_K:
        b = sic.ball_batch(D, K)
        certify_lengths(b, K, ("ball", D, K))
        rows = {"more": False, "partly": False, "none": False, "edge": False}
        for radius in sic.BALL_RADII:
            r2 = np.float32(radius) * np.float32(radius)
            idx, _ = oracle.ball_query(b["p1"], b["p2"], b["l1"], b["l2"], K, radius)
            P2 = b["p2"].shape[1]
            every, dist = oracle.ball_query(b["p1"][:1], b["p2"][:1], b["l1"][:1], b["l2"][:1], P2, radius)
            inside = (every[0] >= 0).sum(axis=1)
            rows["more"] |= bool((inside > K).any())
            for n in range(6):
                hits = (idx[n, :b["l1"][n]] >= 0).sum(axis=1)
                rows["partly"] |= bool(((hits > 0) & (hits < K)).any())
                rows["none"] |= bool((hits == 0).any())
            # a candidate of the full cloud at exactly radius^2: the unfused fp32 distance of the oracle, recomputed
            diff = b["p1"][0][:, None, :] - b["p2"][0][None, :, :]
            d2 = np.zeros(diff.shape[:2], np.float32)
            for k in range(D):
                d2 = d2 + diff[:, :, k] * diff[:, :, k]
            at = np.argwhere(d2 == r2)
            if len(at):
                i, j = at[0]
                assert j not in every[0, i], ("ball", D, K, radius, i, j)
                assert (dist[0, i][every[0, i] >= 0] < r2).all()
                rows["edge"] = True
        if K == 1:
            rows["partly"] = True  # (a row of one slot is full or empty)
        assert all(rows.values()), ("ball", D, K, rows)
