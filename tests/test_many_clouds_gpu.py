"""Every operator on batches of 65 535 to 70 000 tiny clouds (tests/many_clouds_cases.py): N is launch geometry -- the
cloud is blockIdx.y (limit 65 535), or folded into blockIdx.x, or the batch runs in slices -- and nothing else in the
suite goes past 33 000 clouds.  Every cloud differs from the clouds 32 768 and 65 536 before it in length and in
points (asserted by test_many_clouds_cpu.py), so a launch that serves cloud n as n mod 32768 or n mod 65536, reads the
wrong lengths[n] or never writes the tail cannot pass; every assertion names the first failing cloud with both residues.

References: the C oracle bit for bit (searches, FPS, sample_pdf, gathers), scatter_ref's EXACT inputs bit for bit
(scatter backward passes), derived_ref's sequential fp32 restatement bit for bit (covariances), numpy restatements bit
for bit (packed <-> padded), and float64 with the bars of the existing GPU files (chamfer, frames, FPFH, alignment).
No tolerance here is new.  Which kernel each case reaches follows from the host predicates quoted in the docstrings
(the tests force paths with the POINTOPS_DEBUG knobs of csrc/debug.h).

Memory: batches are at most 70 000 clouds of <= 12 points (a few MB); the one large allocation is the grid search's own
workspace, 54 KB per cloud of a 32 768-cloud slice (1.74 GiB) whatever the clouds hold.
"""
import numpy as np
import pytest
import torch

import many_clouds_cases as mc
from oracle import oracle as oracle_py

pytestmark = pytest.mark.gpu

K4 = 4


def G(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def H(t):
    return t.detach().cpu().numpy()


def knob(monkeypatch, value):
    if value:
        monkeypatch.setenv("POINTOPS_DEBUG", value)
    else:
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)


def _C():
    from pytorch3d_pointops_amd import _C as c

    return c


_MEMO = {}


def memo(key, fn):
    """A reference computed once and shared (never written)."""
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def oracle_knn(oracle, N, norm, K, D=3, P1=6):
    b = mc.batch(N, D=D, P1=P1)
    return memo(("knn", N, norm, K, D, P1), lambda: oracle.knn_points_idx(b["p1"], b["p2"], b["l1"], b["l2"], norm, K))


def check_search(got, want, what):
    """(idx, dists) against the oracle, bit for bit, padding included."""
    mc.assert_clouds_equal(H(got[0]), want[0], f"{what}: idx")
    mc.assert_clouds_equal(H(got[1]), want[1], f"{what}: dists", as_bits=True)


# ================================================================================================ knn_points_idx
KNN_PATHS = [  # (name, version, knob): D = 3, K = 4
    ("auto", -1, None),          # choose_version -> 2 (P2 < 4096: no grid); N * ceil(P1 / 64) >= 2048 -> knn_reg_kernel
    ("v0_wide", 0, None),        # knn_wide.hip, register lists, 256-lane workgroups (N * tiles >= 2048)
    ("v0_generic", 0, "knn_generic=1"),  # knn_generic_kernel
    ("v1", 1, None),             # knn_reg_kernel, cloud = blockIdx.x / tiles
    ("v2", 2, None),
    ("v2_small", 2, "knn_small=1"),  # knn_small_kernel: by itself only below 2048 query waves, never at this N
]


@pytest.mark.parametrize("N", mc.EDGE_NS)
def test_knn_versions(dev, oracle, monkeypatch, N):
    """version -1, 0, 1, 2 (and the generic and wave-per-query kernels behind their knobs) at D = 3, K = 4: all fold
    the cloud into blockIdx.x = n * tiles + tile.  The 64-lane / split forms of the scan and of knn_wide need
    N * tiles < 2048 and cannot be reached at this N."""
    b = mc.batch(N)
    want = oracle_knn(oracle, N, 2, K4)
    args = [G(b[k], dev) for k in ("p1", "p2", "l1", "l2")]
    for name, version, kb in KNN_PATHS:
        knob(monkeypatch, kb)
        check_search(_C().knn_points_idx(*args, 2, K4, version), want, f"knn {name} N={N}")


@pytest.mark.parametrize("N", mc.EDGE_NS)
def test_knn_wide_shapes(dev, oracle, monkeypatch, N):
    """D = 9 (no register-scan instance: version -1 falls to knn_wide's register lists) and K = 33 (knn_wide's LDS
    lists; K exceeds every cloud, so every row carries padding), L1 on the second."""
    knob(monkeypatch, None)
    b = mc.batch(N, D=9)
    want = oracle_knn(oracle, N, 2, K4, D=9)
    check_search(_C().knn_points_idx(*[G(b[k], dev) for k in ("p1", "p2", "l1", "l2")], 2, K4, -1), want,
                 f"knn D=9 N={N}")
    b = mc.batch(N, P1=4)
    want = oracle_knn(oracle, N, 1, 33, P1=4)
    check_search(_C().knn_points_idx(*[G(b[k], dev) for k in ("p1", "p2", "l1", "l2")], 1, 33, -1), want,
                 f"knn K=33 N={N}")


@pytest.mark.parametrize("N", mc.SLICE_NS)
def test_knn_grid_slices(dev, oracle, monkeypatch, N):
    """version = 3 in one, two and three slices of 32 768 clouds (knn_grid.hip: knn_grid_run), K in {1, 8, 16}, both
    norms, ragged on both sides with empty clouds -- none of which the sliced path had run with.  Clouds this small have
    no usable grid, so every slice goes build -> lane search -> whole-cloud fallback with slice-relative cloud indices
    over offset pointers."""
    knob(monkeypatch, None)
    b = mc.batch(N)
    args = [G(b[k], dev) for k in ("p1", "p2", "l1", "l2")]
    for K in (1, 8, 16):
        for norm in (2, 1):
            assert _C()._lib.pointops_knn_uses_grid(N, 6, 10, 3, K, 3) == 1
            check_search(_C().knn_points_idx(*args, norm, K, 3), oracle_knn(oracle, N, norm, K),
                         f"knn grid K={K} L{norm} N={N}")


def test_knn_grid_self_query_in_three_slices(dev, oracle, monkeypatch):
    """p1 is p2 and lengths1 is lengths2: the self-query is recognised by pointer equality, which every slice's offset
    pointers must preserve (s.p2 = s.p1, s.l2 = s.l1).  With grid_same=0 the same call sorts the queries separately."""
    N = 65537
    b = mc.batch(N)
    p, l = G(b["p2"], dev), G(b["l2"], dev)
    want = memo(("knn_self", N), lambda: oracle.knn_points_idx(b["p2"], b["p2"], b["l2"], b["l2"], 2, 8))
    for kb in (None, "grid_same=0"):
        knob(monkeypatch, kb)
        check_search(_C().knn_points_idx(p, p, l, l, 2, 8, 3), want, f"knn grid self-query ({kb})")


def test_knn_grid_diagnostics_per_slice(dev, oracle, monkeypatch):
    """knn_grid_stats / knn_grid_fallback_counts take N <= 32768: each slice of the 65 537-cloud batch through them.
    Results equal the oracle's rows of that slice; the two diagnostics agree with each other; the per-cloud geometry
    columns equal those of a run over the probe clouds alone (stats are read per cloud: an aliased read shows)."""
    knob(monkeypatch, None)
    N, K = 65537, 8
    b = mc.batch(N)
    want = oracle_knn(oracle, N, 2, K)
    pr = mc.probe_set(N)
    sub = [G(b[k][pr], dev) for k in ("p1", "p2", "l1", "l2")]
    _, _, probe_stats = _C().knn_grid_stats(*sub, 2, K)
    probe_stats = H(probe_stats)
    for a in range(0, N, mc.SLICE):
        sl = slice(a, min(a + mc.SLICE, N))
        args = [G(b[k][sl], dev) for k in ("p1", "p2", "l1", "l2")]
        idx, dists, stats = _C().knn_grid_stats(*args, 2, K)
        check_search((idx, dists), (want[0][sl], want[1][sl]), f"knn_grid_stats slice at {a}")
        idx, dists, counts = _C().knn_grid_fallback_counts(*args, 2, K)
        check_search((idx, dists), (want[0][sl], want[1][sl]), f"knn_grid_fallback_counts slice at {a}")
        stats, counts = H(stats), H(counts)
        l1 = b["l1"][sl]
        assert stats.shape == (sl.stop - a, 14) and counts.shape == (2, sl.stop - a)
        mc.assert_clouds_equal(counts[0], stats[:, 5], f"slice at {a}: wave-search counts")
        mc.assert_clouds_equal(counts[1], stats[:, 7], f"slice at {a}: whole-cloud counts")
        bad = (stats[:, 7] < 0) | (stats[:, 7] > l1) | (stats[:, 5] < 0) | (stats[:, 5] > l1) | (stats[:, 4] < 0) \
            | (stats[:, 4] > 1)
        assert not bad.any(), f"slice at {a}: counters out of range: {mc.first_bad(bad)}"
        inside = (pr >= a) & (pr < sl.stop)
        mc.assert_clouds_equal(stats[pr[inside] - a][:, :5], probe_stats[inside][:, :5],
                               f"slice at {a}: grid geometry", clouds=pr[inside])


# ================================================================================================ knn_points_backward
KNN_BWD = [  # (name, D, plans)
    ("four_lane_D3", 3, ["atomic", "tiled_s1", "tiled_s2", "deterministic"]),
    ("generic_D5", 5, ["atomic", "deterministic"]),  # C > 4 has no LDS-tile form
]


def _choose(monkeypatch, op, plan):
    if plan == "deterministic":
        knob(monkeypatch, None)
        return True
    knob(monkeypatch, f"{op}_bwd_mode=atomic" if plan == "atomic"
         else f"{op}_bwd_mode=tiled,{op}_bwd_split={plan[-1]}")
    return False


@pytest.mark.parametrize("N", mc.EDGE_NS)
@pytest.mark.parametrize("name,D,plans", KNN_BWD, ids=[c[0] for c in KNN_BWD])
def test_knn_backward_plans_exact(dev, monkeypatch, name, D, plans, N):
    """scatter_ref's EXACT inputs (lattice coordinates, integer gradients, max A < 2^22 asserted by the generator): no
    addition rounds, so device atomics (the four-lane kernel at D <= 4, knn_backward_kernel<0> at D = 5), LDS tiles
    without and with a row split, and the deterministic form must all return the float64 sum cast to fp32, bit for
    bit, in every cloud.  All of them recover the cloud from a flat index by division."""
    p1, p2, l1, l2, idx, grad, ref = memo(("knn_bwd", N, D), lambda: mc.exact_knn_backward_inputs(N, D))
    w1, w2 = ref.g1.astype(np.float32), ref.g2.astype(np.float32)
    t = [G(a, dev) for a in (p1, p2, l1, l2, idx)]
    for plan in plans:
        det = _choose(monkeypatch, "knn", plan)
        g1, g2 = _C().knn_points_backward(*t, 2, G(grad, dev), deterministic=det)
        mc.assert_clouds_equal(H(g1), w1, f"knn backward {name} {plan} N={N}: grad_p1", as_bits=True)
        mc.assert_clouds_equal(H(g2), w2, f"knn backward {name} {plan} N={N}: grad_p2", as_bits=True)


# ================================================================================================ ball_query
BALL_RADIUS = 0.25  # lattice clouds (spacing 0.25) put distances exactly on radius^2, where the test is strict '<'


@pytest.mark.parametrize("N", mc.EDGE_NS)
def test_ball_query_paths(dev, oracle, monkeypatch, N):
    """Auto must be the scan: ball_grid_candidate needs P2 >= 4096 and N < 65536 (ball_query.hip), so no workspace is
    asked for and ball_query_kernel<3> runs in storage order (cloud = blockIdx.x / tiles).  ball_small=1 forces the
    wave-per-query kernel, which by itself needs N * ceil(P1 / 64) < 2048.  D = 5 takes the runtime-D instance.
    Unreachable here: the staged list kernel and the coarse-cell query order (both need the grid's lists: flag != null,
    i.e. ball_grid_candidate; even ball_grid=1 is declined by its N < 65536 at the two larger N, and at N = 65 535 it
    would need a 4.5 GB workspace, which this file does not allocate)."""
    b = mc.batch(N)
    args = [G(b[k], dev) for k in ("p1", "p2", "l1", "l2")]
    want = memo(("ball", N), lambda: oracle.ball_query(b["p1"], b["p2"], b["l1"], b["l2"], K4, BALL_RADIUS))
    full, some = (want[0] >= 0).all(-1), (want[0] >= 0).any(-1)
    on_radius = memo(("ball_on_radius", N), lambda: _hits_on_radius(b))
    assert full.any() and (some & ~full).any() and (~some).any() and on_radius > 0, "the radius exercises every row kind"
    for kb in (None, "ball_small=1", "ball_grid=1" if N >= mc.GRID_Y else "ball_grid=0"):
        knob(monkeypatch, kb)
        assert _C()._lib.pointops_ball_query_workspace_bytes(N, 6, 10, 3, K4) == 0, "the grid declines"
        check_search(_C().ball_query(*args, K4, BALL_RADIUS), want, f"ball_query ({kb}) N={N}")
    knob(monkeypatch, None)
    b5 = mc.batch(N, D=5)
    want5 = memo(("ball5", N), lambda: oracle.ball_query(b5["p1"], b5["p2"], b5["l1"], b5["l2"], K4, 0.6))
    check_search(_C().ball_query(*[G(b5[k], dev) for k in ("p1", "p2", "l1", "l2")], K4, 0.6), want5,
                 f"ball_query D=5 N={N}")


def _hits_on_radius(b):
    d2 = ((b["p1"][::5, :, None, :] - b["p2"][::5, None, :, :]) ** 2).sum(-1)
    return int((d2 == np.float32(BALL_RADIUS) * np.float32(BALL_RADIUS)).sum())


# ================================================================================================ FPS
@pytest.mark.parametrize("N", mc.EDGE_NS)
def test_sample_farthest_points(dev, oracle, monkeypatch, N):
    """One workgroup per cloud on blockIdx.x in all three kernels: fps_single_kernel<.., 256> (D = 3, D = 2),
    fps_single_kernel<.., 1024> (fps_small=0) and fps_kernel (D = 4, running minima in the workspace, one row per
    cloud).  Per-cloud K ragged with 0 and K > length, empty clouds, random start indices.  The cluster kernel needs
    clouds above 8192 points."""
    for D, kb in ((3, None), (3, "fps_small=0"), (2, None), (4, None)):
        knob(monkeypatch, kb)
        b = mc.batch(N, D=D)
        pts, lens = b["p2"], b["l2"]
        Ks = mc.fps_k(N, 10)
        for start in (np.zeros(N, np.int64), mc.fps_start(lens)):
            want = oracle.sample_farthest_points(pts, lens, Ks, start)
            got = _C().sample_farthest_points(G(pts, dev), G(lens, dev), G(Ks, dev), G(start, dev))
            mc.assert_clouds_equal(H(got), want, f"FPS D={D} ({kb}) start={'given' if start.any() else 0} N={N}")
    assert (Ks == 0).any() and (Ks > lens).any() and (lens == 0).any()


# ================================================================================================ gather
def _gather_tables(oracle, N):
    b = mc.batch(N)
    knn_idx = oracle_knn(oracle, N, 2, K4)[0]
    ball_idx = memo(("ball", N), lambda: oracle.ball_query(b["p1"], b["p2"], b["l1"], b["l2"], K4, BALL_RADIUS))[0]
    return b, knn_idx, ball_idx


@pytest.mark.parametrize("N", mc.EDGE_NS)
def test_gather_neighbors(dev, oracle, N):
    """U = 1, 2, 3, 4, 7 with lengths (knn_gather's mask) and with -1 entries (masked_gather's).  gather.hip:134 sends
    N < 65536 to gather_rows_kernel<U> (U <= 4) / gather_elems32_kernel (U = 7), cloud on blockIdx.y -- N = 65 535 is the
    largest legal grid.y -- and N >= 65536 to the 64-bit gather_kernel, which no other test reaches."""
    b, knn_idx, ball_idx = _gather_tables(oracle, N)
    assert (ball_idx < 0).any() and (b["l2"] < K4).any()
    for U in (1, 2, 3, 4, 7):
        x = mc.points(500 + U, N, 10, U)
        got = _C().gather_neighbors(G(x, dev), G(knn_idx, dev), G(b["l2"], dev))
        mc.assert_clouds_equal(H(got), oracle_py.knn_gather(x, knn_idx, b["l2"]), f"knn_gather U={U} N={N}",
                               as_bits=True)
        got = _C().gather_neighbors(G(x, dev), G(ball_idx, dev), None)
        mc.assert_clouds_equal(H(got), oracle_py.masked_gather(x, ball_idx), f"masked_gather U={U} N={N}", as_bits=True)


@pytest.mark.parametrize("N", mc.EDGE_NS)
def test_gather_backward_plans_exact(dev, monkeypatch, N):
    """Exact inputs as for the knn backward: device atomics (flat 64-bit index), LDS tiles without and with a row
    split, deterministic; with and without lengths; U = 3 and (atomics / deterministic only) U = 7."""
    for U, plans in ((3, ["atomic", "tiled_s1", "tiled_s2", "deterministic"]), (7, ["atomic", "deterministic"])):
        for with_lengths in (True, False):
            go, idx, lengths, ref = memo(("gather_bwd", N, U, with_lengths),
                                         lambda: mc.exact_gather_backward_inputs(N, U, with_lengths=with_lengths))
            want = ref.gx.astype(np.float32)
            for plan in plans:
                det = _choose(monkeypatch, "gather", plan)
                gx = _C().gather_neighbors_backward(G(go, dev), G(idx, dev), G(lengths, dev), 10, deterministic=det)
                mc.assert_clouds_equal(H(gx), want, f"gather backward U={U} {plan} lengths={with_lengths} N={N}",
                                       as_bits=True)


# ================================================================================================ covariances, sample_pdf
@pytest.mark.parametrize("N", mc.EDGE_NS)
@pytest.mark.parametrize("K", [21, 22], ids=["staged_KD63", "per_row_KD66"])
def test_point_covariances(dev, N, K):
    """K * D = 63 / 66 at D = 3: the staged and the per-row form (covariance.hip), flat rows N * P, against
    derived_ref's sequential fp32 restatement, every value, forward and backward."""
    import derived_ref as dr
    from pytorch3d_pointops_amd import synth

    P, D = 2, 3
    knn = (synth.uniform_f32(8100 + K, (N, P, K, D)) * np.float32(2) - np.float32(0.75)).astype(np.float32)
    g = (synth.uniform_f32(8200 + K, (N, P, D, D)) * np.float32(2) - np.float32(1)).astype(np.float32)
    mc.assert_clouds_equal(H(_C().point_covariances(G(knn, dev))), dr.cov_fp32(knn), f"covariances K={K} N={N}",
                           as_bits=True)
    mc.assert_clouds_equal(H(_C().point_covariances_backward(G(knn, dev), G(g, dev))), dr.cov_backward_fp32(knn, g),
                           f"covariances backward K={K} N={N}", as_bits=True)


def test_sample_pdf_65537_rows(dev, oracle):
    """One workgroup per row on blockIdx.x: 65 537 rows, 5 bins, 3 samples, every row its own bins and weights."""
    from pytorch3d_pointops_amd import synth

    B, nb, ns = 65537, 5, 3
    bins = np.sort(synth.uniform_f32(711, (B, nb + 1)), axis=1).astype(np.float32)
    w = synth.uniform_f32(712, (B, nb))
    w[::7, :2] = 0.0
    u = synth.uniform_f32(713, (B, ns))
    u[::11, 0], u[::13, -1] = 0.0, 1.0
    out = G(u, dev)
    _C().sample_pdf(G(bins, dev), G(w, dev), out, 1e-5)
    mc.assert_clouds_equal(H(out), oracle.sample_pdf(bins, w, u, 1e-5), "sample_pdf", as_bits=True)


# ================================================================================================ chamfer_reduce
@pytest.mark.parametrize("N", mc.EDGE_NS)
def test_chamfer_reduce(dev, N):
    """One workgroup per cloud on blockIdx.x; float64 sums, the loss bar of test_chamfer_float64_gpu.py
    (1e-5 max(1, |ref|)), per cloud."""
    from pytorch3d_pointops_amd import synth

    b = mc.batch(N)
    d = synth.uniform_f32(720, (N, 6))
    w = (synth.uniform_f32(721, (N,)) + np.float32(0.25)).astype(np.float32)
    valid = np.arange(6)[None, :] < b["l1"][:, None]
    for mean in (False, True):
        for weights in (None, w):
            want = np.where(valid, d.astype(np.float64), 0).sum(1)
            if weights is not None:
                want = want * weights
            if mean:
                want = want / np.maximum(b["l1"], 1)
            got = H(_C().chamfer_reduce(G(d, dev), G(b["l1"], dev), G(weights, dev), mean))
            mc.assert_clouds_close(got, want, 1e-5 * np.maximum(1.0, np.abs(want)),
                                   f"chamfer_reduce mean={mean} weights={weights is not None} N={N}")


# ================================================================================================ packed <-> padded
@pytest.mark.parametrize("N", mc.EDGE_NS + (mc.N_BIG,))
def test_packed_padded(dev, N):
    """packed_to_padded / padded_to_packed past blockIdx.y: a dense layout with a trailing (2, 3) dimension through the
    functions, and a layout with packed rows owned by no cloud (they stay zero) through the operator boundary.  numpy
    restatement (held to the oracle and the reference by the CPU test), bit for bit.  The entries run slices of 65 535
    clouds; the last cloud's end is F, which only the last slice may see."""
    from pytorch3d_pointops_amd import synth
    from pytorch3d_pointops_amd.functions.packed_to_padded import packed_to_padded, padded_to_packed

    b = mc.batch(N)
    lens = b["l2"]
    first = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    F = int(lens.sum())
    x = (synth.uniform_f32(57, (F, 2, 3)) + np.float32(0.5)).astype(np.float32)
    want = mc.packed_to_padded_np(x.reshape(F, 6), first, 10).reshape(N, 10, 2, 3)
    padded = packed_to_padded(G(x, dev), G(first, dev), 10)
    mc.assert_clouds_equal(H(padded), want, f"packed_to_padded N={N}", as_bits=True)
    back = H(padded_to_packed(padded, G(first, dev), F))
    assert np.array_equal(mc.bits(back), mc.bits(x)), f"padded_to_packed N={N}: the round trip is not the input"
    full = np.where(np.arange(N) % 3 == 0, 10, lens)  # gapped clouds are full: their extra row lies past max_size
    first, F = mc.gapped_first_idxs(full)
    x = (synth.uniform_f32(58, (F, 3)) + np.float32(0.5)).astype(np.float32)
    want = mc.packed_to_padded_np(x, first, 10)
    padded = _C().packed_to_padded(G(x, dev), G(first, dev), 10)
    mc.assert_clouds_equal(H(padded), want, f"packed_to_padded (gaps) N={N}", as_bits=True)
    back = H(_C().padded_to_packed(padded, G(first, dev), F))
    want_back = mc.padded_to_packed_np(want, first, F)
    owner = np.repeat(np.arange(N), np.diff(np.concatenate([first, [F]])))  # cloud of every packed row from first[0] on
    bad = (mc.bits(back) != mc.bits(want_back)).any(1)
    assert not bad.any(), f"padded_to_packed (gaps) N={N}: {mc.first_bad(_by_cloud(bad[first[0]:], owner, N))}"
    assert (want_back == 0).all(1).sum() >= (N + 2) // 3, "owner-less rows exist and are zero"


def _by_cloud(bad_rows, owner, N):
    out = np.zeros(N, bool)
    out[owner[bad_rows]] = True
    return out


@pytest.mark.parametrize("N", [65535, 65537])
def test_pointclouds_list_packed_padded(dev, N):
    """A Pointclouds of N small patches: list -> packed -> padded and padded -> packed, the conversions the reference's
    own API makes, which used to raise "bad sizes" above 65 535 clouds."""
    from pytorch3d_pointops_amd.structures import Pointclouds

    b = mc.batch(N)
    lens, pts = b["l2"], b["p2"]
    valid = np.arange(10)[None, :] < lens[:, None]
    packed = G(pts[valid], dev)
    pc = Pointclouds(list(torch.split(packed, lens.tolist())))
    assert torch.equal(pc.points_packed(), packed)
    want = np.where(valid[..., None], pts, 0)
    mc.assert_clouds_equal(H(pc.points_padded()), want, f"Pointclouds list -> padded N={N}", as_bits=True)
    full = Pointclouds(G(pts, dev))  # a padded tensor: every cloud has 10 points
    assert np.array_equal(mc.bits(H(full.points_packed())), mc.bits(pts.reshape(-1, 3)))


# ================================================================================================ chamfer_distance
def _chamfer_case(N, normals):
    from pytorch3d_pointops_amd import synth

    b = mc.batch(N)
    fx = {"n": synth.unit_normals(730, (N, 6, 3))} if normals else {}
    fy = {"n": synth.unit_normals(731, (N, 10, 3))} if normals else {}
    return dict(name=f"many{N}", x=b["p1"], y=b["p2"], xl=b["l1"], yl=b["l2"], fx=fx, fy=fy, norm=2, abs_cosine=True,
                lattice=True)


CHAMFER_ROUTES = {  # route -> (kwargs, mode of test_chamfer_float64_gpu._mode, normals, expected call counts)
    "pair_mean_normals": (dict(point_reduction="mean", batch_reduction="mean"), None, True, (1, 0, 0)),
    "pair_none_normals": (dict(point_reduction="sum", batch_reduction=None), None, True, (1, 0, 0)),
    "pair_sum": (dict(point_reduction="mean", batch_reduction="sum"), None, False, (1, 0, 0)),
    "direction_sum_weights_normals": (dict(point_reduction="mean", batch_reduction="sum", weights="w"), None, True,
                                      (0, 2, 0)),
    "direction_single_none": (dict(point_reduction="sum", batch_reduction=None, single_directional=True), None, False,
                              (0, 1, 0)),
    "composed_forced_sum_normals": (dict(point_reduction="mean", batch_reduction="sum"), "forced", True, (0, 0, 2)),
    "composed_unreduced": (dict(point_reduction=None, batch_reduction=None), None, False, (0, 0, 2)),
}


@pytest.mark.parametrize("N", [65535, 65537])
@pytest.mark.parametrize("route", sorted(CHAMFER_ROUTES))
def test_chamfer_distance_routes(dev, oracle, monkeypatch, route, N):
    """chamfer_distance through the one-call pair entry, the per-direction fused node and the composed path, with and
    without normals, forward and backward, batch_reduction mean / sum / None, against chamfer_ref in float64 over ALL
    clouds with the bars of test_chamfer_float64_gpu.py (losses 1e-5 max(1, |ref|); gradients 1e-4 |ref| + 1e-5
    max(1, max |ref|); under batch_reduction "mean" every gradient is 1 / N of a cloud's and that bar says little, so
    the gradients are really held by the "sum" and None routes).  The fused entries refused N >= 65536 before; they now
    run slices of 65 535 clouds, and the pair entry's batch reduction must cover all of them."""
    import test_chamfer_float64_gpu as cf
    from chamfer_ref import CachedKnn
    from pytorch3d_pointops_amd import synth

    knob(monkeypatch, None)
    kw, mode, normals, expect = CHAMFER_ROUTES[route]
    kw = dict(kw)
    if kw.get("weights") == "w":
        kw["weights"] = (synth.uniform_f32(732, (N,)) + np.float32(0.25)).astype(np.float32)
    c = _chamfer_case(N, normals)
    knn = memo(("chamfer_knn", N), lambda: CachedKnn(oracle))
    calls = cf._counting(monkeypatch)
    with cf._mode(monkeypatch, mode):
        got = cf._run_gpu(dev, c, kw)
    assert (calls["pair"], calls["forward"], calls["composed"]) == expect, (route, calls)
    want = cf._run_ref(knn, c, kw)
    assert [t for t, _ in got["outputs"]] == [t for t, _ in want["outputs"]]
    for (tag, a), (_, r) in zip(got["outputs"], want["outputs"]):
        assert a.shape == r.shape, (route, tag)
        if a.ndim == 0:
            err = abs(float(a) - float(r))
            assert err <= 1e-5 * max(1.0, abs(float(r))), (route, tag, float(a), float(r))
        else:
            mc.assert_clouds_close(a, r, 1e-5 * np.maximum(1.0, np.abs(r)), f"chamfer {route} N={N}: {tag}")
    for key, a, r in [("grad_x", got["grad_x"], want["grad_x"]), ("grad_y", got["grad_y"], want["grad_y"])] + \
            [(f"{key}/{k}", got[key][k], want[key][k]) for key in ("grad_xf", "grad_yf") for k in want[key]]:
        tol = 1e-4 * np.abs(r) + 1e-5 * max(1.0, float(np.abs(r).max()))
        mc.assert_clouds_close(a, r, tol, f"chamfer {route} N={N}: {key}")


# ================================================================================================ frames, FPFH
def _self_table(dev, N, K):
    b = mc.batch(N)
    p, l = G(b["p2"], dev), G(b["l2"], dev)
    return b["p2"], b["l2"], _C().knn_points_idx(p, p, l, l, 2, K, -1)[0]


def test_local_frames_at_65535_clouds(dev, monkeypatch):
    """N = 65 535, the largest batch local_frames takes (cloud on blockIdx.y): every check of
    test_derived_edges_gpu._frames_forward_checks over ALL clouds (the same C bit for bit, eigenvalues, orthogonality,
    reconstruction, columns 0 and 2 the raw columns up to sign, y = n x z), and the backward against its float64 closed
    form with that file's per-row bar -- the backward has flat rows and no batch limit, so it also runs at 65 537.

    The majority rule of the sign is checked on the four clouds in five that are not on the lattice, as a batch of their
    own, and the full batch must give those clouds the same bits.  Lattice neighbourhoods are often coplanar with
    projections on their normal that are EXACTLY zero in float64 (rational geometry) while the kernel's fp32 sum rounds
    to +-1e-8: the sign of rounding noise, which that check excludes for K = 3 and for tiny non-zero projections but
    cannot see at an exact zero (seven rows of this batch)."""
    import test_derived_edges_gpu as de

    knob(monkeypatch, None)
    N, K = 65535, 4
    pts, lens, idx = _self_table(dev, N, K)
    idx = H(idx)
    de._frames_forward_checks(dev, pts, idx, lens, f"local_frames N={N}", sign_check=False)
    keep = np.arange(N) % 5 != 0
    de._frames_forward_checks(dev, pts[keep], idx[keep], lens[keep], f"local_frames N={N}, random clouds",
                              sign_check=True)
    full = _C().local_frames(G(pts, dev), G(lens, dev), G(idx, dev), True)
    sub = _C().local_frames(G(pts[keep], dev), G(lens[keep], dev), G(idx[keep], dev), True)
    for name, a, c in zip(("curvatures", "frames"), full, sub):
        mc.assert_clouds_equal(H(a)[keep], H(c), f"local_frames {name}: full batch against its random clouds alone",
                               as_bits=True, clouds=np.nonzero(keep)[0])
    for n in (65535, 65537):
        de.test_local_frames_backward_per_entry(dev, n, 10, mc.batch(n)["l2"], True)


def test_fpfh_at_65535_clouds(dev, monkeypatch):
    """N = 65 535, the largest batch the FPFH entries take: pair features, SPFH bits and FPFH values over ALL clouds
    with the stages and bars of test_fpfh_gpu.py (fpfh_ref is vectorised over clouds)."""
    import test_fpfh_gpu as tf
    from pytorch3d_pointops_amd import synth

    knob(monkeypatch, None)
    N, K = 65535, 4
    pts, lens, idx = _self_table(dev, N, K)
    r = tf._Run(dev, pts, synth.unit_normals(740, (N, 10, 3)), lens, idx)
    have = tf._staged(r, f"fpfh N={N}")
    assert np.isfinite(have).all()
    sums = tf._group_sums(r.spfh.cpu().numpy())
    counted = (r.pair.cpu().numpy()[..., 3] > 0).any(-1)
    bad = np.abs(sums - np.where(counted[..., None], 100.0, 0.0)) > 1e-3
    assert not bad.any(), f"SPFH group sums: {mc.first_bad(bad)}"


LIMIT = "65536"


def _refused(monkeypatch, call):
    """`call` must raise an error naming the limit, launch nothing and leave every output it allocated as it was:
    guarded buffers (tests/buffers.py) filled with 0xFF."""
    import buffers

    with buffers.contract(monkeypatch, "ones") as c:
        with pytest.raises(RuntimeError, match=LIMIT):
            call()
    c.assert_guards_intact()
    outs = [b for b in c.buffers if b.kind == "out"]
    assert outs
    for b in outs:
        assert bool((b.payload == 0xFF).all()), f"a refused call wrote into {b.name}"


def test_limited_entries_refuse_65536_clouds(dev, monkeypatch):
    """local_frames, the FPFH entries and the ICP iteration keep N < 65536 (stated in include/pointops_amd.h): at
    N = 65 536 their wrappers raise an error that names the limit, no kernel runs and the outputs keep their fill."""
    from pytorch3d_pointops_amd import _C_descriptors as dsc
    from pytorch3d_pointops_amd import synth

    knob(monkeypatch, None)
    N, K = 65536, 4
    pts, lens, idx = _self_table(dev, N, K)
    p, l = G(pts, dev), G(lens, dev)
    nrm = G(synth.unit_normals(741, (N, 10, 3)), dev)
    spfh = torch.zeros((N, 10, 33), device=dev)
    _refused(monkeypatch, lambda: _C().local_frames(p, l, idx, True))
    _refused(monkeypatch, lambda: dsc.spfh(p, nrm, idx, l, want_pair_features=True))
    _refused(monkeypatch, lambda: dsc.fpfh(p, idx, l, spfh))
    b = mc.batch(N)
    x, lx = G(b["p1"], dev), G(b["l1"], dev)
    _refused(monkeypatch, lambda: _C().IcpState(x, x.clone(), p, lx, l, 1, False, False, 1e-6).step())


# ================================================================================================ alignment, ICP
def _alignment_inputs(N):
    """X = the batch's targets, Y = s X R + T + 0.01 noise with a random similarity transform per cloud (what
    test_points_alignment_gpu._moved builds cloud by cloud, vectorised), mask = the validity of each row."""
    import test_derived_edges_gpu as de

    b = mc.batch(N)
    rng = np.random.default_rng(7700)
    X = b["p2"].astype(np.float64)
    Rm = de._rotations(7701, (N,))
    s = 0.7 + 0.6 * rng.random((N, 1, 1))
    Y = s * np.einsum("npa,nab->npb", X, Rm) + (rng.random((N, 1, 3)) - 0.5) + 0.01 * rng.standard_normal(X.shape)
    mask = (torch.arange(10)[None, :] < torch.from_numpy(b["l2"])[:, None]).float()
    return torch.from_numpy(b["p2"].copy()), torch.from_numpy(Y.astype(np.float32)), mask


@pytest.mark.parametrize("N", mc.EDGE_NS)
def test_alignment_against_float64(dev, monkeypatch, N):
    """corresponding_points_alignment with the validity mask as weights (ragged clouds, empty ones included) against
    points_alignment_ref over ALL clouds with test_points_alignment_gpu._check_alignment's bars.  The C entries keep
    N < 65536; the operator boundary hands them contiguous slices of 65 535 clouds, so 65 536 and 65 537 clouds give
    what the same clouds give in smaller batches.  One cloud in eleven has an all-zero mask over rows that hold points:
    R = I and T = 0 by the definition (the first run returned T = Y[n,0] - X[n,0] R there: the pivots were counted
    although W had been clamped to eps; fixed in pa_solve)."""
    import points_alignment_ref as ref
    import test_points_alignment_gpu as ta

    knob(monkeypatch, None)
    from pytorch3d_pointops_amd.functions.points_alignment import corresponding_points_alignment as cpa

    X, Y, mask = memo(("align", N), lambda: _alignment_inputs(N))
    for estimate_scale, allow_reflection in ((False, False), (True, True)):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (tiny and empty clouds: the "cannot return a unique rotation" warnings)
            got = cpa(X.to(dev), Y.to(dev), mask.to(dev), estimate_scale, allow_reflection)
        want = ref.alignment(X, Y, mask, estimate_scale, allow_reflection)
        ok = ta._check_alignment(got, want, float(Y.abs().max()), allow_reflection, f"alignment N={N}")
        assert bool(ok[-1]) or int(mask[-1].sum()) < 4, "the last cloud is held to the accuracy bars"
        # the same bars per cloud, for the message: the first cloud that misses them
        R, T = got[0].double().cpu(), got[1].double().cpu()
        bad = ok & (((R - want[0]).abs().amax((1, 2)) > 1e-5)
                    | ((T - want[1]).abs().amax(1) > 1e-5 * (1 + float(Y.abs().max()))))
        assert not bool(bad.any()), mc.first_bad(bad.numpy())


def test_alignment_gradients_at_65537_clouds(dev, monkeypatch):
    """The autograd node over 65 537 full clouds with per-cloud weights: forward slices, float64 solves, the backward
    kernel in slices; test_points_alignment_gpu's gradient bar (1e-3 of the largest reference entry)."""
    import points_alignment_ref as ref
    import test_points_alignment_gpu as ta

    knob(monkeypatch, None)
    from pytorch3d_pointops_amd.functions.points_alignment import corresponding_points_alignment as cpa

    N = 65537
    X, Y, _ = memo(("align", N), lambda: _alignment_inputs(N))
    g = ta._gen(7800)
    w = 0.2 + torch.rand((N, 10), generator=g)
    gR, gT, gs = (torch.randn(sh, generator=g, dtype=torch.float64) for sh in ((N, 3, 3), (N, 3), (N,)))

    def loss(R_, T_, s_):
        d = R_.device
        return (R_ * gR.to(d, R_.dtype)).sum() + (T_ * gT.to(d, T_.dtype)).sum() + (s_ * gs.to(d, s_.dtype)).sum()

    leaves64 = [t.double().clone().requires_grad_(True) for t in (X, Y, w)]
    R64, T64, s64, S = ref.alignment(*leaves64, estimate_scale=True)
    assert bool(ref.well_determined(S).all())
    want = torch.autograd.grad(loss(R64, T64, s64), leaves64)
    leaves = [t.to(dev).clone().requires_grad_(True) for t in (X, Y, w)]
    got = torch.autograd.grad(loss(*cpa(*leaves, estimate_scale=True)), leaves)
    for name, u, v in zip("XYw", got, want):
        scale = float(v.abs().max())
        assert bool(torch.isfinite(u).all()) and scale > 0
        mc.assert_clouds_close(u.double().cpu().numpy(), v.numpy(), 1e-3 * scale, f"alignment grad {name}")


def test_icp_iteration_at_65535_clouds(dev, oracle, monkeypatch):
    """One fused ICP iteration on the largest batch it takes: the K = 1 search equals the oracle in every cloud; every
    cloud's transform is finite, a proper rotation to 1e-5 and OPTIMAL -- its float64 residual exceeds the checker's
    optimum by at most test_derived_edges_gpu's 16 u sum (|s x R|^2 + |y|^2) --; where the rotation is determined
    (test_points_alignment_gpu's rule, and sigma_1 > 0: a cloud whose queries all found the same target has C = 0, for
    which every rotation is optimal and the rule's 0 >= 0 says nothing) R, T, Xt and rmse meet that file's bars."""
    import points_alignment_ref as ref
    import test_derived_edges_gpu as de

    knob(monkeypatch, None)
    N = 65535
    b = mc.batch(N)
    X, Y = torch.from_numpy(b["p1"]), torch.from_numpy(b["p2"])
    lx, ly = torch.from_numpy(b["l1"]), torch.from_numpy(b["l2"])
    xd = X.to(dev)
    state = _C().IcpState(xd, xd.clone(), Y.to(dev), lx.to(dev), ly.to(dev), 1, False, False, 1e-6)
    state.step()
    want_idx = oracle_knn(oracle, N, 2, 1)[0][..., 0]
    mc.assert_clouds_equal(H(state.idx), want_idx, "icp: nearest neighbours")
    mask = ref.valid_mask(lx, 6).double()
    Ynn = ref.gather(Y.double(), torch.from_numpy(want_idx))
    R64, T64, s64, S = ref.alignment(X, Ynn, mask, False)
    ymax = float(Y.abs().max())
    Rg, Tg, sg = (t.double().cpu() for t in (state.R[0], state.T[0], state.s[0]))
    assert bool(torch.isfinite(Rg).all() and torch.isfinite(Tg).all() and torch.equal(sg, torch.ones_like(sg)))
    orth = (Rg.transpose(1, 2) @ Rg - torch.eye(3, dtype=torch.float64)).abs().amax((1, 2))
    bad = (orth > 1e-5) | ((torch.linalg.det(Rg) - 1).abs() > 1e-5)
    assert not bool(bad.any()), f"icp: not a proper rotation: {mc.first_bad(bad.numpy())}"
    got, size = de._residual(X.double(), Ynn, mask, Rg, Tg, sg)
    best, _ = de._residual(X.double(), Ynn, mask, R64, T64, s64)
    bad = (got - best) > 16 * de.U * size
    assert not bool(bad.any()), f"icp: transform not optimal: {mc.first_bad(bad.numpy())}"
    ok = ref.well_determined(S) & (S[:, 0] > 0)
    okn = ok.numpy()
    clouds = np.nonzero(okn)[0]
    assert okn.sum() > 1000 and okn[-8:].any(), "enough determined clouds, some at the tail"
    mc.assert_clouds_close(Rg.numpy()[okn], R64.numpy()[okn], 1e-5, "icp: R", clouds=clouds)
    mc.assert_clouds_close(Tg.numpy()[okn], T64.numpy()[okn], 1e-5 * (1 + ymax), "icp: T", clouds=clouds)
    Xt64 = (ref.apply(X, R64, T64, s64) * mask[..., None]).numpy()
    mc.assert_clouds_close(H(state.Xt)[okn], Xt64[okn], 1e-5 * (1 + ymax), "icp: Xt", clouds=clouds)
    assert not H(state.Xt)[~mask.bool().numpy()].any(), "rows past a length are zero"
    rmse64 = ((((torch.from_numpy(Xt64) - Ynn) ** 2).sum(2) * mask).sum(1) / lx.double().clamp(min=1e-9)).sqrt().numpy()
    mc.assert_clouds_close(H(state.rmse)[okn], rmse64[okn], 1e-5 * (1 + ymax), "icp: rmse", clouds=clouds)
    assert np.isfinite(H(state.rmse)).all() and np.isfinite(H(state.Xt)).all()
