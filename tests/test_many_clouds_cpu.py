"""CPU half of the many-clouds tests: what tests/many_clouds_cases.py promises is ASSERTED here, the reference is shown
to have no batch limit (the oracle equals its compiled CPU kernels on 65 537 clouds), and every numpy / float64
restatement the GPU half leans on is shown to take such a batch (whole, or on the probe set)."""
import numpy as np
import pytest
import torch

import many_clouds_cases as mc
from conftest import bits
from pytorch3d_pointops_amd import synth

N3 = 65537  # three slices of 32 768, one cloud past blockIdx.y


# ------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("N", mc.ALL_NS + (mc.N_BIG,))
def test_clouds_are_separated_from_their_aliases(N):
    """Cloud n differs from cloud n - 32768 and n - 65536 in length AND in every point row, on both sides; empty and
    full clouds occur; the last cloud has rows; K = 4 exceeds some targets.  A launch that serves cloud n as
    n mod 32768 or n mod 65536, or that never writes the tail, cannot produce this batch's expected output."""
    b = mc.batch(N)
    for side, P in (("1", 6), ("2", 10)):
        p, l = b["p" + side], b["l" + side]
        assert p.shape == (N, P, 3) and l.shape == (N,) and l.dtype == np.int64
        assert l.min() == 0 and l.max() == P, "empty and full clouds"
        assert l[-1] > 0, "the last cloud is non-empty"
        for shift in (mc.SLICE, mc.GRID_Y):
            if N > shift:
                assert (l[shift:] != l[:-shift]).all(), (side, shift, mc.first_bad(l[shift:] == l[:-shift]))
                rows_differ = (p[shift:] != p[:-shift]).any(-1)  # (N - shift, P)
                assert rows_differ.all(), (side, shift, mc.first_bad(~rows_differ))
    assert (b["l2"] < 4).any() and (b["l2"] >= 4).any(), "some clouds have fewer targets than K = 4"
    lattice = b["p2"][::5]
    assert np.array_equal(lattice, np.round(lattice * 4) / 4), "every 5th cloud is on the 0.25 lattice"
    assert not np.array_equal(b["p2"][1], np.round(b["p2"][1] * 4) / 4)


def test_batches_are_prefixes_of_each_other():
    """The same cloud index has the same content whatever N (except the repaired last length), so a failure at one N
    can be looked at in a smaller batch."""
    a, b = mc.batch(32769), mc.batch(N3)
    assert np.array_equal(a["p1"], b["p1"][:32769]) and np.array_equal(a["p2"], b["p2"][:32769])
    assert np.array_equal(a["l1"][:-1], b["l1"][:32768]) and np.array_equal(a["l2"][:-1], b["l2"][:32768])


def test_probe_set_covers_the_edges():
    for N in mc.ALL_NS + (mc.N_BIG,):
        pr = mc.probe_set(N)
        assert pr.min() == 0 and pr.max() == N - 1 and len(np.unique(pr)) == len(pr) <= 8 + 16 + 17 + 8 + 64
        for n in list(range(8)) + list(range(N - 8, N)) + [m for m in range(32760, 32776) if m < N] \
                + [m for m in range(65527, 65544) if m < N]:
            assert n in pr
        assert len(pr) >= 64


def test_first_bad_reports_the_residues():
    bad = np.zeros((N3, 2), bool)
    assert mc.first_bad(bad) == ""
    bad[65536, 1] = bad[70, 0] = True
    bad[70, 0] = False
    assert "n = 65536 (n % 32768 = 0, n % 65536 = 0)" in mc.first_bad(bad)
    with pytest.raises(AssertionError, match="n = 65536"):
        mc.assert_clouds_equal(bad, np.zeros_like(bad), "demo")


# ------------------------------------------------------------------------------------------ the reference has no limit
@pytest.fixture(scope="module")
def ref():
    from oracle.oracle import load_ref

    r = load_ref()
    if r is None:
        pytest.skip("oracle/_ref not built")
    return r


def test_reference_kernels_take_65537_clouds(oracle, ref):
    """knn_points_idx, ball_query, sample_farthest_points, packed_to_padded, padded_to_packed: the oracle is bit-equal
    to the reference's compiled CPU kernels on a 65 537-cloud batch -- the reference has no batch limit, and the oracle
    is a valid yardstick at this N."""
    b = mc.batch(N3)
    p1, p2, l1, l2 = b["p1"], b["p2"], b["l1"], b["l2"]
    for norm, K in ((2, 4), (1, 8)):
        oi, od = oracle.knn_points_idx(p1, p2, l1, l2, norm, K)
        ri, rd = ref.knn_points_idx(p1, p2, l1, l2, norm, K)
        mc.assert_clouds_equal(oi, ri, f"knn idx L{norm} K{K}")
        mc.assert_clouds_equal(od, rd, f"knn dists L{norm} K{K}", as_bits=True)
    oi, od = oracle.ball_query(p1, p2, l1, l2, 4, 0.5)
    ri, rd = ref.ball_query(p1, p2, l1, l2, 4, 0.5)
    mc.assert_clouds_equal(oi, ri, "ball_query idx")
    mc.assert_clouds_equal(od, rd, "ball_query dists", as_bits=True)
    # (an empty cloud is undefined behaviour in the reference's FPS -- it marks point 0 of an empty vector --, and the
    # oracle defines it as a row of -1: the comparison gives every cloud at least one point)
    lf = np.maximum(l2, 1)
    Ks, start = mc.fps_k(N3, 10), mc.fps_start(lf)
    mc.assert_clouds_equal(oracle.sample_farthest_points(p2, lf, Ks, start),
                           ref.sample_farthest_points(p2, lf, Ks, start), "sample_farthest_points")
    x, first, F = mc.packed_of(b["p2"], l2)
    op, rp = oracle.packed_to_padded(x, first, 10), ref.packed_to_padded(x, first, 10)
    mc.assert_clouds_equal(op, rp, "packed_to_padded", as_bits=True)
    assert np.array_equal(bits(oracle.padded_to_packed(op, first, F)), bits(ref.padded_to_packed(rp, first, F)))
    assert np.array_equal(bits(oracle.padded_to_packed(op, first, F)), bits(x))


# ------------------------------------------------------------------------------------------ restatements take the batch
def test_packed_padded_restatement_matches_oracle(oracle):
    """The numpy restatement the GPU test uses against the oracle on 65 537 clouds: a dense layout, and one with packed
    rows owned by no cloud (gapped_first_idxs: clouds whose range is one row longer than max_size lets them take)."""
    b = mc.batch(N3)
    x, first, F = mc.packed_of(b["p2"], b["l2"])
    padded = mc.packed_to_padded_np(x, first, 10)
    assert np.array_equal(bits(padded), bits(oracle.packed_to_padded(x, first, 10)))
    assert np.array_equal(padded, np.where((np.arange(10)[None, :] < b["l2"][:, None])[..., None], b["p2"], 0))
    assert np.array_equal(bits(mc.padded_to_packed_np(padded, first, F)), bits(x))
    l = np.where(np.arange(N3) % 3 == 0, 10, b["l2"])  # the gapped clouds are full: their extra row is beyond max_size
    first, F = mc.gapped_first_idxs(l)
    x = (synth.uniform_f32(55, (F, 3)) + np.float32(0.5)).astype(np.float32)
    padded = mc.packed_to_padded_np(x, first, 10)
    assert np.array_equal(bits(padded), bits(oracle.packed_to_padded(x, first, 10)))
    back = mc.padded_to_packed_np(padded, first, F)
    assert np.array_equal(bits(back), bits(oracle.padded_to_packed(padded, first, F)))
    ownerless = np.ones(F, bool)
    ownerless[(first[:, None] + np.arange(10)[None, :])[np.arange(10)[None, :] < l[:, None]]] = False
    assert ownerless.sum() == 1 + (N3 + 2) // 3 and not back[ownerless].any() and x[ownerless].any()


def test_derived_refs_take_the_batch():
    """cov_fp32 / cov_backward_fp32 are vectorised over rows: whole batch.  gather_neighbourhoods and the alignment
    moments loop per cloud: the probe set is what they are given on the GPU side."""
    import derived_ref as dr

    b = mc.batch(N3)
    knn = np.ascontiguousarray(np.broadcast_to(b["p2"][:, :, None, :], (N3, 10, 5, 3)) * np.float32(0.5))
    knn = knn + b["p2"][:, :5][:, None, :, :]
    cov = dr.cov_fp32(knn)
    assert cov.shape == (N3, 10, 3, 3) and cov.dtype == np.float32
    assert np.abs(cov - dr.cov_f64(knn)).max() < 1e-5
    g = dr.cov_backward_fp32(knn, cov)
    assert g.shape == knn.shape and np.abs(g - dr.cov_backward_f64(knn, cov)).max() < 1e-4
    pr = mc.probe_set(N3)
    mom, mabs, rows = dr.alignment_moments_f64(b["p2"][pr], b["p2"][pr][:, ::-1], None, b["l2"][pr], None)
    assert mom.shape == (len(pr), 3 + 12 + 9) and np.array_equal(rows, b["l2"][pr])


def test_chamfer_ref_takes_the_batch(oracle):
    from chamfer_ref import CachedKnn, chamfer_distance_ref

    b = mc.batch(N3)
    r = chamfer_distance_ref(CachedKnn(oracle), b["p1"], b["p2"], b["l1"], b["l2"], batch_reduction=None)
    (tag, loss), = r["outputs"]
    assert loss.shape == (N3,) and np.isfinite(loss).all() and r["grad_x"].shape == b["p1"].shape
    empty = (b["l1"] == 0) & (b["l2"] == 0)
    assert empty.any() and (loss[empty] == 0).all()
    assert (loss[(b["l1"] > 0) & (b["l2"] > 0) & (np.arange(N3) % 5 != 0)] > 0).all()


def test_scatter_ref_takes_the_batch():
    p1, p2, l1, l2, idx, grad, ref = mc.exact_knn_backward_inputs(N3, 3)
    assert ref.g1.shape == (N3, 6, 3) and ref.g2.shape == (N3, 10, 3)
    assert max(ref.A1.max(), ref.A2.max()) < 2.0 ** 22
    last = N3 - 1
    assert ref.n1[last].any() and ref.n2[last].any(), "the last cloud receives gradient"
    go, idx, lengths, gref = mc.exact_gather_backward_inputs(N3, 3)
    assert gref.gx.shape == (N3, 10, 3) and gref.n[last].any()


def test_fpfh_and_alignment_refs_take_the_batch():
    import fpfh_ref
    import points_alignment_ref as par

    b = mc.batch(65535)
    R, T, s, S = par.alignment(torch.from_numpy(b["p2"]), torch.from_numpy(b["p2"][:, ::-1].copy()),
                               par.valid_mask(b["l2"], 10).double(), estimate_scale=True)
    assert R.shape == (65535, 3, 3) and torch.isfinite(R).all() and torch.isfinite(T).all()
    pr = mc.probe_set(65535)
    idx = np.broadcast_to(np.arange(8)[None, None, :], (len(pr), 10, 8)).copy()
    f = fpfh_ref.pair_features(b["p2"][pr], b["p2"][pr][:, ::-1], idx, b["l2"][pr], np.float32)
    assert f["f"].shape == (len(pr), 10, 8, 4)
