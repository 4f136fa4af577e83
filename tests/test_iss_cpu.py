"""The checker of iss_keypoints (tests/iss_ref.py) against Open3D's algorithm restated in float64, and on hand-made
clouds whose keypoints are known.  No GPU: what the GPU tests compare the kernels to is held to its own definition here.

The bound on the eigenvalues: every quantized offset is off by at most half a quantum, 2^-20 * 2^e <= 2^-19 rs, so with
offsets of up to rs every entry of C is off by about 2 * rs * 2^-19 rs = 2^-18 rs^2 from the products and as much again
from the mean: 2^-17 rs^2; an eigenvalue moves by at most the 2-norm of the perturbation, which is at most 3 times its
largest entry: 3 * 2^-17 rs^2."""
import numpy as np
import pytest

import iss_ref as ref


def _frame(p, shift):
    return (p.astype(np.float64) + np.asarray(shift, np.float64)).astype(np.float32)


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (1000.0, -1000.0, 500.0)], ids=["unit-cube", "translated"])
@pytest.mark.parametrize("rs", [0.05, 0.08])
@pytest.mark.parametrize("P", [1000, 4096])
def test_integer_moments_stay_within_the_quantization_bound(P, rs, shift):
    p = _frame(ref.blobs_scene(70, P), shift)
    rn = 2.0 / 3.0 * rs
    got = ref.iss(p[None], None, rs, rn)
    eig64, sal64, mask64 = ref.iss_float64(p, rs, rn)
    lam = ref.eigenvalues64(got["C"][0])  # (before the rounding to float32, which is not what is bounded here)
    err = np.abs(lam - eig64).max()
    bound = 3.0 * 2.0 ** -17 * rs * rs
    same = int((got["mask"][0] == mask64).sum())
    print(f"P={P} rs={rs} shift={shift}: max |lambda - lambda64| = {err:.3e} = {err / (rs * rs):.3e} rs^2 "
          f"(bound {bound:.3e}); keypoints {int(got['mask'].sum())} vs {int(mask64.sum())} in float64, "
          f"{P - same} rows differ")  # (the masks are reported, not asserted: near-ties legitimately differ)
    assert err <= bound
    assert got["mask"].sum() > 0 and (got["saliency"] > 0).sum() > got["mask"].sum()
    if shift[0]:
        # coordinates near 2^10 are multiples of 2^-14, the quantum is 2^-23 or 2^-22: nothing is rounded, and what
        # is left is float64 rounding of coordinates of size 2^10 (2^-43 each), far below the bound
        s = ref.scale(rs)
        d = (p[:, None, :].astype(np.float64) - p[None, :64, :].astype(np.float64)) * s
        assert np.array_equal(d, np.rint(d))
        assert err <= 2.0 ** -30 * rs * rs


def test_scale_is_the_power_of_two_above_the_radius():
    for rs, e in ((1.0, 0), (0.5, -1), (0.05, -4), (0.08, -3), (1.0000001, 1), (0.99999994, 0), (3.0, 2), (1e-3, -9),
                  (1e-45, -149)):
        assert ref.scale(rs) == 2.0 ** (19 - e), rs


def test_single_point_and_pair():
    one = ref.iss(np.zeros((1, 1, 3), np.float32) + 0.25, None, 0.1, 0.1, min_neighbors=0)
    assert one["moments"][0, 0].tolist() == [1] + [0] * 9 and not one["eigenvalues"].any()
    assert not one["saliency"].any() and not one["mask"].any()
    pair = np.array([[[0.0, 0.0, 0.0], [0.03, 0.04, 0.0]]], np.float32)
    two = ref.iss(pair, None, 0.1, 0.1, min_neighbors=0)
    assert two["moments"][0, :, 0].tolist() == [2, 2]
    lam = two["eigenvalues"][0]
    assert np.allclose(lam[:, 2], 0.05 ** 2 / 4, rtol=1e-5) and (np.abs(lam[:, :2]) < 1e-9).all()  # a line: rank 1
    assert not two["saliency"].any() and not two["mask"].any()
    empty = ref.iss(pair, np.array([0]), 0.1, 0.1)
    assert not empty["moments"].any() and not empty["mask"].any() and empty["num_keypoints"].tolist() == [0]


def test_tilted_plane_has_nothing_salient():
    """The smallest eigenvalue of a plane is rounding: without the floor rule it would pass both ratio tests wherever it
    happens to be positive."""
    p = ref.tilted_plane()
    got = ref.iss(p[None], None, 0.08, 0.05, min_neighbors=0)
    lam = got["eigenvalues"][0]
    assert (lam[:, 1] > 1e-4).all() and (np.abs(lam[:, 0]) <= 2.0 ** -20 * lam[:, 2]).all()
    assert not got["saliency"].any() and not got["mask"].any()
    no_floor = (lam[:, 0] > 0) & (lam[:, 1] < np.float32(0.975) * lam[:, 2]) & (lam[:, 0] < np.float32(0.975) * lam[:, 1])
    print(f"rows the ratio tests alone would accept: {int(no_floor.sum())} of {len(p)}")


def test_cube_corner_is_a_keypoint():
    p = ref.cube_corner()
    assert p[0].tolist() == [0.0, 0.0, 0.0]
    got = ref.iss(p[None], None, 0.13, 0.11, min_neighbors=4)
    assert got["saliency"][0, 0] > 0 and got["moments"][0, 0, 0] == 6  # the corner, three edge and two face points
    assert np.flatnonzero(got["mask"][0]).tolist() == [0] and got["num_keypoints"].tolist() == [1]
    interior = (p > 0.15).sum(1) == 2  # face interiors: planes
    assert interior.any() and not got["saliency"][0, interior].any()
    eig64, sal64, mask64 = ref.iss_float64(p, 0.13, 0.11, min_neighbors=4)
    # (the float64 restatement has no floor rule: on the exact planes of the faces it keeps rounding noise, so only
    # the corner's own value is compared)
    assert abs(sal64[0] - got["saliency"][0, 0]) <= 3.0 * 2.0 ** -17 * 0.13 * 0.13 + 2.0 ** -23 * sal64[0]


def test_doubled_cloud_keeps_the_lower_index_of_every_maximal_pair():
    base = ref.blobs_scene(71, 500)
    P = len(base)
    rs, rn = 0.08, 0.05
    single = ref.iss(base[None], None, rs, rn, min_neighbors=2)
    both = ref.iss(ref.doubled(base)[None], None, rs, rn, min_neighbors=2)
    # a doubled support has the same mean and covariance: exactly, since every integer moment doubles with n
    assert np.array_equal(both["moments"][0, :P], 2 * single["moments"][0])
    assert np.array_equal(both["eigenvalues"][0, :P], both["eigenvalues"][0, P:])
    assert np.array_equal(both["saliency"][0, :P], both["saliency"][0, P:])
    mask = both["mask"][0]
    assert mask[:P].sum() > 0 and not mask[P:].any()  # exactly the lower index of each pair survives
    maximal = ref.nms(single["saliency"], base[None], None, rn, 1)[0]  # min_neighbors counts the twins: 2 -> 1
    assert np.array_equal(mask[:P], maximal)


def test_the_overflow_edge_in_python_integers():
    """n = 2^24 hits of |q| = 2^19: the largest second moment is 2^62, inside int64, and the covariance formula holds."""
    n, q = 2 ** 24, 2 ** 19
    m2 = n * q * q
    assert m2 == 2 ** 62 and m2 < 2 ** 63 and n * q < 2 ** 63
    mom = np.array([n, n * q, -n * q, 0, m2, -m2, 0, m2, 0, 0], np.int64)
    assert int(mom[4]) == m2
    C = ref.covariance(mom, 1.0)  # s = 2^19: every offset is one radius
    assert np.array_equal(C, np.zeros((3, 3)))  # all hits at one offset: no spread
    half = np.array([n, 0, 0, 0, m2, 0, 0, m2, 0, 0], np.int64)  # +-q in x and y, half each: mean 0
    assert np.array_equal(ref.covariance(half, 1.0), np.diag([1.0, 1.0, 0.0]))
