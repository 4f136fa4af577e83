"""CPU proof of the exact-frame expectations (tests/frames.py) for the REFERENCE semantics themselves: the oracle --
and the reference's own compiled CPU kernels where oracle/_ref holds them -- run on a base case and on its shifted,
negated and 2^k-scaled images must give identical indices and distances / gradients that differ by the exact factor.
With that established here, a failure of tests/test_coordinate_frames_gpu.py can only be the kernel's.

One narrowing, found by running this file: a gradient entry that is exactly zero (a neighbour coinciding with its
query: a - b = +0 in either frame) keeps its +0 under a negation instead of turning into -0, so gradients are compared
bit for bit after adding +0.0 (which maps -0 to +0 and changes nothing else).  Distances need no such rule."""
import numpy as np
import pytest

import cases
import frames
from conftest import bits


@pytest.fixture(params=["port", "reference"])
def ora(request, oracle):
    """The plain-C oracle, and the reference's own compiled CPU kernels (oracle/_ref, built by build() where the
    reference tree is present): the test IDs show which one took part."""
    if request.param == "port":
        return oracle
    from oracle.oracle import load_ref

    ref = load_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


def bits0(a):
    return bits(np.asarray(a, np.float32) + np.float32(0.0))


KNN = ["ragged_k8", "ties_lattice_k16", "l1_k4", "l1_ties_k3"]  # uniform / lattice, L2 / L1
BALL = ["ragged_r0.2", "boundary_lattice"]
FPS = ["per_cloud_k", "lattice_ties"]
BWD = ["ragged_k8", "ties_lattice_k16", "l1_k4"]


def _exact(name):
    return frames.frames_for(lattice="lattice" in name, inexact=False)


def _ids(pairs):
    return [f"{n}-{f.name}" for n, f in pairs]


_KNN_P = [(n, f) for n in KNN for f in _exact(n)]
_BALL_P = [(n, f) for n in BALL for f in _exact(n)]
_FPS_P = [(n, f) for n in FPS for f in _exact(n)]
_BWD_P = [(n, f) for n in BWD for f in _exact(n)]


@pytest.mark.parametrize("name,frame", _KNN_P, ids=_ids(_KNN_P))
def test_knn_reference_semantics_in_exact_frames(ora, name, frame):
    c = cases.knn_cases()[name]
    q1, q2 = frame.apply(c["p1"], c["p2"])
    for o in (ora,):
        bi, bd = o.knn_points_idx(c["p1"], c["p2"], c["l1"], c["l2"], c["norm"], c["K"])
        fi, fd = o.knn_points_idx(q1, q2, c["l1"], c["l2"], c["norm"], c["K"])
        assert np.array_equal(fi, bi), (o.kind, name, frame)
        assert np.array_equal(bits(fd), bits(bd * frame.dist_factor(c["norm"]))), (o.kind, name, frame)


@pytest.mark.parametrize("name,frame", _BALL_P, ids=_ids(_BALL_P))
def test_ball_query_reference_semantics_in_exact_frames(ora, name, frame):
    c = cases.ball_query_cases()[name]
    q1, q2 = frame.apply(c["p1"], c["p2"])
    for o in (ora,):
        bi, bd = o.ball_query(c["p1"], c["p2"], c["l1"], c["l2"], c["K"], c["radius"])
        fi, fd = o.ball_query(q1, q2, c["l1"], c["l2"], c["K"], frame.radius(c["radius"]))
        assert np.array_equal(fi, bi), (o.kind, name, frame)
        assert np.array_equal(bits(fd), bits(bd * frame.dist_factor(2))), (o.kind, name, frame)
    if name == "boundary_lattice":  # the case is about distances exactly ON radius^2: they stay out in every frame
        on = ((c["p1"][0, :, None, :] - c["p2"][0, None, :, :]) ** 2).sum(-1) == np.float32(c["radius"]) ** 2
        assert on.any()


@pytest.mark.parametrize("name,frame", _FPS_P, ids=_ids(_FPS_P))
def test_fps_reference_semantics_in_exact_frames(ora, name, frame):
    c = cases.fps_cases()[name]
    q, _ = frame.apply(c["points"])
    for o in (ora,):
        base = o.sample_farthest_points(c["points"], c["lengths"], c["K"], c["start"])
        got = o.sample_farthest_points(q, c["lengths"], c["K"], c["start"])
        assert np.array_equal(got, base), (o.kind, name, frame)


@pytest.mark.parametrize("name,frame", _BWD_P, ids=_ids(_BWD_P))
def test_knn_backward_reference_semantics_in_exact_frames(ora, name, frame):
    c = cases.knn_backward_cases()[name]
    D = c["p1"].shape[2]
    q1, q2 = frame.apply(c["p1"], c["p2"])
    for o in (ora,):
        idx, _ = o.knn_points_idx(c["p1"], c["p2"], c["l1"], c["l2"], c["norm"], c["K"])
        grad = cases.grad_for(name, idx.shape)
        b1, b2 = o.knn_points_backward(c["p1"], c["p2"], c["l1"], c["l2"], idx, c["norm"], grad)
        f1, f2 = o.knn_points_backward(q1, q2, c["l1"], c["l2"], idx, c["norm"], grad)
        fac = frame.grad_factor(c["norm"], D)
        assert np.array_equal(bits0(f1), bits0(b1 * fac)), (o.kind, name, frame)
        assert np.array_equal(bits0(f2), bits0(b2 * fac)), (o.kind, name, frame)


# ---------------------------------------------------------------------------------------------- the helpers
def test_shift_helper_rejects_clouds_off_the_grid():
    u = cases.cloud(7001, (1, 500, 3))
    assert frames.quantum(u) >= 2.0 ** -24  # uniform_f32: multiples of 2^-24 in [0, 1)
    frames.shift_exact(u, -0.5), frames.shift_exact(u, -1.0)
    off = (u ** np.float32(6.0)).astype(np.float32)  # small values carry bits far below 2^-24
    with pytest.raises(ValueError, match="not exact"):
        frames.shift_exact(off, -1.0)
    frames.shift_exact(frames.quantise(off, 20), -1.0)
    lt = cases.lattice(7002, 1, 100)
    for t in (float(2 ** 20), -float(2 ** 20 - 3)):
        y = frames.shift_exact(lt, t)
        assert np.array_equal((y.astype(np.float64) - t).astype(np.float32), lt)
    with pytest.raises(ValueError, match="not exact"):
        frames.shift_exact(u, float(2 ** 20))  # 24-bit fractions do not survive next to 2^20


def test_scale_helper_rejects_exponents_that_leave_the_normal_range():
    u = cases.cloud(7003, (1, 500, 3))
    for k in (-30, 40, 60):
        frames.scale_exact([u], k)
    with pytest.raises(ValueError, match="normal range"):
        frames.scale_exact([u], -60)  # 4^-60 2^-48 = 2^-168 < FLT_MIN
    with pytest.raises(ValueError, match="overflow"):
        frames.scale_exact([u], 64)
    lt = cases.lattice(7004, 1, 100)
    frames.scale_exact([lt], -60)  # quantum 0.25: squares stay normal
    assert frames.quantum(lt) == 0.25 and frames.quantum(np.zeros((1, 4, 3), np.float32)) == 1.0


def test_negation_keeps_negative_zero_and_frames_are_finite():
    lt = cases.lattice(7005, 1, 100)
    q, _ = frames.BY_NAME["neg_all"].apply(lt)
    assert (lt == 0).any() and np.array_equal(np.signbit(q), np.ones(q.shape, bool))  # 0.0 -> -0.0, kept
    q, _ = frames.BY_NAME["shift-1.0"].apply(cases.lattice(7005, 1, 100, levels=6))  # levels 0 .. 1.25
    assert (q == 0).any() and (q < 0).any() and (q > 0).any()  # mostly negative, crossing zero at one level
    u1, u2 = cases.cloud(7006, (2, 300, 3)), cases.cloud(7007, (2, 200, 3))
    for f in frames.INEXACT:
        a, b = f.apply(u1, u2)
        assert a.dtype == np.float32 and a.shape == u1.shape and b.shape == u2.shape
        if not f.needs_pair:
            s, s2 = f.apply(u2, u2)
            assert s is s2
    a, b = frames.BY_NAME["mag1e-18"].apply(u1, u2)
    sq = ((a[0, :, None, :] - b[0, None, :, :]) ** 2).astype(np.float32)  # per-axis terms of every pair
    assert (sq == 0).any() and ((sq > 0) & (sq < frames.FLT_MIN)).any()  # exact zeros and subnormals, not flushed
    a, b = frames.BY_NAME["opposite_signs"].apply(u1, u2)
    assert (a < 0).all() and (b > 0).all()
