"""Every template instance of fps.hip at the sizes where its ownership pattern can go wrong, bit-equal to the oracle.

A lane of a B-lane workgroup owns the points tid, tid + B, ...; a cluster member m owns [m, m + 1) * PPT * 1024.  So the
sizes sit on both sides of every PPT bucket (B * 4, B * 8, B * 16) and of the member boundaries, the batches are ragged
(a full cloud, one of P - 1 points, one of a single point, and by turns an empty one, one with K = 0 and one with
K = 1), and cloud 0 carries blocks of duplicated points whose twins lie across a lane-stride or a member boundary:
points [B - 50, B + 50) copied onto [0, 100), the points around each member boundary onto the next hundred.  In cloud 0
the twins are pushed outwards so that the first samples come from them: every one of those samples is an exact tie
between an index below 251 and its twin, decided between lanes, waves or workgroups -- the lower index has to win.
(Checked with the oracle while writing: moving the lower twin of a chosen sample away makes the oracle return the
upper twin's index there, in every case of this file.)  Cloud 1 keeps its twins where they were, so its samples come
from all over the cloud.
"""
import functools

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

G = lambda a, dev: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731  (a copy: the cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def batch(D, P, block, members=()):
    """(points, lengths, K, start, twin blocks as (first, count)) -- never modified by a test."""
    pts = cases.cloud(7000 + 8 * P + D, (4, P, D))
    blocks = []
    for e in (block,) + tuple(members):
        lo, hi = (e - 50, min(e + 50, P)) if e < P else (P - 100, P)  # no such boundary in the cloud: its last points
        first = 100 * len(blocks)
        pts[0, lo:hi] = (pts[0, lo:hi] - np.float32(0.5)) * np.float32(3.0) + np.float32(0.5)
        pts[:, first:first + hi - lo] = pts[:, lo:hi].copy()
        blocks.append((first, hi - lo))
    tail = [(0, 3, 0), (40, 0, 39), (40, 1, 39)][(P + D) % 3]  # an empty cloud / K = 0 / K = 1
    lengths = np.array([P, P - 1, 1, tail[0]])
    K = np.array([48, 31, 5, tail[1]])  # (5: above the cloud's single point)
    start = np.array([7, P - 2, 0, tail[2]])
    for a in (pts, lengths, K, start):
        a.setflags(write=False)
    return pts, lengths, K, start, tuple(blocks)


@functools.lru_cache(maxsize=None)
def expected(oracle, key):
    pts, lengths, K, start, blocks = batch(*key)
    want = oracle.sample_farthest_points(pts, lengths, K, start)
    for first, count in blocks:  # the inputs do what the docstring says: a sample of cloud 0 out of every twin block
        assert np.isin(want[0, 1:], np.arange(first, first + count)).any(), (key, first)
    want.setflags(write=False)
    return want


def check(dev, oracle, monkeypatch, knob, key):
    from pytorch3d_pointops_amd import _C

    monkeypatch.setenv("POINTOPS_DEBUG", knob)
    pts, lengths, K, start, _ = batch(*key)
    got = _C.sample_farthest_points(G(pts, dev), G(lengths, dev), G(K, dev), G(start, dev)).cpu().numpy()
    assert np.array_equal(got, expected(oracle, key)), (key, knob)


@pytest.mark.parametrize("P", [255, 256, 257, 1024, 1025, 2048, 2049, 4096])
@pytest.mark.parametrize("D", [2, 3])
def test_single_256_lanes(dev, oracle, monkeypatch, D, P):
    """fps_single_kernel<D, 4 | 8 | 16, 256>: both edges of each bucket of points per lane."""
    check(dev, oracle, monkeypatch, "", (D, P, 256))


@pytest.mark.parametrize("P", [257, 1024, 1025, 4096])
@pytest.mark.parametrize("D", [2, 3])
def test_single_1024_lanes_lds_copy(dev, oracle, monkeypatch, D, P):
    """fps_single_kernel<D, 4, 1024>: the winner's coordinates from the LDS copy of the cloud."""
    check(dev, oracle, monkeypatch, "fps_small=0", (D, P, 1024))


@pytest.mark.parametrize("P,knob", [(4097, ""), (8192, ""), (8193, "fps_ppt=16"), (16384, "fps_ppt=16")])
@pytest.mark.parametrize("D", [2, 3])
def test_single_1024_lanes_global_winner(dev, oracle, monkeypatch, D, P, knob):
    """fps_single_kernel<D, 8 | 16, 1024>: the winner's coordinates from global memory."""
    check(dev, oracle, monkeypatch, knob, (D, P, 1024))


# (D, P, plan knob, member boundaries): G = 2 with eight points per lane, G = 3 with four, G = 2 with four
_EXCHANGES = [(2, 8193, "", (8192,)), (3, 8193, "", (4096, 8192)), (2, 4097, "fps_ppt=4", (4096,)), (3, 4097, "fps_ppt=4", (4096,))]


@pytest.mark.parametrize("how", ["fps_mode=0", "fps_mode=1", "fps_mode=2", "fps_spin_limit=0"])
@pytest.mark.parametrize("D,P,plan,members", _EXCHANGES)
def test_smallest_exchange(dev, oracle, monkeypatch, D, P, plan, members, how):
    """fps_cluster_kernel<D, 4 | 8> in every placement mode, and with every wait timing out at once: then the repair
    pass, fps_kernel<2 | 3> over the flagged clouds, produces the rows."""
    check(dev, oracle, monkeypatch, ",".join(k for k in (plan, how) if k), (D, P, 1024, members))


@pytest.mark.parametrize("P", [1023, 1025, 2049])
@pytest.mark.parametrize("D", [1, 4, 5])
def test_generic_dimension(dev, oracle, monkeypatch, D, P):
    """fps_kernel<0>: one, two and (2049) three strides of 1024 on some lanes."""
    check(dev, oracle, monkeypatch, "", (D, P, 1024))


@pytest.mark.parametrize("knob,key", [
    ("", (3, 2049, 256)),
    ("fps_small=0", (2, 1025, 1024)),
    ("fps_ppt=16", (3, 8193, 1024)),
    ("", (3, 8193, 1024, (4096, 8192))),
    ("fps_spin_limit=0", (2, 8193, 1024, (8192,))),
    ("", (5, 2049, 1024)),
])
def test_batch_equals_alone(dev, oracle, monkeypatch, knob, key):
    """Each cloud sampled by itself gives the row it got in the batch."""
    from pytorch3d_pointops_amd import _C

    monkeypatch.setenv("POINTOPS_DEBUG", knob)
    pts, lengths, K, start, _ = batch(*key)
    want = expected(oracle, key)
    for n in range(len(lengths)):
        one = [G(a[n:n + 1], dev) for a in (pts, lengths, K, start)]
        got = _C.sample_farthest_points(*one, max_K=want.shape[1]).cpu().numpy()
        assert np.array_equal(got[0], want[n]), (key, knob, n)
