"""Host logic of the default-`lengths` cache (functions/_common.full_lengths) that needs no GPU: one tensor object per
key and for both sides of a self-query, and nothing cached while a graph is traced.  Its behaviour across streams is
pinned on the GPU (tests/test_streams_devices_gpu.py, part B)."""
import torch

from pytorch3d_pointops_amd.functions import _common


def test_one_object_per_shape_and_for_a_self_query():
    saved = dict(_common._LENGTHS_CACHE)
    _common._LENGTHS_CACHE.clear()
    try:
        cpu = torch.device("cpu")
        t = _common.full_lengths(3, 11, cpu)
        assert t.dtype == torch.int64 and t.tolist() == [11, 11, 11]
        assert _common.full_lengths(3, 11, cpu) is t and _common.full_lengths(3, 12, cpu) is not t
        pts = torch.zeros((3, 11, 3))
        p1, p2, l1, l2 = _common.point_pair(pts, pts, None, None)
        assert p1 is p2 and l1 is l2 and l1 is t
        _, _, l1, l2 = _common.point_pair(pts, torch.zeros((3, 12, 3)), None, None)
        assert l1 is t and l2.tolist() == [12, 12, 12]
        for key in _common._LENGTHS_CACHE:  # (n, p, device index, stream): -1 and 0 off the GPU
            assert key[2:] == (-1, 0)
    finally:
        _common._LENGTHS_CACHE.clear()
        _common._LENGTHS_CACHE.update(saved)


def test_eviction_drops_everything_at_65_entries():
    saved = dict(_common._LENGTHS_CACHE)
    _common._LENGTHS_CACHE.clear()
    try:
        cpu = torch.device("cpu")
        first = _common.full_lengths(1, 1, cpu)
        for p in range(2, 66):
            _common.full_lengths(1, p, cpu)
        assert len(_common._LENGTHS_CACHE) == 65 and _common.full_lengths(1, 1, cpu) is first
        _common.full_lengths(1, 66, cpu)
        assert list(_common._LENGTHS_CACHE) == [(1, 66, -1, 0)]
        assert _common.full_lengths(1, 1, cpu) is not first and first.tolist() == [1]
    finally:
        _common._LENGTHS_CACHE.clear()
        _common._LENGTHS_CACHE.update(saved)


def test_a_traced_call_gets_a_tensor_of_its_graph_and_caches_nothing():
    saved = dict(_common._LENGTHS_CACHE)
    _common._LENGTHS_CACHE.clear()
    try:
        torch._dynamo.reset()
        fn = torch.compile(lambda x: x + _common.full_lengths(2, 7, x.device), backend="eager", fullgraph=True)
        assert fn(torch.zeros(2, dtype=torch.int64)).tolist() == [7, 7]
        assert not _common._LENGTHS_CACHE
    finally:
        _common._LENGTHS_CACHE.clear()
        _common._LENGTHS_CACHE.update(saved)
