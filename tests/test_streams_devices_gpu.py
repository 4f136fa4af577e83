"""Every operator on side streams and on a device that is not the current one (the table: tests/streams_cases.py).

The other GPU tests run on the default stream of cuda:0, where a launch that lands on the wrong stream or device still
gives right answers.  Here the inputs of a call are NOT READY when it is made:

    the buffers hold decoy data (a cloud of another seed); on a side stream `s` a delay is enqueued, then a
    device-to-device copy of the real data into the same buffers, an event `ready`, and -- still under
    torch.cuda.stream(s) -- the call.  A kernel the package launches on any other stream reads the decoy (or a
    workspace that is not written yet) and the comparison with the expected value fails.

A test proves its own power: right after the Python call returns it asserts `not ready.query()` -- had the delay ended
by then, every stream would have seen the real data and the run would have proved nothing.  (Operators that read back
from the device by design -- ICP's convergence flag, FPS with a tensor K, the warnings of
corresponding_points_alignment -- synchronise `s` themselves: values only, said at their table entries; their stepping
primitives / native entries are in the table without a read.)  Before that, one call on the default stream pays the
first-launch costs (and supplies the expected value of the bit-reproducible operators) and one call on `s` with the
decoy data fills the caching allocator's pool of `s`.

Sizing of the delay.  Measured on an MI355X, the host side of one call enqueued behind the delay (every test prints
its own): 0.02 - 0.07 ms for the searches, FPS and the small operators, 0.10 - 0.13 ms for normals, knn_gather and three
ICP steps, 0.17 - 0.30 ms for forward + backward of knn_points and chamfer_distance; the slowest entry, the overlap
chamfer, took 0.30 ms (HOST_ENQUEUE_MS).  The delay is DELAY_MS = 40 ms for every call made behind it (two calls on
two streams: 80 ms on each): 130 times the slowest enqueue, where 20 times would cover the jitter of a shared host.
The three entries that read back from the device return after 40.1 - 40.3 ms: they wait for the delay, as expected.

Parts: A every entry behind a delay; B the default-`lengths` cache across two streams and across its eviction;
C two streams at once; D all tensors on cuda:1 while cuda:0 is current (skipped with fewer than two devices).
"""
import time

import numpy as np
import pytest
import torch

import streams_cases as sc

pytestmark = pytest.mark.gpu

HOST_ENQUEUE_MS = 0.30  # the slowest entry's call (chamfer_overlap, forward + backward), as measured
DELAY_MS = 40.0  # per call enqueued behind the delay
assert DELAY_MS >= 20 * HOST_ENQUEUE_MS

NAMES = sorted(sc.TABLE)
_CYCLES_PER_MS, _STREAMS, _BASE = {}, {}, {}


def _delay(device, ms):
    """Enqueue `ms` milliseconds of spinning on the current stream of `device` (torch.cuda._sleep counts device clock
    ticks: their rate is measured once per device)."""
    i = device.index
    if i not in _CYCLES_PER_MS:
        with torch.cuda.device(i):
            torch.cuda._sleep(1_000_000)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(20_000_000)
            b.record()
            b.synchronize()
            _CYCLES_PER_MS[i] = 20_000_000 / a.elapsed_time(b)
    with torch.cuda.device(i):
        torch.cuda._sleep(int(ms * _CYCLES_PER_MS[i]))


def _streams(device):
    """Two side streams per device, shared by all tests: their allocator pools stay warm."""
    if device.index not in _STREAMS:
        _STREAMS[device.index] = (torch.cuda.Stream(device), torch.cuda.Stream(device))
    return _STREAMS[device.index]


def _numpy(outs):
    return tuple(o.detach().cpu().numpy() for o in outs)


def _call(entry, data, static):
    with entry.knobs():
        return tuple(entry.run({**data, **static}))


def _base(entry, k, oracle):
    """Result of data set k on the default stream of cuda:0 (once): the expected value of a bit-reproducible entry."""
    if (entry.name, k) not in _BASE:
        data, static = entry.tensors(k, oracle, torch.device("cuda:0"))
        _BASE[entry.name, k] = _numpy(_call(entry, data, static))
    return _BASE[entry.name, k]


def _assert_matches(entry, k, oracle, outs, what):
    want = entry.expected(k, oracle)
    if want is None:
        want = _base(entry, k, oracle)
    got = _numpy(outs)
    assert len(got) == len(want) == len(entry.kinds)
    for j, (g, w, kind) in enumerate(zip(got, want, entry.kinds)):
        bad = sc.same(g, w, kind)
        assert bad is None, f"{entry.name} {what}: output {j} ({kind}): {bad}"


class _Job:
    """One entry on one stream: default-stream call, decoy buffers, warm call on the stream; then `enqueue` (delay, copy
    of the real data, event, call) and `finish` (synchronise, compare)."""

    def __init__(self, entry, k, stream, oracle, on_outputs=None):
        self.entry, self.k, self.stream, self.oracle = entry, k, stream, oracle
        device = stream.device
        self.real, self.static = entry.tensors(k, oracle, device)
        first = _call(entry, self.real, self.static)  # default stream of `device`, whatever the current device is
        if on_outputs is not None:
            on_outputs(first)
        _assert_matches(entry, k, oracle, first, f"on the default stream of {device}")
        if entry.prove is not None:
            with entry.knobs():
                entry.prove({**self.real, **self.static})
        self.bufs = entry.tensors(1, oracle, device)[0]  # the decoy
        with torch.cuda.stream(stream):
            _call(entry, self.bufs, self.static)
        torch.cuda.synchronize(device)

    def enqueue(self, delay_ms):
        with torch.cuda.stream(self.stream):
            _delay(self.stream.device, delay_ms)
            with torch.no_grad():
                for name, buf in self.bufs.items():
                    buf.copy_(self.real[name])
            self.ready = torch.cuda.Event()
            self.ready.record(self.stream)
            t0 = time.perf_counter()
            self.outs = _call(self.entry, self.bufs, self.static)
            self.host_ms = (time.perf_counter() - t0) * 1e3

    def finish(self):
        self.stream.synchronize()
        _assert_matches(self.entry, self.k, self.oracle, self.outs, f"on a side stream of {self.stream.device}")


def _run_behind_delays(jobs):
    for job in jobs:
        job.enqueue(DELAY_MS * len(jobs))
    still = [not job.ready.query() for job in jobs]  # (after the LAST call returned: all delays still running)
    for job in jobs:
        print(f"{job.entry.name}: host enqueue {job.host_ms:.3f} ms behind a delay of {DELAY_MS * len(jobs):.0f} ms")
    for job, ok in zip(jobs, still):
        if job.entry.syncs is None:
            assert ok, (f"{job.entry.name}: the delay on its stream had ended when the calls returned (host enqueue "
                        f"{job.host_ms:.3f} ms): the inputs were ready, this run proved nothing")
    for job in jobs:
        job.finish()


# ------------------------------------------------------------------------------------------------- A. one side stream
@pytest.mark.parametrize("name", NAMES)
def test_side_stream_with_inputs_not_ready(dev, oracle, name):
    _run_behind_delays([_Job(sc.TABLE[name], 0, _streams(dev)[0], oracle)])


# ------------------------------------------------------------------------------- B. the default-lengths cache
def _knn8(x, y):
    from pytorch3d_pointops_amd.functions import knn_points

    r = knn_points(x, y, K=8)
    return r.idx, r.dists


def _ball8(x, y):
    from pytorch3d_pointops_amd.functions import ball_query

    r = ball_query(x, y, K=8, radius=0.2, return_nn=False)
    return r.idx, r.dists


def _fps8(x, y):
    from pytorch3d_pointops_amd.functions import sample_farthest_points

    return sample_farthest_points(x, K=8)


def _chamfer(x, y):
    from pytorch3d_pointops_amd.functions.chamfer import chamfer_distance

    return (chamfer_distance(x, y)[0],)


def _full_lengths(t):
    return torch.full((t.shape[0],), t.shape[1], dtype=torch.int64, device=t.device)


def _explicit(op, x, y):
    """The same operator with explicit full lengths: warms the kernels up and leaves the cache alone."""
    from pytorch3d_pointops_amd import functions
    from pytorch3d_pointops_amd.functions.chamfer import chamfer_distance

    lx, ly = _full_lengths(x), _full_lengths(y)
    if op == "knn":
        functions.knn_points(x, y, lx, ly, K=8)
    elif op == "ball":
        functions.ball_query(x, y, lx, ly, K=8, radius=0.2, return_nn=False)
    elif op == "fps":
        functions.sample_farthest_points(x, lx, K=8)
    else:
        chamfer_distance(x, y, x_lengths=lx, y_lengths=ly)


def _expected_default_lengths(op, oracle, x, y):
    n = x.shape[0]
    lx, ly = np.full((n,), x.shape[1], np.int64), np.full((n,), y.shape[1], np.int64)
    if op == "knn":
        return oracle.knn_points_idx(x, y, lx, ly, 2, 8), ("bits", "bits")
    if op == "ball":
        return oracle.ball_query(x, y, lx, ly, 8, 0.2), ("bits", "bits")
    if op == "fps":
        idx = oracle.sample_farthest_points(x, lx, np.full((n,), 8, np.int64), np.zeros((n,), np.int64))
        return (sc.oracle_module.masked_gather(x, idx), idx), ("bits", "bits")
    return sc._chamfer_expect(oracle, dict(x=x, y=y))[:1], ("loss",)


_CACHE_OPS = {"knn": _knn8, "ball": _ball8, "fps": _fps8, "chamfer": _chamfer}
# (n, p1, p2) no other test uses: the entries of these tests are made by these tests
_CACHE_SHAPES = {"knn": (3, 777, 913), "ball": (3, 779, 911), "fps": (3, 781, 781), "chamfer": (3, 783, 907)}


def _cache_clouds(op, dev, seed):
    n, p1, p2 = _CACHE_SHAPES[op]
    x, y = sc.cases.cloud(seed, (n, p1, 3)), sc.cases.cloud(seed + 1, (n, p2, 3))
    return x, y, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


def _zeroed_free_blocks(stream, n):
    """Leave freed int64 blocks of n zeros in the allocator pools of the default stream and of `stream`: a default
    lengths tensor allocated next most likely reuses one, so that reading it before its fill gives lengths 0 (an
    all-padding result) rather than whatever the pool held.  Likely, not certain: nothing asserts it."""
    for s in (torch.cuda.current_stream(stream.device), stream):
        with torch.cuda.stream(s):
            junk = [torch.zeros((n,), dtype=torch.int64, device=stream.device) for _ in range(64)]
            del junk
    torch.cuda.synchronize(stream.device)


def _check_default_lengths(op, oracle, x, y, outs, what):
    want, kinds = _expected_default_lengths(op, oracle, x, y)
    for j, (g, w, kind) in enumerate(zip(_numpy(outs), want, kinds)):
        bad = sc.same(g, np.asarray(w), kind)
        assert bad is None, f"{op} with default lengths {what}: output {j}: {bad}"


@pytest.mark.parametrize("op", sorted(_CACHE_OPS))
def test_default_lengths_first_used_on_two_streams_at_once(dev, oracle, op):
    """The first call with `lengths=None` of a shape sits behind a delay on stream a -- and with it the fill of the
    lengths tensor it makes; the same call on stream b, made at once, must not read a tensor that is not filled yet."""
    from pytorch3d_pointops_amd.functions import _common

    a, b = _streams(dev)
    xa, ya, txa, tya = _cache_clouds(op, dev, 6100)
    xb, yb, txb, tyb = _cache_clouds(op, dev, 6200)
    _common._LENGTHS_CACHE.clear()
    try:
        for s in (torch.cuda.current_stream(dev), a, b):
            with torch.cuda.stream(s):
                _explicit(op, txa, tya)
        assert not _common._LENGTHS_CACHE
        _zeroed_free_blocks(a, txa.shape[0])
        with torch.cuda.stream(a):
            _delay(dev, DELAY_MS * 2)
            delay_over = torch.cuda.Event()
            delay_over.record(a)
            out_a = _CACHE_OPS[op](txa, tya)
        with torch.cuda.stream(b):
            out_b = _CACHE_OPS[op](txb, tyb)
        assert not delay_over.query(), "the delay on stream a had ended when the calls returned: it proved nothing"
        a.synchronize()
        b.synchronize()
        _check_default_lengths(op, oracle, xb, yb, out_b, "on stream b while the first use waits on stream a")
        _check_default_lengths(op, oracle, xa, ya, out_a, "behind the delay on stream a")
    finally:
        torch.cuda.synchronize(dev)
        _common._LENGTHS_CACHE.clear()


def test_default_lengths_evicted_while_another_stream_reads_them(dev, oracle):
    """The cache drops its entries (65 of them) while a call with default lengths waits behind a delay on stream b; a
    same-sized tensor is then allocated and filled on stream a, where this shape's default lengths were first used: the
    waiting call must still read ITS lengths."""
    from pytorch3d_pointops_amd.functions import _common, knn_points

    a, b = _streams(dev)
    n, p1, p2 = 3, 787, 903
    x, y = sc.cases.cloud(6301, (n, p1, 3)), sc.cases.cloud(6302, (n, p2, 3))
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    tiny = torch.from_numpy(sc.cases.cloud(6303, (1, 5, 3))).to(dev)
    _common._LENGTHS_CACHE.clear()
    try:
        for s in (a, b):
            with torch.cuda.stream(s):
                _explicit("knn", tx, ty)
                knn_points(tiny, tiny, _full_lengths(tiny), _full_lengths(tiny), K=1)
        with torch.cuda.stream(a):
            first = _knn8(tx, ty)  # first use of the shape: on stream a
        torch.cuda.synchronize(dev)
        _check_default_lengths("knn", oracle, x, y, first, "at first use")
        with torch.cuda.stream(b):
            _delay(dev, DELAY_MS * 2)
            delay_over = torch.cuda.Event()
            delay_over.record(b)
            out_b = _knn8(tx, ty)
        real = set(_common._LENGTHS_CACHE)
        for i in range(65):
            _common._LENGTHS_CACHE[("filler", i)] = None
        with torch.cuda.stream(a):
            knn_points(tiny, tiny, K=1)  # a new shape: one entry too many, the cache drops everything
            assert not (real | {("filler", 0)}) & set(_common._LENGTHS_CACHE), "the cache did not evict"
            refill = [torch.full((n,), 1, dtype=torch.int64, device=dev) for _ in range(64)]
        assert not delay_over.query(), "the delay on stream b had ended when the calls returned: it proved nothing"
        a.synchronize()
        b.synchronize()
        del refill
        _check_default_lengths("knn", oracle, x, y, out_b, "on stream b across the eviction")
    finally:
        torch.cuda.synchronize(dev)
        _common._LENGTHS_CACHE.clear()


def test_default_lengths_cache_properties(dev):
    """What the cache must keep while being safe across streams: one tensor object for both sides of a self-query, the
    same object call after call on one stream (no fill launch, no allocation), nothing cached from a capture."""
    from pytorch3d_pointops_amd.functions import _common

    a, _ = _streams(dev)
    _common._LENGTHS_CACHE.clear()
    try:
        pts = torch.from_numpy(sc.cases.cloud(6401, (2, 321, 3))).to(dev)
        p1, p2, l1, l2 = _common.point_pair(pts, pts, None, None)
        assert p1 is p2 and l1 is l2
        assert _common.full_lengths(2, 321, dev) is l1 and len(_common._LENGTHS_CACHE) == 1
        with torch.cuda.stream(a):
            on_a = _common.full_lengths(2, 321, dev)
            assert on_a is not l1 and _common.full_lengths(2, 321, dev) is on_a
        a.synchronize()
        assert torch.equal(on_a, l1) and bool((l1 == 321).all())
        before = dict(_common._LENGTHS_CACHE)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = _common.full_lengths(2, 323, dev)
        assert dict(_common._LENGTHS_CACHE) == before  # (a graph-pool tensor, filled by a replay only)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert bool((captured == 323).all())
    finally:
        _common._LENGTHS_CACHE.clear()


# ---------------------------------------------------------------------------------------------- C. two streams at once
_PAIRS = [("chamfer_overlap", "chamfer_overlap"), ("chamfer_overlap_full", "chamfer_small"),
          ("knn_refined", "knn_refined"), ("knn_small", "ball_small"), ("fps_small", "knn_gather"),
          ("sample_pdf", "packed_padded"), ("knn_backward_atomic", "chamfer_small_full"),
          ("knn_grid_k40", "ball_grid"), ("fps_cluster_full", "knn_scan")]


@pytest.mark.parametrize("first,second", _PAIRS, ids=["+".join(p) for p in _PAIRS])
def test_two_streams_at_once(dev, oracle, first, second):
    """Two entries on two streams, each behind its own delay, on different data and with no synchronisation between
    them.  (Two overlap chamfers share the library's one side stream and event pair; the multi-workgroup FPS stays
    out: its exchange needs all of its workgroups resident, and its timeout path has a test of its own.)"""
    a, b = _streams(dev)
    assert sc.TABLE[first].concurrent and sc.TABLE[second].concurrent
    _run_behind_delays([_Job(sc.TABLE[first], 0, a, oracle), _Job(sc.TABLE[second], 2, b, oracle)])


def test_two_streams_share_a_target_under_grid_reuse(dev, oracle):
    """set_grid_cache(True) keys a cached grid on the stream: the SAME target tensors searched on two streams, each
    behind a delay, must give each stream a workspace of its own (two misses) -- a hit on the second stream would
    search a grid the first has not built yet."""
    import pytorch3d_pointops_amd as pa
    from pytorch3d_pointops_amd import _C

    entry = sc.TABLE["knn_refined"]
    a, b = _streams(dev)
    data, static = entry.tensors(0, oracle, dev)
    pa.set_grid_cache(True)
    try:
        _call(entry, data, static)  # default stream: first launches (and an entry of its own, evicted below)
        torch.cuda.synchronize(dev)
        before = dict(_C.grid_cache_stats)
        outs, events = [], []
        for s in (a, b):
            with torch.cuda.stream(s):
                _delay(dev, DELAY_MS * 2)
                events.append(torch.cuda.Event())
                events[-1].record(s)
                outs.append(_call(entry, data, static))
        assert not any(e.query() for e in events), "a delay had ended when the calls returned: this run proved nothing"
        after = dict(_C.grid_cache_stats)
        assert (after["miss"], after["points"], after["both"]) == (before["miss"] + 2, before["points"], before["both"])
        keys = list(_C._GRID_CACHE)
        assert len(keys) == 2 and {k[3] for k in keys} == {a.cuda_stream, b.cuda_stream}
        ws = [_C._GRID_CACHE[k]["ws"] for k in keys]
        assert ws[0].data_ptr() != ws[1].data_ptr()
        with torch.cuda.stream(a):
            outs.append(_call(entry, data, static))  # the same stream again: now the grid is reused
        assert _C.grid_cache_stats["both"] == before["both"] + 1
        torch.cuda.synchronize(dev)
        for o, what in zip(outs, ("on stream a", "on stream b", "on stream a, grid reused")):
            _assert_matches(entry, 0, oracle, o, what)
    finally:
        torch.cuda.synchronize(dev)
        pa.set_grid_cache(False)


# ------------------------------------------------------------------------------------ D. a device that is not current
def _second_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: all tensors on cuda:1 while cuda:0 is the current device")
    return torch.device("cuda:1")


def _assert_on(device):
    def check(outs):
        assert torch.cuda.current_device() == 0
        assert all(o.device == device for o in outs), [o.device for o in outs]
    return check


@pytest.mark.parametrize("name", NAMES)
def test_device_that_is_not_current(dev, oracle, name):
    """All tensors on cuda:1 while cuda:0 is current: on the default stream of cuda:1, then behind a delay on a side
    stream of cuda:1.  Bit-reproducible operators must give what cuda:0 gives on the same inputs."""
    other = _second_device()
    assert torch.cuda.current_device() == 0
    job = _Job(sc.TABLE[name], 0, _streams(other)[0], oracle, on_outputs=_assert_on(other))
    assert torch.cuda.current_device() == 0
    _run_behind_delays([job])
    assert torch.cuda.current_device() == 0 and all(o.device == other for o in job.outs)


def test_large_lds_kernels_on_the_second_device_a_process_touches(dev, oracle):
    """The kernels that raise their dynamic-LDS limit above 64 KB (the 128 KB refine kernel, the long-list wide kernel)
    on cuda:0 FIRST and on cuda:1 second: the limit is set once per device, not once per process."""
    other = _second_device()
    for name in ("knn_refined", "knn_wide_k300", "knn_wide_k100"):
        entry = sc.TABLE[name]
        for device in (dev, other):
            data, static = entry.tensors(0, oracle, device)
            outs = _call(entry, data, static)
            torch.cuda.synchronize(device)
            _assert_matches(entry, 0, oracle, outs, f"on {device}")
            if entry.prove is not None:
                entry.prove({**data, **static})
    assert torch.cuda.current_device() == 0


def test_mixed_devices_raise(dev):
    from pytorch3d_pointops_amd.functions import knn_points

    other = _second_device()
    x = torch.from_numpy(sc.cases.cloud(6501, (1, 64, 3)))
    with pytest.raises(RuntimeError, match="same GPU device"):
        knn_points(x.to(dev), x.to(other), K=2)
    with pytest.raises(RuntimeError, match="same GPU device"):
        knn_points(x.to(other), x.to(other), lengths1=torch.full((1,), 64, dtype=torch.int64, device=dev), K=2)


def test_graph_capture_on_the_device_that_is_not_current(dev, oracle):
    from pytorch3d_pointops_amd import graphs

    other = _second_device()
    entry = sc.TABLE["knn_small"]
    data, static = entry.tensors(0, oracle, other)
    step = graphs.capture(lambda p1, p2: _call(entry, dict(p1=p1, p2=p2), static), (data["p1"], data["p2"]))
    assert torch.cuda.current_device() == 0
    _assert_matches(entry, 0, oracle, step(), "replayed on cuda:1")
    fresh, _ = entry.tensors(2, oracle, other)
    outs = step(fresh["p1"], fresh["p2"])
    torch.cuda.synchronize(other)
    assert torch.cuda.current_device() == 0 and all(o.device == other for o in outs)
    _assert_matches(entry, 2, oracle, outs, "replayed on cuda:1 on new data")
