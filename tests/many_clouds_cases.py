"""Batches of 32 768 to 70 000 tiny clouds: the inputs of test_many_clouds_cpu.py / test_many_clouds_gpu.py.

N, the number of clouds, is launch geometry: kernels read the cloud from blockIdx.y (limit 65 535), fold it into
blockIdx.x, or are run in slices of 32 768 or 65 535 clouds.  The way such code goes wrong is aliasing -- cloud n served
as cloud n mod 32 768 or n mod 65 536, tail clouds never written, the wrong lengths[n] read -- so every cloud here has
content of its own:

* lengths come from a per-cloud hash over 0..Pmax and are then SEPARATED: lengths[n] differs from lengths[n - 32768]
  and from lengths[n - 65536] on both sides (empty and full clouds occur; the last cloud is never empty);
* points are seeded random fp32, or a 0.25 lattice (distance ties, distances exactly on a radius^2) on every 5th cloud;
  32768 % 5 = 3 and 65536 % 5 = 1, so a lattice cloud's aliases are random clouds.

Everything is a counter hash of the cloud index (synth.splitmix64), so batch(N) is a prefix of batch(N') for N < N'
except for the last-cloud repair.  test_many_clouds_cpu.py ASSERTS the separation; nothing relies on it unchecked.
"""
import numpy as np

import scatter_ref
from pytorch3d_pointops_amd import synth

SLICE = 32768   # clouds per launch of the sliced grid search (csrc/knn_grid.hip)
GRID_Y = 65536  # first cloud count that no longer fits blockIdx.y
EDGE_NS = (65535, 65536, 65537)
SLICE_NS = (32768, 32769, 65537)  # one, two and three slices
ALL_NS = (32768, 32769, 65535, 65536, 65537)
N_BIG = 70000


def _hash(seed, N):
    """One uint64 per cloud index (independent of N)."""
    return synth.splitmix64(seed, N) >> np.uint64(11)


def separated_lengths(seed, N, Pmax):
    """(N,) int64 in [0, Pmax], hashed per cloud, with lengths[n] != lengths[n - 32768] and != lengths[n - 65536];
    the last cloud is non-empty.  Needs Pmax >= 3."""
    assert Pmax >= 3 and N <= 3 * SLICE
    M = Pmax + 1
    h =[_hash(seed + 7919 * b, SLICE).astype(np.int64) for b in range(3)]
    a = h[0] % M
    b = (a + 1 + h[1] % Pmax) % M  # != a
    c = h[2] % (M - 2)             # the c-th value of [0, Pmax] without a and b
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    c = c + (c >= lo)
    c = c + (c >= hi)
    out = np.concatenate([a, b, c])[:N].astype(np.int64)
    if out[N - 1] == 0:  # the last cloud has rows: a launch that drops the tail cannot hide behind an empty cloud
        taken = {int(out[N - 1 - s]) for s in (SLICE, GRID_Y) if N - 1 - s >= 0}
        out[N - 1] = next(v for v in range(1, M) if v not in taken)
    return out


def points(seed, N, P, D):
    """(N, P, D) fp32: uniform [0, 1) clouds; every 5th cloud on the 0.25 lattice {0, .25, .5, .75}^D.  All P rows have
    content, whatever the cloud's length."""
    p = synth.uniform_f32(seed, (N, P, D))
    lat = synth.randint(seed + 1, 0, 3, (N, P, D)).astype(np.float32) * np.float32(0.25)
    p[::5] = lat[::5]
    return np.ascontiguousarray(p, dtype=np.float32)


_MEMO = {}


def batch(N, D=3, P1=6, P2=10, seed=1000):
    """dict(p1 (N,P1,D), p2 (N,P2,D), l1, l2): queries of up to P1 (4..8) rows, targets of up to P2 (8..12).  Memoised:
    the arrays are shared between tests and must not be written."""
    key = (N, D, P1, P2, seed)
    if key not in _MEMO:
        assert 4 <= P1 <= 8 and 8 <= P2 <= 12, "the issue's cloud sizes"
        _MEMO[key] = dict(p1=points(seed, N, P1, D), p2=points(seed + 10, N, P2, D),
                          l1=separated_lengths(seed + 20, N, P1), l2=separated_lengths(seed + 30, N, P2))
    return _MEMO[key]


def probe_set(N, seed=77):
    """Sorted cloud indices where a per-cloud Python reference is affordable: the first 8, both sides of 32 768 and of
    65 536 (as far as N reaches), the last 8 and 64 drawn by seed."""
    want = list(range(8)) + list(range(32760, 32776)) + list(range(65527, 65544)) + list(range(N - 8, N))
    want += [int(v) for v in synth.randint(seed, 0, N - 1, (64,))]
    return np.array(sorted({n for n in want if 0 <= n < N}), np.int64)


def fps_k(N, P):
    """Per-cloud K in [0, P + 2]: zero, below, at and above the length."""
    return synth.randint(4242, 0, P + 2, (N,))


def fps_start(lengths):
    return synth.randint(4243, 0, 1 << 20, lengths.shape) % np.maximum(lengths, 1)


def packed_of(padded, lengths):
    """(packed (F, D), first_idxs, F) holding the valid rows of `padded`."""
    valid = np.arange(padded.shape[1])[None, :] < lengths[:, None]
    first = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    return np.ascontiguousarray(padded[valid]), first, int(lengths.sum())


def gapped_first_idxs(lengths, every=3):
    """(first_idxs, F) of a packed layout in which every `every`-th cloud is followed by one row owned by no cloud and
    the first row belongs to nobody either.  Cloud b owns [first[b], first[b + 1]) (the last: to F), so an owner-less
    row shows as a cloud whose range is LONGER than max_size: callers pass max_size = the true maximum and the
    converters clamp, which is what makes rows past it owner-less."""
    gaps = (np.arange(len(lengths)) % every == 0).astype(np.int64)
    sizes = lengths + gaps
    first = 1 + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return first, int(1 + sizes.sum())


def packed_to_padded_np(x, first, max_size):
    """numpy restatement of packed_to_padded (reference: packed_to_padded_tensor_cpu.cpp:11-40): cloud b takes rows
    [first[b], first[b + 1]) (the last: to F), at most max_size of them; the rest of its rows are zero."""
    F, B = x.shape[0], len(first)
    end = np.concatenate([first[1:], [F]])
    num = np.minimum(end - first, max_size)
    col = np.arange(max_size)[None, :]
    valid = col < num[:, None]
    src = np.where(valid, first[:, None] + col, 0)
    return np.where(valid.reshape(B, max_size, *([1] * (x.ndim - 1))), x[src], 0).astype(x.dtype)


def padded_to_packed_np(padded, first, F):
    """numpy restatement of padded_to_packed (same file :42-70): zeros, then every cloud's rows copied to its range."""
    B, max_size = padded.shape[:2]
    end = np.concatenate([first[1:], [F]])
    num = np.minimum(end - first, max_size)
    valid = np.arange(max_size)[None, :] < num[:, None]
    out = np.zeros((F,) + padded.shape[2:], padded.dtype)
    out[(first[:, None] + np.arange(max_size)[None, :])[valid]] = padded[valid]
    return out


# ------------------------------------------------------------------------------------------ failure messages
def first_bad(bad):
    """`bad`: boolean array whose FIRST axis is the cloud.  '' when nothing is set, else the first failing cloud with
    its residues: an aliased launch is readable from them at once."""
    bad = np.asarray(bad)
    per = bad.reshape(bad.shape[0], -1).any(1) if bad.ndim > 1 else bad
    if not per.any():
        return ""
    n = int(np.argmax(per))
    return (f"first failing cloud n = {n} (n % 32768 = {n % SLICE}, n % 65536 = {n % GRID_Y}); "
            f"{int(per.sum())} of {per.size} clouds differ")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_clouds_equal(got, want, what, as_bits=False, clouds=None):
    """Equality of two arrays whose first axis is the cloud (`clouds`: the cloud index of each row when the arrays are
    a subset), with the first failing cloud in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (bits(got) != bits(want)) if as_bits else (got != want)
    msg = first_bad(bad)
    if msg and clouds is not None:
        n = int(np.asarray(clouds)[int(np.argmax(bad.reshape(bad.shape[0], -1).any(1)))])
        msg = f"first failing cloud n = {n} (n % 32768 = {n % SLICE}, n % 65536 = {n % GRID_Y}) of the probe set"
    assert not msg, f"{what}: {msg}"


def assert_clouds_close(got, want, tol, what, clouds=None):
    """|got - want| <= tol elementwise (tol broadcastable), first axis the cloud."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bad = ~(err <= tol)
    if bad.any():
        row = int(np.argmax(bad.reshape(bad.shape[0], -1).any(1)))
        n = row if clouds is None else int(np.asarray(clouds)[row])
        raise AssertionError(f"{what}: first failing cloud n = {n} (n % 32768 = {n % SLICE}, n % 65536 = {n % GRID_Y}),"
                             f" max |err| = {float(np.nanmax(err)):g}, {int(bad.sum())} elements outside the bar")


# ------------------------------------------------------------------------------------------ exact scatter inputs
def exact_knn_backward_inputs(N, D, L=6, M=10, K=4, norm=2, seed=3000):
    """Inputs of knn_points_backward on scatter_ref's EXACT lattice (coordinates multiples of 0.25 in [0, 1], integer
    gradients in [-4, 4]) with scatter_ref.table's neighbour table (hub rows, -1 padding) and this file's separated
    lengths.  scatter_ref's precondition max A < 2^22 is asserted, so every plan must return the float64 sum cast to
    fp32 bit for bit."""
    rng = np.random.default_rng(seed)
    p1 = (rng.integers(0, 5, (N, L, D)) * 0.25).astype(np.float32)
    p2 = (rng.integers(0, 5, (N, M, D)) * 0.25).astype(np.float32)
    grad = rng.integers(-4, 5, (N, L, K)).astype(np.float32)
    idx = scatter_ref.table(seed, N, L, K, M, scatter_ref.tile_rows(min(D, 4)))
    l1, l2 = separated_lengths(seed + 1, N, L), separated_lengths(seed + 2, N, M)
    ref = scatter_ref.knn_backward_ref(p1, p2, l1, l2, idx, norm, grad)
    scatter_ref._assert_exact(ref.A1, "many clouds (grad_p1)")
    scatter_ref._assert_exact(ref.A2, "many clouds (grad_p2)")
    return p1, p2, l1, l2, idx, grad, ref


def exact_gather_backward_inputs(N, C, L=6, M=10, K=4, with_lengths=True, seed=3100):
    rng = np.random.default_rng(seed)
    grad_out = rng.integers(-4, 5, (N, L, K, C)).astype(np.float32)
    idx = scatter_ref.table(seed, N, L, K, M, scatter_ref.tile_rows(min(C, 4)))
    lengths = separated_lengths(seed + 2, N, M) if with_lengths else None
    ref = scatter_ref.gather_backward_ref(grad_out, idx, lengths, M)
    scatter_ref._assert_exact(ref.A, "many clouds (gather)")
    return grad_out, idx, lengths, ref
